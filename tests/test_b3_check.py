"""The receiver's side of the BLAKE3 outboards (csrc/engine/outboard.hpp: B3Check, check_outboard, load_outboard), alone and without a
device: tests/drain_pipeline/b3_check_test.cpp builds real outboards with the host writer for three streams of 1 665, 775, 64 and 0
records at k = 2 and 0 and feeds their values back in uneven batches.  Cases: everything matches; of two differences the lowest group,
then the lowest instance is blamed; a group too many, pending values too early or in the wrong number; a flipped pending value names
its record; the text of where(); reset(); and the refusals of check_outboard, in their order, with both sides named."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "drain_pipeline")


def test_b3_check_blames_the_first_difference_and_refuses_foreign_outboards():
    subprocess.check_call(["make", "-C", DIR, "-f", "b3_check.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "b3_check_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("b3_check: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
