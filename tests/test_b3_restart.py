"""The host half of a restart point of a sliced, verified evaluation (csrc/engine/outboard.hpp: B3Check.position / rewind / holds;
host_crypto.hpp: Blake3Host kept by value), alone and without a device: tests/drain_pipeline/b3_restart_test.cpp models the device half
of a B3Stream on the host (open chunk, pending chunk values, chunks done) for three streams with real outboards and uneven segments.
At every segment boundary the receiver is saved, advanced over a stream with one flipped bit until the comparison stops it (or, for a
bit in the last chunk, until the digest differs), restored and advanced over the clean stream, twice: the comparison's positions and
the digests are the straight run's.  Shapes: 1 665 records at k = 2 (saves while a group is open, and while two chunk values are pending
at the end), the same cut on group boundaries, k = 0, the small plan's 775 records in its four windows at k = 1, a single chunk."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "drain_pipeline")


def test_check_and_hashers_saved_mid_stream_and_restored():
    subprocess.check_call(["make", "-C", DIR, "-f", "b3_restart.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "b3_restart_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("b3_restart: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the headers alone: no HIP runtime, no engine library
