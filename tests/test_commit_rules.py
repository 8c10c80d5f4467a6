"""What a streaming garble may combine, without a device (csrc/engine/drain_pipeline.hpp: DrainSink::commit, DrainSink::refusal,
commit_slice_conflict): tests/drain_pipeline/commit_rules_test.cpp runs all 2^9 combinations of the nine destinations, with and without
a ciphertext ring and an evaluator beside the garbler, against the rules written out on bit masks, and all 32 x 32 pairs of a first
slice's and a later slice's commitments against the two-line rule.  The refusal texts are pinned there as literals; tests/
test_garble_commit_rules.py meets them again through the C entry points on the device."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "drain_pipeline")


def test_every_combination_of_destinations_and_every_pair_of_slices():
    subprocess.check_call(["make", "-C", DIR, "-f", "commit_rules.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "commit_rules_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("commit_rules: ok (2048 sink cases, 1024 slice pairs)")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
