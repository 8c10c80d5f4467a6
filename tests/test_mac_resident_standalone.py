"""The CBC-MAC check of resident and sliced streams without a device, in a stand-alone program (tests/mac_resident/mac_resident_test.cpp,
built under the address and undefined-behaviour sanitizers and run directly): the indexed record accessor of the resident check against
the gathered stream — random n_ct, position tables, replay counts, range sizes and k, the same verdicts and the same carries as the plain
accessor, range by range —, save and restore of the check's host-side state in the middle of a stream, and which commitments and kinds
of verification a streaming evaluation may combine, slice after slice, as plain values."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "mac_resident")


def test_indexed_accessor_restore_and_commit_rules_stand_alone():
    subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "mac_resident_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("mac_resident: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the headers alone: no HIP runtime, no engine library
