"""CBC-MAC checkpoints without a device, in a stand-alone program (tests/mac_checkpoints/mac_checkpoints_test.cpp, built under the address
and undefined-behaviour sanitizers): the drain-side CheckpointWriter behind the MAC workers against asynchronous stand-ins for the HIP
calls — segments that are no multiple of the chunk, empty segments, segments shorter than a group, groups of 4 and 1 chains, two slices
appending to the same files, byte-identical to the file writer's output — the format code (files of one call that disagree on k or
n_records), and the chain bookkeeping the device kernel runs, here with PlainTables over the GPU tests' segmentations.  A deadlock is a
failure, not a hang: the program runs under a time limit."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "mac_checkpoints")


def test_checkpoint_writer_and_chain_bookkeeping_stand_alone(tmp_path):
    subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "mac_checkpoints_test")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("mac_checkpoints: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the headers alone: no HIP runtime, no engine library
