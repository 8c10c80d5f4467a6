"""The host side of the streaming drain (csrc/engine/drain_pipeline.hpp: the gc files of a pass, the MAC / copy workers behind their
segment queue, the BLAKE3 absorbers), alone and without a device: tests/drain_pipeline/drain_pipeline_test.cpp includes the header and
defines the hip* functions it calls itself.  Those stand-ins model asynchrony — a copy only moves its bytes when its stream, or an event
recorded behind it, is synchronised — and fail a copy on request.  Cases: a ragged last group over segments that are no multiple of the
chunk / empty / shorter than a chunk / several chunks, with MAC, files and callback together (groups of 4, 1 and, with VAES, 16); buffer
recycling at depth 1 and 2; two slices chaining over the same MAC states and appended files; a failing sink; a failing copy; no segment at
all; the absorbers.  A deadlock is a failure, not a hang: the program runs under a time limit."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "drain_pipeline")


def test_drain_pipeline_against_asynchronous_stand_ins():
    subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "drain_pipeline_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("drain_pipeline: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
