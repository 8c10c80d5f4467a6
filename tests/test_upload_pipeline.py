"""The host side of the streaming evaluator (csrc/engine/upload_pipeline.hpp: the page-locked staging buffers a ciphertext source is read
into, the H2D copies out of them, the MAC pool beside them), alone and without a device: tests/upload_pipeline/upload_pipeline_test.cpp
includes the header and the HIP stand-ins of tests/hip_standin.  Those model asynchrony — a copy only moves its bytes when its stream, or
an event recorded behind it, is synchronised — and fail a copy on request.  Cases: placement in the gate-order buffer, chunk-major read
order and MACs over segments that are no multiple of the chunk / empty / shorter than a chunk / several chunks, with 0, 1, 2 and 5
workers (0: two staging buffers for fifteen reads); no segment at all and one chunk of one instance; a source that runs dry; a failing
copy with copies still queued when the uploader goes away; a second pass over the same source.  A deadlock is a failure, not a hang: the
program runs under a time limit."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "upload_pipeline")


def test_upload_pipeline_against_asynchronous_stand_ins():
    subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "upload_pipeline_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("upload_pipeline: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
