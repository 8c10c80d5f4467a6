"""CtUploader (csrc/engine/upload_pipeline.hpp) started at a record other than 0, as a later slice of a sliced evaluation starts it, alone
and without a device: tests/upload_pipeline/upload_resume_test.cpp against the asynchronous HIP stand-ins of tests/hip_standin.  Streams
of 7, 8, 9, 17, 40 and 41 records around a chunk of 8 (the engine's is 16 MiB) in segments of 19, read from files (GcFileSource, opened
per slice) and through a callback reader, with 0 and 2 MAC workers.  For every pair of cut points a <= b: the bytes staged and the MAC
folded over [a, b) and then — by a fresh uploader that takes the first one's states — over [b, n) equal those of one read over [a, n),
the stream's own bytes and its serial MAC from record 0, and nothing in front of `a` is read.  A file that ends early is reported with
the absolute first record of the chunk whose read failed; an upload that does not follow the stream is refused before anything is read."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "upload_pipeline")


def test_uploader_started_in_the_middle_of_the_stream():
    subprocess.check_call(["make", "-C", DIR, "-f", "upload_resume.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "upload_resume_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("upload_resume: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
