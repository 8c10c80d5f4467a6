"""The file source of the streaming evaluator and of blake3_files (csrc/engine/upload_pipeline.hpp, GcFileSource: one gc file per
instance, read where the caller asks, seeking only when the position is not the expected one), alone and without a device:
tests/upload_pipeline/gc_file_source_test.cpp reads three files of distinct content.  Cases: the instances alternating at increasing
offsets; backwards and forwards jumps; n = 0; reads past the end fail and leave the source usable; a missing file names its path."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "upload_pipeline")


def test_gc_file_source_reads_where_asked_and_reports_short_files():
    subprocess.check_call(["make", "-C", DIR, "-f", "gc_file_source.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "gc_file_source_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("gc_file_source: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
