"""The two back ends of the drain-side outboard writer (csrc/engine/drain_pipeline.hpp, OutboardWriter: gc_<i>.b3o files and the host
callback behind gsv_session_garble_streaming_sink_commit), alone and without a device: tests/drain_pipeline/outboard_sink_test.cpp
drives both as the drain does — the header at the open, group values through the absorbers' threads, the pending chunk values from the
pass's own thread — with real values of streams made there.  Cases: callback bytes == file bytes == the host writer's outboard for
streams of 0, 1, 64, 65, 256, 257, 320 and 1 665 records at k = 0 and 2; two slices chaining (the header once, offsets going on); a
sample drain; a callback that fails (the pass fails, nothing further is delivered; a refused header fails the open); a failed call in
file mode removes its files.  A deadlock is a failure, not a hang: the program runs under a time limit."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "drain_pipeline")


def test_outboard_writer_back_ends_against_stand_ins():
    subprocess.check_call(["make", "-C", DIR, "-f", "outboard_sink.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "outboard_sink_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("outboard_sink: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
