"""The move-only owners of csrc/engine/hip_owned.hpp (device buffers, page-locked host buffers, streams, events), alone and without a
device: tests/hip_owned/hip_owned_test.cpp includes the header and defines the hip* functions it calls itself, keeping the set of live
handles.  Those stand-ins abort on a handle released twice or never created; the program returns non-zero when a check fails or a handle
is still live at its end.  Cases: construct / destroy, move-construct, move-assign onto a live handle, reset twice, alloc over a live
buffer, failed creates (owner empty, the runtime's error cleared), std::vector growth, a shared image filed under two keys."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hip_owned")


def test_owners_release_every_handle_exactly_once():
    subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(DIR, "hip_owned_test")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("hip_owned: ok")
    needed = subprocess.check_output(["readelf", "-d", os.path.join(DIR, "hip_owned_test")], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
