"""The schedule-dependent tables of a plan session and the policy that sizes its schedule, without a device (csrc/engine/plan_layout.hpp:
build_plan_layout, plan_sched_params): tests/plan_layout/plan_layout_test.cpp builds the tables of a hand-made plan of twelve calls for
the retained, windowed, ring and safe layouts and asserts their properties one by one, meets each of the three error returns with the
output left as it was, and pins the parameter policy with one case per clamp.  tests/test_engine_host.py executes the same tables gate by
gate against the oracle (test_scheduled_plan_matches_flat_stream)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "plan_layout")


def test_tables_errors_and_parameter_policy():
    subprocess.check_call(["make", "-C", DIR], stdout=subprocess.DEVNULL)
    exe = os.path.join(DIR, "plan_layout_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("plan_layout: ok (4 layouts with and without a withheld dependency, 3 errors, the parameter policy)")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed  # the header alone: no HIP runtime, no engine library
