"""Orders of creating and destroying sessions that the other GPU tests do not take (they create a session, run it, close it, and keep
their plans to the end of the process).  A session owns its buffers, streams and events and only LOOKS at the device images of its
programs, which belong to the programs: destroying a session in whatever state releases the former and must leave the latter alone.

  * sessions that never ran a pass — a program session, plan sessions with and without the stream retained — are destroyed; sessions
    created afterwards on the same program and plan run them;
  * two sessions on one plan: the first drains one instance's stream, then all five on the same session (the gate-order buffers, several
    of them, are released and re-allocated for the larger batch), and is destroyed first; the second runs after that; then it is
    destroyed and then the plan.

The synthetic plan of tests/plan_small_lib.py (~3.5 k gates), five instances, at one and four instances per workgroup.  Expected MACs and
output labels come from tests/gate_list_ref.py on the flat gate list, never from the engine."""
import numpy as np
import pytest

import gate_list_ref as G
import plan_small_lib as P
import test_kernel_step_shapes as S
from test_plan_small import KINDS, SEED0, small_plan

B = 5
LAYOUTS = [1, 4]


def _batch(gsv, sp):
    """(delta, consts, input label0s) of the B instances: instance i has seed SEED0 + i, whose reference test_plan_small shares."""
    labs = [P.labels(gsv, sp, SEED0 + i) for i in range(B)]
    return [np.stack([x[j] for x in labs]) for j in range(3)]


def _check(gsv, sp, what, macs, out0, n_drained=B):
    for i in range(B):
        g = P.reference(gsv, sp, SEED0 + i)[0]
        w = "%s, instance %d" % (what, i)
        assert macs[i] == (g.ct_hash if i < n_drained else bytes(16)), w + ": CBC-MAC"
        assert (out0[i] == g.output_label0).all(), w + ": output label0s"


def _garble_retained(gsv, sp, sess, what):
    sess.set_garble_inputs(*_batch(gsv, sp))
    sess.garble(0)
    sess.sync()
    _check(gsv, sp, what, [sess.ciphertext_hash(i) for i in range(B)], sess.read_outputs())


@pytest.mark.gpu
@pytest.mark.parametrize("ni", LAYOUTS)
def test_sessions_that_never_ran_are_destroyed(engine, monkeypatch, ni):
    gsv, sp = small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    gates, outputs, _ = S.build_layered([(20, 12), (9, 30), (33, 5)], n_inputs=16)
    prog = gsv.Program.from_gates(16, gates, outputs)
    gsv.Session(engine, prog, B).close()
    for kind in "ad":
        gsv.Session(engine, sp.plan, B, **KINDS[kind](sp)).close()
    sess = gsv.Session(engine, sp.plan, B, **KINDS["b"](sp))
    assert sess.instances_per_workgroup == ni
    _garble_retained(gsv, sp, sess, "plan session after three that never ran, %d per workgroup" % ni)
    sess.close()
    ps = gsv.Session(engine, prog, B)
    assert ps.instances_per_workgroup == ni
    labs = [gsv.labels_from_seed(40 + i, 16) for i in range(B)]
    ps.set_garble_inputs(np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
    ps.garble(0)
    ps.sync()
    out0 = ps.read_outputs()
    for i, (d, f, t, inp) in enumerate(labs):
        g = G.garble(gates, d, np.stack([f, t]), inp, outputs)
        assert ps.ciphertext_hash(i) == g.ct_hash and (out0[i] == g.output_label0).all(), "program session, instance %d, %d per workgroup" % (i, ni)
    ps.close()
    prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ni", LAYOUTS)
def test_two_sessions_of_a_plan_destroyed_in_creation_order_then_the_plan(engine, monkeypatch, ni):
    gsv, shared = small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    sp = P.build_small_plan(gsv)  # a plan of this test's own (it is destroyed below): the same flat list, so the shared references hold
    assert sp.flat == shared.flat and sp.outputs == shared.outputs and sp.inputs == shared.inputs
    first = gsv.Session(engine, sp.plan, B, **KINDS["d"](sp))
    second = gsv.Session(engine, sp.plan, B, **KINDS["a"](sp))
    assert first.instances_per_workgroup == second.instances_per_workgroup == ni and first.schedule_info()["n_segments"] >= 3
    what = "%d per workgroup" % ni
    first.set_drain_instances(1)
    first.set_garble_inputs(*_batch(gsv, shared))
    _check(gsv, shared, what + ", one instance drained", first.garble_streaming(), first.read_outputs(), n_drained=1)
    first.set_drain_instances(0)  # every instance: the gate-order buffers were sized for one
    first.set_garble_inputs(*_batch(gsv, shared))
    _check(gsv, shared, what + ", every instance drained by the same session", first.garble_streaming(), first.read_outputs())
    first.close()
    _garble_retained(gsv, shared, second, what + ", the second session after the first was destroyed")
    second.close()
    sp.plan.close()
