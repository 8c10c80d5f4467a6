"""What a streaming garble refuses, and that a refusal leaves the session as good as new: the rules on the destinations of a pass
(drain_pipeline.hpp: DrainSink::refusal, commit_slice_conflict) and the call range of a program session, through the C entry points.

The texts are pinned as literals.  The Python wrappers refuse most of these combinations themselves (ValueError), so the sink rules and
the call ranges go to the library directly.  Nothing here provokes a device fault: every refused call returns before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SAME_B3 = "every slice of a pass with a BLAKE3 commitment must ask for the same commitments as its first slice"
SAME_MCK = "every slice of a pass that writes or checks CBC-MAC checkpoints must ask for the same as its first slice"
ONE_PASS = "program sessions are garbled in one pass (first_call = n_calls = 0)"
NEEDS_B3_OUTBOARD = "an outboard holds the values of the BLAKE3 commitment: blake3_digests must be given"
NEEDS_B3_LAST = "the last chunks come with the BLAKE3 commitment: blake3_digests must be given"
NO_HASHES = "null hash buffer"  # (what gsv_session_garble_streaming_checkpoints answers a checkpoint directory without hashes with)
RING = ("CBC-MAC checkpoints are not written or checked over a ciphertext ring (retain_stream = GSV_STREAM_RING): "
        "create the session with launch windows")


def _refused(gsv, rc, text):
    assert rc == 1, "status %d: %s" % (rc, gsv.lib().gsv_last_error().decode())
    assert gsv.lib().gsv_last_error().decode() == text


def _plan_inputs(gsv, sp, P, seeds):
    labs = [P.labels(gsv, sp, s) for s in seeds]
    return np.stack([x[0] for x in labs]), np.stack([x[1] for x in labs]), np.stack([x[2] for x in labs])


def _mck(gsv, d, n):
    return [open(os.path.join(d, gsv.checkpoint_file_name(i)), "rb").read() for i in range(n)]


def test_slices_must_carry_the_commitments_of_the_first(engine, monkeypatch, tmp_path):
    """The small plan in at least three windows, three instances.  A middle slice that asks for other commitments than slice 0 is
    refused with the rule it breaks; the whole pass from call 0 then returns what a fresh session returns."""
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    n_ct = sp.plan.info["n_ciphertexts"]
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", "1")
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "1")   # groups of 128 records
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", "6")    # ... and of 64: several per stream
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")  # (a stall would end the pass with an error after seconds, not a minute)
    assert n_ct > 4 * 128
    seeds = [T.SEED0 + i for i in range(3)]
    macs_want = [P.reference(gsv, sp, s)[0].ct_hash for s in seeds]
    opts = dict(retain_stream=False, window_ct_records=n_ct // 4, drain_segment_records=n_ct // 8)
    dirs = {q: str(tmp_path / q) for q in ("fresh", "slice", "again")}
    for q in dirs.values():
        os.mkdir(q)
    fresh = gsv.Session(engine, sp.plan, 3, **opts)
    fresh.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    macs, digests = fresh.garble_streaming(commitment="both")
    assert macs == macs_want and len(digests) == 3
    fresh.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert fresh.garble_streaming(directory=dirs["fresh"], checkpoint_dir=dirs["fresh"]) == macs
    fresh.close()
    files = _mck(gsv, dirs["fresh"], 3)
    assert len(files[0]) > 24 + 3 * 16

    sess = gsv.Session(engine, sp.plan, 3, **opts)
    w = sess.windows()
    assert len(w) >= 3
    c1, c2 = w[1][0], w[2][0]
    assert 0 < c1 < c2 < sess.schedule_info()["n_calls"]
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_calls(0, c1, commitment="blake3") is None
    with pytest.raises(gsv.GsvError) as ei:
        sess.garble_calls(c1, c2 - c1)  # without the digests: the BLAKE3 state would miss this slice
    assert str(ei.value) == "gsv status 1: " + SAME_B3
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_streaming(commitment="both") == (macs, digests)

    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    sess.garble_calls(0, c1, directory=dirs["slice"], checkpoint_dir=dirs["slice"])
    with pytest.raises(gsv.GsvError) as ei:
        sess.garble_calls(c1, c2 - c1, directory=dirs["slice"])  # without the checkpoint files
    assert str(ei.value) == "gsv status 1: " + SAME_MCK
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_streaming(directory=dirs["again"], checkpoint_dir=dirs["again"]) == macs
    assert _mck(gsv, dirs["again"], 3) == files
    for i in range(3):
        assert gsv.read_gc_file(os.path.join(dirs["again"], gsv.gc_file_name(i)))[1] == macs[i]
    assert sess.fallback_count() == 0
    sess.close()


def _layered_session(gsv, engine):
    import test_blake3_evaluate as E
    p = E._layered()
    sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    return p, sess


def _buf(n):
    a = np.zeros(n, np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_call_range_on_a_program_session(engine, tmp_path):
    """first_call = 1 on a program session: four of the five entry points refuse it, gsv_session_garble_streaming_sink runs the pass."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    L = gsv.lib()
    p, sess = _layered_session(gsv, engine)
    d = os.fsencode(str(tmp_path))
    (_, macs), (_, dig) = _buf(3 * 16), _buf(3 * 32)
    no_ct, no_ob = gsv.CT_SINK_FN(), gsv.OUTBOARD_SINK_FN()
    _refused(gsv, L.gsv_session_garble_streaming_commit_outboard(sess.h, 0, 1, 0, None, 0, 0, macs, dig, None), ONE_PASS)
    _refused(gsv, L.gsv_session_garble_streaming_checkpoints(sess.h, 0, 1, 0, None, 0, 0, macs, d), ONE_PASS)
    _refused(gsv, L.gsv_session_garble_streaming_check(sess.h, 0, 1, 0, d, None, 0, None, macs), ONE_PASS)
    _refused(gsv, L.gsv_session_garble_streaming_sink_commit(sess.h, 0, 1, 0, no_ct, None, 0, macs, dig, no_ob, None, None), ONE_PASS)
    assert os.listdir(str(tmp_path)) == []
    got = [[] for _ in range(3)]
    out = sess.garble_to_sink(lambda i, first, recs: got[i].append((first, recs.copy())), first_call=1, n_calls=0, threads=2, with_hashes=True)
    for i in range(3):
        runs = sorted(got[i], key=lambda x: x[0])
        assert [f for f, _ in runs] == list(np.cumsum([0] + [len(r) for _, r in runs[:-1]]))
        assert (np.concatenate([r for _, r in runs]) == p["refs"][i]).all()
        assert out[i] == o.cbcmac(p["refs"][i])
    sess.close()


def test_sink_rules(engine, monkeypatch, tmp_path):
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    import plan_small_lib as P
    import test_plan_small as T
    L = gsv.lib()
    p, sess = _layered_session(gsv, engine)
    d = os.fsencode(str(tmp_path))
    (_, macs), (_, last) = _buf(3 * 16), _buf(3 * 1024)
    no_ct, no_ob = gsv.CT_SINK_FN(), gsv.OUTBOARD_SINK_FN()
    ob = gsv.OUTBOARD_SINK_FN(lambda *a: 1)
    _refused(gsv, L.gsv_session_garble_streaming_commit_outboard(sess.h, 0, 0, 0, None, 0, 0, macs, None, d), NEEDS_B3_OUTBOARD)
    _refused(gsv, L.gsv_session_garble_streaming_sink_commit(sess.h, 0, 0, 0, no_ct, None, 0, macs, None, ob, None, None), NEEDS_B3_OUTBOARD)
    _refused(gsv, L.gsv_session_garble_streaming_sink_commit(sess.h, 0, 0, 0, no_ct, None, 0, macs, None, no_ob, None, last), NEEDS_B3_LAST)
    _refused(gsv, L.gsv_session_garble_streaming_checkpoints(sess.h, 0, 0, 0, None, 0, 0, None, d), NO_HASHES)
    assert os.listdir(str(tmp_path)) == []
    assert sess.garble_streaming() == [o.cbcmac(r) for r in p["refs"]]  # the session is as good as new
    sess.close()
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", "1")
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    seeds = [T.SEED0 + i for i in range(3)]
    ring = gsv.Session(engine, sp.plan, 3, retain_stream="ring", concurrent_calls=8, drain_segment_records=sp.plan.info["n_ciphertexts"] // 4)
    ring.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    with pytest.raises(gsv.GsvError) as ei:
        ring.garble_streaming(checkpoint_dir=str(tmp_path))
    assert str(ei.value) == "gsv status 1: " + RING
    assert os.listdir(str(tmp_path)) == []
    ring.close()
