"""BLAKE3 commitments, outboards and verified evaluation on the callback paths (include/gsv_engine.h "Commitments on the callback
paths"), on the device: the garbler hands ciphertexts to a handler and outboards to a second callback while it commits
(gsv_session_garble_streaming_sink_commit), the evaluator pulls the stream from a source and verifies it per group of chunks against
outboards held in memory (gsv_session_evaluate_streaming_source_verified) — with the last chunks up front, or deferred to the end of
the pass.

References: the reference streams and b3_ref's digests of test_blake3_evaluate's fixtures, gsv.cbcmac and gsv.blake3_file_outboard on
the host (checked against tests/b3_ref.py in test_blake3_outboard.py), and the directory path's gc_<i>.b3o.  GSV_B3_SUBTREE_LOG2=2
throughout: groups of 4 chunks = 256 records = 4 096 bytes.  A tampered stream is data: nothing here provokes a device fault."""
import ctypes as C
import os

import numpy as np
import pytest

import test_blake3_evaluate as E

pytestmark = pytest.mark.gpu
K = 2
N_PROGRAM = 1665  # records per instance of the layered program session: six groups, two pending chunk values, a last chunk of one record
# byte of instance 1 that is flipped -> (group, first_record) of the mismatch (test_blake3_verified.py's table); the last one lies in
# the last chunk, which no value of the outboard covers: the digest at the end of the pass does
TAMPER = ((5, 0, 0), (3 * 4096 + 100, 3, 3 * 256), (5 * 4096 + 50, 5, 5 * 256), (6 * 4096 + 1024 + 10, 6, 6 * 256 + 64), (1664 * 16 + 3, 6, 1664))
MODES = ("up_front", "deferred")


class Collector:
    """A CiphertextHandler that keeps the streams, and notes runs that arrive out of order"""

    def __init__(self, n_inst, n_records):
        self.streams = np.zeros((n_inst, n_records, 16), np.uint8)
        self.next = [0] * n_inst
        self.out_of_order = 0

    def __call__(self, inst, first, records):
        if first != self.next[inst]:
            self.out_of_order += 1
        self.streams[inst, first:first + len(records)] = records
        self.next[inst] = first + len(records)

    def complete(self):
        return self.out_of_order == 0 and all(x == self.streams.shape[1] for x in self.next)


class Source:
    """A CiphertextSource over streams held in memory; `flip` = (instance, byte) tampers with one bit on the way out, `dry` =
    (instance, record) makes the source run dry there"""

    def __init__(self, streams, flip=None, dry=None):
        self.streams, self.flip, self.dry = streams, flip, dry
        self.calls = 0
        self.highest = -1  # the highest record index asked for, over all instances

    def __call__(self, inst, first, n):
        self.calls += 1
        self.highest = max(self.highest, first + n - 1)
        if self.dry and inst == self.dry[0] and first + n > self.dry[1]:
            return None
        a = np.array(self.streams[inst][first:first + n], np.uint8).reshape(-1)
        if self.flip and inst == self.flip[0] and first * 16 <= self.flip[1] < (first + n) * 16:
            a[self.flip[1] - first * 16] ^= 0x10
        return a


def _mismatch(gsv, call):
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        call()
    assert "gsv status 5:" in str(ei.value)
    return ei.value


def _no_outputs(gsv, sess):
    with pytest.raises(gsv.GsvError, match="nothing ran"):
        sess.read_outputs()


def _host_outboard(gsv, tmp_path, stream):
    """(outboard bytes, digest) of a stream from the host writer"""
    gc, ob = str(tmp_path / "host.bin"), str(tmp_path / "host.b3o")
    gsv.write_gc_file(gc, stream)
    digest = gsv.blake3_file_outboard(gc, K, ob)
    return open(ob, "rb").read(), digest


_garbled = {}


def _program_garbled(gsv, engine):
    """The layered program garbled once through garble_to_sink(commitment="both", outboards=True): fixture, collected streams, the
    SinkCommit, the garbler's outputs.  (GSV_B3_SUBTREE_LOG2 is set by the caller.)"""
    if "p" not in _garbled:
        p = E._layered()
        sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
        sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
        col = Collector(3, N_PROGRAM)
        res = sess.garble_to_sink(col, commitment="both", outboards=True)
        out0 = sess.read_outputs()
        sess.close()
        assert col.complete()
        _garbled["p"] = (p, col.streams, res, out0)
    return _garbled["p"]


def _verified_kwargs(res, mode, expected=None, outboards=None):
    kw = dict(commitment="blake3", outboards=outboards if outboards is not None else res.outboards, expected=expected if expected is not None else res.blake3)
    if mode == "up_front":
        kw["last_chunks"] = res.last_chunks
    return kw


# ---- 1. garbler, program session -----------------------------------------------------------------------------------------------------
def test_garbler_program_session(engine, monkeypatch, tmp_path):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    p, streams, res, _ = _program_garbled(gsv, engine)
    assert isinstance(res, gsv.SinkCommit)
    assert gsv.blake3_outboard_size(N_PROGRAM, K) == (24 + 32 * 8, 16)
    for i in range(3):
        assert streams[i].tobytes() == p["refs"][i].tobytes()
        assert res.cbcmac[i] == gsv.cbcmac(streams[i])
        ob, digest = _host_outboard(gsv, tmp_path, streams[i])
        assert res.outboards[i] == ob and len(ob) == 24 + 32 * (6 + 2)
        assert res.last_chunks[i] == streams[i].tobytes()[-16:]
        assert gsv.blake3_outboard_root(res.outboards[i], res.last_chunks[i]) == res.blake3[i] == digest
    assert res.blake3 == p["want"]
    # no handler and BLAKE3 alone: nothing of the stream leaves the device, the commitment and the outboards are the same
    sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    alone = sess.garble_to_sink(None, commitment="blake3", outboards=True)
    assert alone.cbcmac is None and alone.blake3 == p["want"] and alone.outboards == res.outboards and alone.last_chunks == res.last_chunks
    # the CBC-MAC alone through the same entry point, and the call without a commitment as ever
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    macs = sess.garble_to_sink(Collector(3, N_PROGRAM), commitment="cbcmac")
    assert macs == gsv.SinkCommit(res.cbcmac, None, None, None)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    col = Collector(3, N_PROGRAM)
    assert sess.garble_to_sink(col, with_hashes=True) == res.cbcmac and col.complete() and (col.streams == streams).all()
    with pytest.raises(gsv.GsvError, match="gsv status 1: program sessions are garbled in one pass"):
        sess.garble_to_sink(col, first_call=0, n_calls=1, commitment="blake3")
    sess.close()


# ---- 2. garbler, plan session ---------------------------------------------------------------------------------------------------------
def _plan_setup(gsv, monkeypatch, ni):
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")
    return P, T, sp


def _b3o(gsv, d, i):
    return os.path.join(d, gsv.outboard_file_name(i))


def test_garbler_plan_session_whole_and_sliced(engine, monkeypatch, tmp_path):
    import garbled_snark_verifier_amd as gsv
    import test_blake3_commit as Cm
    P, T, sp = _plan_setup(gsv, monkeypatch, 1)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(3)]
    inputs = Cm._plan_inputs(gsv, sp, P, seeds)
    refs = [P.reference(gsv, sp, s)[0].ciphertexts for s in seeds]
    d = str(tmp_path)
    sess = gsv.Session(engine, sp.plan, 3, **E._plan_opts("windows", n_ct))
    sess.set_garble_inputs(*inputs)
    col = Collector(3, n_ct)
    whole = sess.garble_to_sink(col, commitment="both", outboards=True)
    assert col.complete() and all(col.streams[i].tobytes() == refs[i].tobytes() for i in range(3))
    assert whole.blake3 == [E.ref_digest(r.tobytes()) for r in refs]
    assert whole.cbcmac == [P.reference(gsv, sp, s)[0].ct_hash for s in seeds]
    last_bytes = gsv.blake3_outboard_size(n_ct, K)[1]
    assert whole.last_chunks == [r.tobytes()[-last_bytes:] for r in refs]
    # the directory path's outboards
    sess.set_garble_inputs(*inputs)
    assert sess.garble_streaming(commitment="blake3", outboard_dir=d) == whole.blake3
    assert whole.outboards == [open(_b3o(gsv, d, i), "rb").read() for i in range(3)]
    assert all(len(o) == gsv.blake3_outboard_size(n_ct, K)[0] for o in whole.outboards)
    # the same pass in slices at the window boundaries: nothing but the MAC states until the last one
    win = sess.windows()
    assert len(win) >= 2
    sess.set_garble_inputs(*inputs)
    col = Collector(3, n_ct)
    for j, (c0, nc, _) in enumerate(win):
        r = sess.garble_to_sink(col, first_call=c0, n_calls=nc, commitment="both", outboards=True)
        if j + 1 < len(win):
            assert r.blake3 is None and r.outboards is None and r.last_chunks is None and len(r.cbcmac) == 3
    assert r == whole and col.complete() and (col.streams == np.stack(refs)).all()
    # a slice that asks for other commitments than the first is refused
    sess.set_garble_inputs(*inputs)
    c0, nc, _ = win[0]
    assert sess.garble_to_sink(None, first_call=c0, n_calls=nc, commitment="blake3", outboards=True).blake3 is None
    c0, nc, _ = win[1]
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*same commitments"):
        sess.garble_to_sink(None, first_call=c0, n_calls=nc, commitment="blake3")
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*same commitments"):
        sess.garble_to_sink(None, first_call=c0, n_calls=nc, commitment="both", outboards=True)
    # an outboard callback that raises aborts the pass, and the exception comes back
    boom = RuntimeError("no room for outboards")
    calls = []

    def ob_sink(_user, inst, offset, _ptr, n_bytes):
        calls.append((int(inst), int(offset), int(n_bytes)))
        if len(calls) == 5:  # three headers and one value have been taken
            raise boom
        return 0

    sess.set_garble_inputs(*inputs)
    digests = np.full((3, 32), 0xAA, np.uint8)
    failure = []

    def guarded(*a):
        try:
            return ob_sink(*a)
        except BaseException as e:  # noqa: BLE001
            failure.append(e)
            return 1

    cb = gsv.OUTBOARD_SINK_FN(guarded)
    rc = gsv.lib().gsv_session_garble_streaming_sink_commit(sess.h, 0, 0, 0, gsv.CT_SINK_FN(), None, 0, None, gsv._p(digests), cb, None, None)
    assert rc == 1 and failure == [boom] and b"the outboard sink reported an error" in gsv.lib().gsv_last_error()
    assert calls[:3] == [(i, 0, 24) for i in range(3)] and (digests == 0xAA).all()  # the headers came first; nothing was written
    # no call was started after the refusal (the other absorber threads may have been in one at that moment: one per instance at the
    # most), so no instance has received its whole outboard
    total = gsv.blake3_outboard_size(n_ct, K)[0]
    assert 5 <= len(calls) <= 7 and all(off + n < total for _, off, n in calls)
    sess.close()


def test_garbler_python_outboard_callback_failure_is_reraised(engine, monkeypatch):
    """Through Session.garble_to_sink: an exception raised while the outboards are collected comes back as it is."""
    import garbled_snark_verifier_amd as gsv
    import test_blake3_commit as Cm
    P, T, sp = _plan_setup(gsv, monkeypatch, 1)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(3)]
    sess = gsv.Session(engine, sp.plan, 3, **E._plan_opts("windows", n_ct))
    sess.set_garble_inputs(*Cm._plan_inputs(gsv, sp, P, seeds))

    class Full(bytearray):
        def __iadd__(self, other):
            raise MemoryError("outboard store is full")

    win = sess.windows()
    c0, nc, _ = win[0]
    assert sess.garble_to_sink(None, first_call=c0, n_calls=nc, commitment="blake3", outboards=True).outboards is None
    sess._sink_outboards[1] = Full(sess._sink_outboards[1])
    c0, nc = win[1][0], sum(w[1] for w in win[1:])
    with pytest.raises(MemoryError, match="outboard store is full"):
        sess.garble_to_sink(None, first_call=c0, n_calls=nc, commitment="blake3", outboards=True)
    sess.close()


@pytest.mark.parametrize("ni", [1, 2, 4])
def test_garbler_plan_session_drained_sample(engine, monkeypatch, tmp_path, ni):
    """2 ni + 1 instances, two of them drained: two entries each, equal to the host writer's of the reference streams."""
    import garbled_snark_verifier_amd as gsv
    import test_blake3_commit as Cm
    P, T, sp = _plan_setup(gsv, monkeypatch, ni)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(2 * ni + 1)]
    part = gsv.Session(engine, sp.plan, len(seeds), **E._plan_opts("windows", n_ct))
    assert part.instances_per_workgroup == ni
    part.set_drain_instances(2)
    part.set_garble_inputs(*Cm._plan_inputs(gsv, sp, P, seeds))
    col = Collector(2, n_ct)
    r = part.garble_to_sink(col, commitment="both", outboards=True)
    assert col.complete() and [len(x) for x in r] == [2, 2, 2, 2]
    for i in range(2):
        ref = P.reference(gsv, sp, seeds[i])[0]
        assert col.streams[i].tobytes() == ref.ciphertexts.tobytes() and r.cbcmac[i] == ref.ct_hash
        ob, digest = _host_outboard(gsv, tmp_path, ref.ciphertexts)
        assert r.outboards[i] == ob and r.blake3[i] == digest == E.ref_digest(ref.ciphertexts.tobytes())
        assert gsv.blake3_outboard_root(r.outboards[i], r.last_chunks[i]) == digest
    assert part.fallback_count() == 0
    part.close()


# ---- 3. evaluator, both modes ---------------------------------------------------------------------------------------------------------
def _program_evaluator(gsv, engine, p):
    ev = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    return ev


def _outputs_ok(ev, out0, delta):
    act, ob = ev.read_outputs(with_bits=True)
    assert (act == np.where(ob[:, :, None] == 1, out0 ^ delta[:, None, :], out0)).all()
    return act, ob


@pytest.mark.parametrize("mode", MODES)
def test_evaluator_program_session(engine, monkeypatch, mode):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    p, streams, res, out0 = _program_garbled(gsv, engine)
    ev = _program_evaluator(gsv, engine, p)
    src = Source(streams)
    assert ev.evaluate_from_source(src, **_verified_kwargs(res, mode)) == res.blake3
    assert src.highest == N_PROGRAM - 1
    _outputs_ok(ev, out0, p["delta"])
    with pytest.raises(gsv.GsvError, match="no mismatch"):
        ev.mismatch_info()
    # 16-byte prefixes as commitments; "both" also returns the MACs
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    kw = _verified_kwargs(res, mode, expected=[x[:16] for x in res.blake3])
    kw["commitment"] = "both"
    assert ev.evaluate_from_source(Source(streams), **kw) == (res.cbcmac, res.blake3)
    _outputs_ok(ev, out0, p["delta"])
    ev.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ni", [1, 2, 4])
def test_evaluator_plan_session(engine, monkeypatch, ni, mode):
    """The small plan, 2 ni + 1 instances, one window per launch: garbled through the callbacks, evaluated from what they collected."""
    import garbled_snark_verifier_amd as gsv
    P, T, sp = _plan_setup(gsv, monkeypatch, ni)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(2 * ni + 1)]
    B = len(seeds)
    delta, consts, inputs, bits, active, consts_active = E._plan_case(gsv, sp, P, seeds)
    g = gsv.Session(engine, sp.plan, B, **E._plan_opts("windows", n_ct))
    g.set_garble_inputs(delta, consts, inputs)
    col = Collector(B, n_ct)
    res = g.garble_to_sink(col, commitment="both", outboards=True)
    out0 = g.read_outputs()
    g.close()
    assert col.complete() and res.blake3 == [E.ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    ev = gsv.Session(engine, sp.plan, B, **E._plan_opts("windows", n_ct))
    assert ev.instances_per_workgroup == ni
    info = ev.schedule_info()
    assert info["n_windows"] >= 2 and info["n_segments"] > info["n_windows"]
    ev.set_evaluate_inputs(consts_active, active, bits)
    kw = _verified_kwargs(res, mode)
    kw["commitment"] = "both"
    assert ev.evaluate_from_source(Source(col.streams), **kw) == (res.cbcmac, res.blake3)
    assert ev.schedule_info()["windows_launched"] == info["n_windows"]
    act, ob = _outputs_ok(ev, out0, delta)
    for i, s in enumerate(seeds):
        e = P.reference(gsv, sp, s)[1]
        assert (ob[i] == e.output_bits).all() and (act[i] == e.output_active).all(), "instance %d" % i
    ev.set_evaluate_inputs(consts_active, active, bits)
    assert ev.evaluate_from_source(Source(col.streams), **_verified_kwargs(res, mode, expected=[x[:16] for x in res.blake3])) == res.blake3
    # one flipped bit of instance 1 in the group that straddles the first window boundary: that window's successor is not launched
    counts = [int(r[3]) for r in sp.plan.call_info()]
    w1 = sum(counts[:ev.windows()[1][0]])
    grp = w1 // (64 << K)
    assert w1 % (64 << K) and (grp + 1) * (64 << K) <= n_ct
    ev.set_evaluate_inputs(consts_active, active, bits)
    e = _mismatch(gsv, lambda: ev.evaluate_from_source(Source(col.streams, flip=(1, (w1 + 3) * 16 + 7)), **_verified_kwargs(res, mode)))
    assert (e.instance, e.group, e.first_record) == (1, grp, grp * (64 << K)) == ev.mismatch_info()
    assert ev.schedule_info()["windows_launched"] == 1 < info["n_windows"]
    _no_outputs(gsv, ev)
    ev.set_evaluate_inputs(consts_active, active, bits)
    assert ev.evaluate_from_source(Source(col.streams), **_verified_kwargs(res, mode)) == res.blake3
    assert ev.fallback_count() == 0
    ev.close()


# ---- 4. tamper --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_tampered_source_is_stopped_and_named(engine, monkeypatch, mode):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    p, streams, res, out0 = _program_garbled(gsv, engine)
    ev = _program_evaluator(gsv, engine, p)
    for byte, group, record in TAMPER:
        src = Source(streams, flip=(1, byte))
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
        e = _mismatch(gsv, lambda: ev.evaluate_from_source(src, **_verified_kwargs(res, mode)))
        assert (e.instance, e.group, e.first_record) == (1, group, record), byte  # the other instances are never blamed
        assert ev.mismatch_info() == (1, group, record)
        assert "the ciphertext stream of instance 1 does not match its outboard in group %d (from record %d)" % (group, record) in str(e)
        assert "does not match the commitment" not in str(e)  # (the last byte too: a digest that differs at the end of the pass)
        _no_outputs(gsv, ev)
        if byte == 5:
            assert src.highest < N_PROGRAM - 1  # the source was never asked for the stream's last record
        if byte == TAMPER[-1][0]:
            assert src.highest == N_PROGRAM - 1  # ... while this one is found by the last look at the digests
        # the same session verifies the clean streams afterwards
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
        assert ev.evaluate_from_source(Source(streams), **_verified_kwargs(res, mode)) == res.blake3
        _outputs_ok(ev, out0, p["delta"])
    ev.close()


# ---- 5. what is refused before the source is called ------------------------------------------------------------------------------------
def test_up_front_refusals(engine, monkeypatch):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    p, streams, res, _ = _program_garbled(gsv, engine)
    ev = _program_evaluator(gsv, engine, p)
    wrong = [res.blake3[0], res.blake3[1], res.blake3[1]]
    src = Source(streams)
    e = _mismatch(gsv, lambda: ev.evaluate_from_source(src, **_verified_kwargs(res, "up_front", expected=wrong)))
    assert (e.instance, e.group, e.first_record) == (2, None, None) and "outboard or last chunk of instance 2 does not match the commitment" in str(e)
    assert src.calls == 0
    _no_outputs(gsv, ev)
    # the same commitment in deferred mode: the pass runs, ends with a mismatch, and returns no outputs
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    src = Source(streams)
    e = _mismatch(gsv, lambda: ev.evaluate_from_source(src, **_verified_kwargs(res, "deferred", expected=wrong)))
    assert (e.instance, e.group, e.first_record) == (2, 6, 1664) and src.highest == N_PROGRAM - 1
    _no_outputs(gsv, ev)

    def flipped(ob, byte, bit=0x10):
        b = bytearray(ob)
        b[byte] ^= bit
        return bytes(b)

    def with_1(ob):
        return [res.outboards[0], ob, res.outboards[2]]

    # a flipped group value: up front the outboard no longer folds to the commitment (GSV_ERR_MISMATCH without a place, as for the file path) ...
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    src = Source(streams)
    e = _mismatch(gsv, lambda: ev.evaluate_from_source(src, **_verified_kwargs(res, "up_front", outboards=with_1(flipped(res.outboards[1], 24 + 32 * 4 + 9)))))
    assert (e.instance, e.group) == (1, None) and src.calls == 0
    _no_outputs(gsv, ev)
    # ... deferred, the stream and the outboard disagree in that group
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    e = _mismatch(gsv, lambda: ev.evaluate_from_source(Source(streams), **_verified_kwargs(res, "deferred", outboards=with_1(flipped(res.outboards[1], 24 + 32 * 4 + 9)))))
    assert (e.instance, e.group, e.first_record) == (1, 4, 1024)
    _no_outputs(gsv, ev)
    # malformed outboards: GSV_ERR_INVALID with the file path's messages, in both modes, and the source is never called
    for mode in MODES:
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
        src = Source(streams)
        with pytest.raises(gsv.GsvError, match="gsv status 1: .*holds"):
            ev.evaluate_from_source(src, **_verified_kwargs(res, mode, outboards=with_1(res.outboards[1][:-32])))
        with pytest.raises(gsv.GsvError, match="gsv status 1: .*1664 records, the stream here holds 1665"):
            ev.evaluate_from_source(src, **_verified_kwargs(res, mode, outboards=with_1(flipped(res.outboards[1], 16, 1))))
        monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "3")  # the pass's k against the outboards': both values are named
        with pytest.raises(gsv.GsvError, match=r"gsv status 1: .*2\^2 chunks.*2\^3"):
            ev.evaluate_from_source(src, **_verified_kwargs(res, mode))
        monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
        assert src.calls == 0
    assert ev.evaluate_from_source(Source(streams), **_verified_kwargs(res, "up_front")) == res.blake3
    ev.close()


# ---- 6. other ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_dry_source_leaves_the_digest_arrays_untouched(engine, monkeypatch, mode):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    p, streams, res, _ = _program_garbled(gsv, engine)
    ev = _program_evaluator(gsv, engine, p)
    with pytest.raises(gsv.GsvError, match="gsv status 4: .*exhausted"):
        ev.evaluate_from_source(Source(streams, dry=(2, N_PROGRAM - 1)), **_verified_kwargs(res, mode))
    # the C entry point itself, with arrays of the caller's
    src = Source(streams, dry=(2, N_PROGRAM - 1))

    def cb(_user, inst, first, ptr, n):
        a = src(int(inst), int(first), int(n))
        if a is None:
            return 1
        C.memmove(ptr, a.ctypes.data, a.size)
        return 0

    obs = [np.frombuffer(o, np.uint8) for o in res.outboards]
    ob_p = (C.POINTER(C.c_uint8) * 3)(*[gsv._p(o) for o in obs])
    ob_n = (C.c_uint64 * 3)(*[o.size for o in obs])
    last = np.zeros((3, 1024), np.uint8)
    last[:, :16] = np.stack([np.frombuffer(x, np.uint8) for x in res.last_chunks])
    exp = np.frombuffer(b"".join(res.blake3), np.uint8)
    macs, dig = np.full((3, 16), 0xAA, np.uint8), np.full((3, 32), 0xBB, np.uint8)
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    rc = gsv.lib().gsv_session_evaluate_streaming_source_verified(ev.h, 0, gsv.CT_SOURCE_FN(cb), None, ob_p, ob_n, gsv._p(last) if mode == "up_front" else None, gsv._p(exp), 32,
                                                                  gsv._p(macs), gsv._p(dig))
    assert rc == 4 and (macs == 0xAA).all() and (dig == 0xBB).all()
    # ... and a mismatch leaves them alone too
    src = Source(streams, flip=(1, 5))
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    rc = gsv.lib().gsv_session_evaluate_streaming_source_verified(ev.h, 0, gsv.CT_SOURCE_FN(cb), None, ob_p, ob_n, gsv._p(last) if mode == "up_front" else None, gsv._p(exp), 32,
                                                                  gsv._p(macs), gsv._p(dig))
    assert rc == 5 and (macs == 0xAA).all() and (dig == 0xBB).all() and ev.mismatch_info() == (1, 0, 0)
    ev.close()


def test_ring_plan_session_is_refused(engine, monkeypatch):
    import garbled_snark_verifier_amd as gsv
    P, T, sp = _plan_setup(gsv, monkeypatch, 1)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(3)]
    refs = [P.reference(gsv, sp, s)[0].ciphertexts for s in seeds]
    want = [E.ref_digest(r.tobytes()) for r in refs]
    _, _, _, bits, active, consts_active = E._plan_case(gsv, sp, P, seeds)
    # (a well-formed header is all these outboards need: the ring is refused before anything is parsed)
    obs = [b"GSVB3OB\n" + (1).to_bytes(4, "little") + K.to_bytes(4, "little") + n_ct.to_bytes(8, "little") + bytes(gsv.blake3_outboard_size(n_ct, K)[0] - 24)] * 3
    ring = gsv.Session(engine, sp.plan, 3, **E._plan_opts("ring", n_ct))
    ring.set_evaluate_inputs(consts_active, active, bits)
    src = Source(refs)
    for last in (None, [r.tobytes()[-gsv.blake3_outboard_size(n_ct, K)[1]:] for r in refs]):
        with pytest.raises(gsv.GsvError, match="gsv status 1: verified streaming is not available for plan sessions over a ciphertext ring"):
            ring.evaluate_from_source(src, commitment="blake3", outboards=obs, expected=want, last_chunks=last)
    assert src.calls == 0
    assert ring.evaluate_from_source(src, commitment="blake3") == want  # unverified, the ring serves as ever
    ring.close()
