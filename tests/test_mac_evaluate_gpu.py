"""CBC-MAC checkpoints while evaluating (include/gsv_engine.h "CBC-MAC checkpoints while evaluating"): the streaming evaluators verified
against checkpoint files or in-memory checkpoints (gsv_session_evaluate_streaming_mac_calls / _source_mac_calls), in one pass and in
slices with restart points, and the resident stream checked where it lies (gsv_session_ciphertext_cbcmac_check).

References: the unverified evaluation of the same inputs, plan_small_lib.reference / the oracle for streams, MACs and outputs, and the
host checker gsv.cbcmac_file_check for the place of a mismatch.  A tampered file, stream or checkpoint is data: nothing here provokes
a device fault."""
import os

import numpy as np
import pytest

import test_blake3_evaluate as E
import test_evaluate_slices as S

pytestmark = pytest.mark.gpu


def _mismatch(gsv, call):
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        call()
    return ei.value


def _place(e):
    return e.instance, e.group, e.first_record


def _flip_state(path, g):
    E._flip(path, 24 + 16 * g + 3, 0x40)


# ---- program session -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 11])
def test_program_session(engine, monkeypatch, tmp_path, k):
    """The layered program, 3 instances, 45 replays through a ring of 7: segments of 259 records, 1 665 in all.  At k = 3 groups of 8
    straddle every ring, at k = 11 the stream is one group."""
    import garbled_snark_verifier_amd as gsv
    p = E._layered()
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", str(k))
    d = str(tmp_path)
    sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    macs = sess.garble_streaming(directory=d, first_index=10, threads=2, checkpoint_dir=d)
    sess.close()
    monkeypatch.delenv("GSV_MAC_GROUP_LOG2")  # a reader takes k from the files
    gc = [os.path.join(d, gsv.gc_file_name(10 + i)) for i in range(3)]
    ck = [os.path.join(d, gsv.checkpoint_file_name(10 + i)) for i in range(3)]
    n_states = -(-1665 >> k)

    def inputs(ev):
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])

    ev = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    inputs(ev)
    assert ev.evaluate_streaming(d, first_index=10) == macs  # unverified: the MAC workers
    act0, ob0 = ev.read_outputs(with_bits=True)
    inputs(ev)
    assert ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d, expected=macs) == macs
    act, ob = ev.read_outputs(with_bits=True)
    assert (act == act0).all() and (ob == ob0).all()
    inputs(ev)
    assert ev.evaluate_streaming_indexed(d, [10, 11, 12], checkpoint_dir=d) == macs
    # what the arguments may not be
    with pytest.raises(ValueError):
        ev.evaluate_streaming(d, first_index=10, commitment="blake3", checkpoint_dir=d)
    with pytest.raises(ValueError):
        ev.evaluate_streaming(d, first_index=10, expected=macs)  # expected without checkpoint_dir: as ever
    L = gsv.lib()
    out = np.full((3, 16), 0xAB, np.uint8)
    assert L.gsv_session_evaluate_streaming_mac_calls(ev.h, 0, 0, 0, 1, d.encode(), None, 10, d.encode(), None, gsv._p(out)) == 1  # restartable: plan sessions only
    assert L.gsv_session_evaluate_streaming_mac_calls(ev.h, 0, 0, 1, 0, d.encode(), None, 10, d.encode(), None, gsv._p(out)) == 1
    assert (out == 0xAB).all()
    # one byte of instance 1's file flipped in the second ring
    r = 259 + 100
    E._flip(gc[1], 16 * r + 5)
    inputs(ev)
    e = _mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d, expected=macs))
    assert _place(e) == (1, r >> k, (r >> k) << k) == ev.mismatch_info() and "gsv status 5:" in str(e)
    assert gsv.cbcmac_file_check(gc[1], ck[1]) == (None, r >> k)
    with pytest.raises(gsv.GsvError, match="nothing ran"):
        ev.read_outputs()
    E._flip(gc[1], 16 * r + 5)
    inputs(ev)
    assert ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d, expected=macs) == macs  # the session is as good as new
    act, ob = ev.read_outputs(with_bits=True)
    assert (act == act0).all() and (ob == ob0).all()
    # an inner state of a checkpoint file
    if n_states > 2:
        g = n_states // 2
        _flip_state(ck[2], g)
        inputs(ev)
        assert _place(_mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d, expected=macs))) == (2, g, g << k)
        _flip_state(ck[2], g)
    # the last state: against `expected` it has no place, without `expected` it is the last group
    _flip_state(ck[0], n_states - 1)
    inputs(ev)
    assert _place(_mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d, expected=macs))) == (0, None, None)
    inputs(ev)
    assert _place(_mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d))) == (0, n_states - 1, (n_states - 1) << k)
    _flip_state(ck[0], n_states - 1)
    inputs(ev)
    assert _place(_mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, checkpoint_dir=d, expected=[macs[0], macs[2], macs[2]]))) == (1, None, None)
    inputs(ev)
    assert ev.evaluate_streaming(d, first_index=10) == macs  # a plain pass afterwards: the CBC-MACs on the host, as ever
    ev.close()


# ---- plan sessions -------------------------------------------------------------------------------------------------------------------------
class _Plan:
    """test_mac_check_gpu.test_plan_session's geometry on the evaluator's side: 2 ni + 1 instances, windows of n_ct // 2 and segments of
    n_ct // 8 records, k = (n_ct // 8).bit_length(): groups are larger than a segment and straddle windows."""

    def __init__(self, gsv, engine, monkeypatch, tmp_path, ni):
        import plan_small_lib as P
        import test_plan_small as T
        self.gsv, self.P, self.T = gsv, P, T
        _, self.sp = T.small_plan()
        sp = self.sp
        monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
        monkeypatch.delenv("GSV_AND_TERMS", raising=False)
        monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")
        self.n_ct = n_ct = sp.plan.info["n_ciphertexts"]
        self.k = (n_ct // 8).bit_length()
        self.d = str(tmp_path)
        self.B = B = 2 * ni + 1
        self.seeds = [T.SEED0 + j for j in range(B)]
        self.streams = [P.reference(gsv, sp, s)[0].ciphertexts for s in self.seeds]
        self.macs = [P.reference(gsv, sp, s)[0].ct_hash for s in self.seeds]
        for j in range(B):
            gsv.write_gc_file(self.gc(j), self.streams[j])
            assert gsv.cbcmac_file_checkpoints(self.gc(j), self.k, self.ck(j)) == self.macs[j]
        _, _, _, self.bits, self.active, self.consts_active = E._plan_case(gsv, sp, P, self.seeds)
        self.ev = gsv.Session(engine, sp.plan, B, **E._plan_opts("windows", n_ct))
        assert self.ev.instances_per_workgroup == ni

    def gc(self, j):
        return os.path.join(self.d, self.gsv.gc_file_name(j))

    def ck(self, j):
        return os.path.join(self.d, self.gsv.checkpoint_file_name(j))

    def set_inputs(self):
        self.ev.set_evaluate_inputs(self.consts_active, self.active, self.bits)

    def outputs_ok(self):
        act, ob = self.ev.read_outputs(with_bits=True)
        for i, s in enumerate(self.seeds):
            e = self.P.reference(self.gsv, self.sp, s)[1]
            assert (ob[i] == e.output_bits).all() and (act[i] == e.output_active).all(), "instance %d" % i
        return act, ob


@pytest.mark.parametrize("ni", [1, 4])
def test_plan_session(engine, monkeypatch, tmp_path, ni):
    import garbled_snark_verifier_amd as gsv
    c = _Plan(gsv, engine, monkeypatch, tmp_path, ni)
    idx = list(range(c.B))
    info = c.ev.schedule_info()
    assert info["n_windows"] >= 2 and info["n_segments"] > info["n_windows"] and info["segment_ct_records"] < (1 << c.k)
    c.set_inputs()
    assert c.ev.evaluate_streaming_indexed(c.d, idx) == c.macs
    act0, ob0 = c.outputs_ok()
    c.set_inputs()
    assert c.ev.evaluate_streaming_indexed(c.d, idx, checkpoint_dir=c.d, expected=c.macs) == c.macs
    act, ob = c.outputs_ok()
    assert (act == act0).all() and (ob == ob0).all()
    assert c.ev.schedule_info()["windows_launched"] == info["n_windows"]
    # a group that straddles the first window boundary, corrupted in front of the boundary: found before the second window is launched
    counts = [int(r[3]) for r in c.sp.plan.call_info()]
    bound = sum(counts[:c.ev.windows()[1][0]])
    g = bound >> c.k
    assert (g << c.k) < bound - 1 and bound < min((g + 1) << c.k, c.n_ct)
    last, r = c.B - 1, bound - 1
    E._flip(c.gc(last), 16 * r + 9)
    c.set_inputs()
    e = _mismatch(gsv, lambda: c.ev.evaluate_streaming_indexed(c.d, idx, checkpoint_dir=c.d, expected=c.macs))
    assert _place(e) == (last, g, g << c.k) and gsv.cbcmac_file_check(c.gc(last), c.ck(last)) == (None, g)
    assert c.ev.schedule_info()["windows_launched"] < info["n_windows"]
    with pytest.raises(gsv.GsvError, match="nothing ran"):
        c.ev.read_outputs()
    E._flip(c.gc(last), 16 * r + 9)
    c.set_inputs()
    assert c.ev.evaluate_streaming(c.d, checkpoint_dir=c.d) == c.macs
    c.outputs_ok()
    assert c.ev.fallback_count() == 0
    c.ev.close()
    ring = gsv.Session(engine, c.sp.plan, c.B, **E._plan_opts("ring", c.n_ct))
    ring.set_evaluate_inputs(c.consts_active, c.active, c.bits)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*ring"):
        ring.evaluate_streaming(c.d, checkpoint_dir=c.d)
    ring.close()


# ---- slices: test_evaluate_slices' case — four windows at 214 records, segments of 100 — with groups of 64 records (k = 6) -----------------
MAC_K = 6


def _sliced(gsv, engine, monkeypatch, tmp_path, k=MAC_K):
    c = S._Case(gsv, engine, monkeypatch, tmp_path)  # (its group arithmetic is for 64 records per group: BLAKE3 chunks at its k = 0)
    assert c.group == 1 << MAC_K
    c.mck = str(tmp_path / ("mck%d" % k))
    os.mkdir(c.mck)
    for j in range(c.B):
        gsv.cbcmac_file_checkpoints(c.gc(100 + j), k, os.path.join(c.mck, gsv.checkpoint_file_name(100 + j)))
    return c


def test_slices_equal_the_pass(engine, monkeypatch, tmp_path):
    import garbled_snark_verifier_amd as gsv
    c = _sliced(gsv, engine, monkeypatch, tmp_path)
    c.needs_groups()
    v = c.files(checkpoint_dir=c.mck, expected=c.macs_want)
    c.set_inputs()
    assert c.ev.evaluate_streaming_indexed(c.d, c.idx, checkpoint_dir=c.mck, expected=c.macs_want) == c.macs_want
    act0, ob0 = c.outputs_ok()
    c.set_inputs()
    for w in range(c.n_win):
        got = c.slice(w, w + 1, **v)
        assert c.launched() == w + 1
        if w + 1 < c.n_win:
            assert got is None
            c.no_outputs()
    assert got == c.macs_want
    act, ob = c.outputs_ok()
    assert (act == act0).all() and (ob == ob0).all()
    # a slice that asks for another kind of verification than the first — none, BLAKE3 outboards, in-memory checkpoints — is refused
    cks = [open(os.path.join(c.mck, gsv.checkpoint_file_name(j)), "rb").read() for j in c.idx]
    c.set_inputs()
    assert c.slice(0, 1, **v) is None
    S._invalid(gsv, lambda: c.slice(1, 2, **c.files()), "same commitments")
    S._invalid(gsv, lambda: c.slice(1, 2, **c.verified()), "same commitments")
    S._invalid(gsv, lambda: c.slice(1, 2, source=lambda i, f, n: c.streams[i][f:f + n], checkpoints=cks), "same commitments")
    # `expected` meets the claimed last states in every slice, not only in the one at call 0: no place, nothing to resume, nothing ran
    e = _mismatch(gsv, lambda: c.slice(1, 2, **dict(v, expected=[c.macs_want[1]] + c.macs_want[1:])))
    assert _place(e) == (0, None, None) and e.resume_call is None and c.launched() == 1
    assert c.slice(1, c.n_win, **v) == c.macs_want  # the pass goes on where it stood
    c.outputs_ok()
    c.set_inputs()
    c.slice(0, 1, **c.files())
    S._invalid(gsv, lambda: c.slice(1, 2, **v), "same commitments")
    with pytest.raises(ValueError):
        c.slice(0, 1, **c.files(checkpoint_dir=c.mck, commitment="both"))
    with pytest.raises(ValueError):
        c.slice(0, 1, **c.files(checkpoints=cks))  # in-memory checkpoints belong to a source
    # a verified restartable slice smaller than a group: at k = 8 the first window holds fewer than 256 records
    c8 = str(tmp_path / "k8")
    os.mkdir(c8)
    for j in range(c.B):
        gsv.cbcmac_file_checkpoints(c.gc(100 + j), 8, os.path.join(c8, gsv.checkpoint_file_name(100 + j)))
    assert c.bounds[1] < 256 <= c.bounds[2]
    k8 = c.files(checkpoint_dir=c8)
    c.set_inputs()
    S._invalid(gsv, lambda: c.slice(0, 1, restartable=True, **k8), "at least one whole group of 2\\^k records")
    assert c.slice(0, 2, restartable=True, **k8) is None
    assert c.slice(2, c.n_win, **k8) == c.macs_want
    c.outputs_ok()
    assert c.ev.fallback_count() == 0
    c.ev.close()


def test_bad_group_inside_the_current_slice(engine, monkeypatch, tmp_path):
    """Restartable, one window per slice; a flipped bit in a group that lies wholly in window 2: rolled back to where slice 2 began."""
    import garbled_snark_verifier_amd as gsv
    c = _sliced(gsv, engine, monkeypatch, tmp_path)
    c.needs_groups()
    c.set_inputs()
    assert c.ev.evaluate_streaming_indexed(c.d, c.idx, checkpoint_dir=c.mck) == c.macs_want
    act0, ob0 = c.outputs_ok()
    g = c.whole[2][0]
    bad, record = 1, g * c.group + 2
    path = c.gc(c.idx[bad])
    clean = open(path, "rb").read()
    E._flip(path, record * 16 + 7)
    v = c.files(checkpoint_dir=c.mck, expected=c.macs_want, restartable=True)
    c.set_inputs()
    assert c.slice(0, 1, **v) is None and c.slice(1, 2, **v) is None
    e = _mismatch(gsv, lambda: c.slice(2, 3, **v))
    assert _place(e) == (bad, g, g * c.group) == c.ev.mismatch_info()
    assert gsv.cbcmac_file_check(path, os.path.join(c.mck, gsv.checkpoint_file_name(c.idx[bad]))) == (None, g)
    assert e.resume_call == c.win[2][0] and c.ev.resume_info() == (c.win[2][0], c.bounds[2])
    assert c.launched() == 2  # as it stood when slice 2 began
    c.no_outputs()
    open(path, "wb").write(clean)
    assert c.slice(2, 3, **v) is None
    assert c.slice(3, c.n_win, **v) == c.macs_want
    act, ob = c.outputs_ok()
    assert (act == act0).all() and (ob == ob0).all()
    assert c.launched() == c.n_win  # windows 0 and 1 were not evaluated again
    with pytest.raises(gsv.GsvError, match="nothing to resume"):
        c.ev.resume_info()
    assert c.ev.fallback_count() == 0
    c.ev.close()


@pytest.mark.parametrize("slice_1_restartable", [True, False])
def test_the_open_group(engine, monkeypatch, tmp_path, slice_1_restartable):
    """A flipped bit in the part of a straddling group that lies in window 1: slice 1 evaluates it unverified, slice 2 finds it — and the
    session goes back to where slice 1 began, or, when slice 1 took no restart point, to call 0."""
    import garbled_snark_verifier_amd as gsv
    c = _sliced(gsv, engine, monkeypatch, tmp_path)
    c.needs_groups()
    assert 2 in c.straddling, c.bounds
    g = c.straddling[2]
    bad, record = 2, c.bounds[2] - 3
    assert c.bounds[1] <= g * c.group < record < c.bounds[2] < (g + 1) * c.group <= c.bounds[3]
    path = c.gc(c.idx[bad])
    clean = open(path, "rb").read()
    E._flip(path, record * 16 + 1)
    v = c.files(checkpoint_dir=c.mck, restartable=True)
    c.set_inputs()
    assert c.slice(0, 1, **v) is None
    assert c.slice(1, 2, **dict(v, restartable=slice_1_restartable)) is None  # the open group's records were evaluated before they were verified
    e = _mismatch(gsv, lambda: c.slice(2, 3, **v))
    assert _place(e) == (bad, g, g * c.group)
    c.no_outputs()
    open(path, "wb").write(clean)
    if slice_1_restartable:
        assert e.resume_call == c.win[1][0] and c.ev.resume_info() == (c.win[1][0], c.bounds[1])
        assert c.launched() == 1
        first = 1
    else:
        assert e.resume_call == 0 and c.ev.resume_info() == (0, 0)
        S._invalid(gsv, lambda: c.slice(1, 2, **v), "previous evaluate slice ended at call 0")  # nothing was rolled back: the pass is over
        c.set_inputs()
        first = 0
    for w in range(first, c.n_win):
        assert c.slice(w, w + 1, **v) == (c.macs_want if w + 1 == c.n_win else None)
    c.outputs_ok()
    assert c.launched() == c.n_win
    c.ev.close()


def _checkpoint_bytes(gsv, c):
    return [open(os.path.join(c.mck, gsv.checkpoint_file_name(j)), "rb").read() for j in c.idx]


def test_a_source_that_runs_dry(engine, monkeypatch, tmp_path):
    """Verified against in-memory checkpoints, restartable: the source returns nothing partway through slice 2, inside an open group."""
    import garbled_snark_verifier_amd as gsv
    c = _sliced(gsv, engine, monkeypatch, tmp_path)
    cks = _checkpoint_bytes(gsv, c)
    calls, state = [], {"dry_from": c.bounds[2] + S.SEGMENT + 20}  # behind the slice's first segment
    assert c.bounds[2] + S.SEGMENT < state["dry_from"] < c.bounds[3]

    def source(inst, first, n):
        calls.append((inst, first, n))
        if inst == 1 and state["dry_from"] is not None and first + n > state["dry_from"]:
            return None
        return c.streams[inst][first:first + n]

    kw = dict(source=source, checkpoints=cks, expected=c.macs_want, restartable=True)
    c.set_inputs()
    assert c.slice(0, 1, **kw) is None and c.slice(1, 2, **kw) is None
    with pytest.raises(gsv.GsvError, match="gsv status 4: Ciphertext source exhausted: instance 1"):
        c.slice(2, 3, **kw)
    assert c.ev.resume_info() == (c.win[2][0], c.bounds[2]) and c.launched() == 2
    c.no_outputs()
    state["dry_from"] = None
    del calls[:]
    assert c.slice(2, 3, **kw) is None
    assert calls[0][1] == c.bounds[2]
    assert c.slice(3, c.n_win, **kw) == c.macs_want
    c.outputs_ok()
    assert c.launched() == c.n_win
    c.ev.close()


def test_source_with_in_memory_checkpoints(engine, monkeypatch, tmp_path):
    """The intact stream verifies; a tampered record is named; each malformed checkpoint is refused before the source is called at all."""
    import garbled_snark_verifier_amd as gsv
    c = _sliced(gsv, engine, monkeypatch, tmp_path)
    cks = _checkpoint_bytes(gsv, c)
    calls = []
    served = [s.copy() for s in c.streams]

    def source(inst, first, n):
        calls.append((inst, first, n))
        return served[inst][first:first + n]

    c.set_inputs()
    assert c.ev.evaluate_from_source(source, checkpoints=cks, expected=c.macs_want) == c.macs_want
    c.outputs_ok()
    assert calls
    r = 300
    served[0][r, 4] ^= 1
    c.set_inputs()
    e = _mismatch(gsv, lambda: c.ev.evaluate_from_source(source, checkpoints=cks))
    assert _place(e) == (0, r >> MAC_K, (r >> MAC_K) << MAC_K)
    assert c.launched() < c.n_win
    c.no_outputs()
    served[0][r, 4] ^= 1
    other_k = os.path.join(c.mck, "other.mck")
    gsv.cbcmac_file_checkpoints(c.gc(c.idx[1]), MAC_K + 1, other_k)
    short = os.path.join(c.d, "short.bin")
    open(short, "wb").write(c.streams[0][:-1].tobytes())
    gsv.cbcmac_file_checkpoints(short, MAC_K, short + ".mck")
    malformed = {
        "wrong magic": [b"x" + cks[0][1:]] + cks[1:],
        "bytes, but k = ": [cks[0] + bytes(16)] + cks[1:],
        "agree on k": [cks[0], open(other_k, "rb").read()] + cks[2:],
        "%d records" % (c.n_ct - 1): [open(short + ".mck", "rb").read()] + cks[1:],
        "format version": [cks[0][:8] + bytes([2, 0, 0, 0]) + cks[0][12:]] + cks[1:],
    }
    for what, bad in malformed.items():
        del calls[:]
        c.set_inputs()
        S._invalid(gsv, lambda: c.ev.evaluate_from_source(source, checkpoints=bad, expected=c.macs_want), what)
        assert not calls, what
    del calls[:]
    c.set_inputs()
    e = _mismatch(gsv, lambda: c.ev.evaluate_from_source(source, checkpoints=cks, expected=[c.macs_want[1]] + c.macs_want[1:]))
    assert _place(e) == (0, None, None) and not calls
    with pytest.raises(ValueError):
        c.ev.evaluate_from_source(source, checkpoints=cks, commitment="blake3")
    c.set_inputs()
    assert c.ev.evaluate_from_source(source, checkpoints=cks) == c.macs_want
    c.outputs_ok()
    c.ev.close()


# ---- the resident stream ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [37, 259, None])
@pytest.mark.parametrize("k", [0, 2, 10])
def test_resident_program_session(engine, monkeypatch, tmp_path, k, resident):
    """Launch ranges of 37 records (one replay), of 259 and the default (one range), after garble() and after upload_ciphertexts."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    if resident is None:
        monkeypatch.delenv("GSV_MAC_RESIDENT_RECORDS", raising=False)
    else:
        monkeypatch.setenv("GSV_MAC_RESIDENT_RECORDS", str(resident))
    p = E._layered()
    d = str(tmp_path)
    macs = [bytes(o.cbcmac(r)) for r in p["refs"]]
    for i in range(3):
        gsv.write_gc_file(os.path.join(d, gsv.gc_file_name(i)), p["refs"][i])
        assert gsv.cbcmac_file_checkpoints(os.path.join(d, gsv.gc_file_name(i)), k, os.path.join(d, gsv.checkpoint_file_name(i))) == macs[i]
    sess = gsv.Session(engine, p["prog"], 3, p["K"])
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    sess.garble()  # asynchronous: the check kernels queue behind it
    assert sess.ciphertext_cbcmac_check(d, expected=macs) == macs == [sess.ciphertext_hash(i) for i in range(3)]
    assert (sess.read_ciphertexts(1) == p["refs"][1]).all()  # the block is only read
    sess.close()
    ev = gsv.Session(engine, p["prog"], 3, p["K"])
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    for i in range(2):
        ev.upload_ciphertexts(i, p["refs"][i])
    with pytest.raises(gsv.GsvError, match="exhausted"):
        ev.ciphertext_cbcmac_check(d)  # instance 2 has not been uploaded
    r = 700
    changed = p["refs"][2].copy()
    changed[r, 9] ^= 0x08
    ev.upload_ciphertexts(2, changed)
    e = _mismatch(gsv, lambda: ev.ciphertext_cbcmac_check(d, indexes=[0, 1, 2]))
    assert _place(e) == (2, r >> k, (r >> k) << k) == ev.mismatch_info()
    open(os.path.join(d, "changed.bin"), "wb").write(changed.tobytes())
    assert gsv.cbcmac_file_check(os.path.join(d, "changed.bin"), os.path.join(d, gsv.checkpoint_file_name(2))) == (None, r >> k)
    assert _place(_mismatch(gsv, lambda: ev.ciphertext_cbcmac_check(d, expected=[macs[1], macs[1], macs[2]]))) == (0, None, None)
    fresh = gsv.Session(engine, p["prog"], 3, p["K"])
    fresh.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    for i in range(3):
        fresh.upload_ciphertexts(i, p["refs"][i])
    assert fresh.ciphertext_cbcmac_check(d) == macs
    fresh.evaluate()
    fresh.sync()
    fresh.read_outputs()
    fresh.close()
    ev.close()


@pytest.mark.parametrize("ni", [1, 4])
def test_resident_plan_session(engine, monkeypatch, tmp_path, ni):
    """One launch range per call block, or several (ranges of 100 records); groups of 64 records straddle the blocks through the carry."""
    import garbled_snark_verifier_amd as gsv
    c = _Plan(gsv, engine, monkeypatch, tmp_path, ni)
    c.ev.close()
    k6 = str(tmp_path / "k6")
    os.mkdir(k6)
    for j in range(c.B):
        gsv.cbcmac_file_checkpoints(c.gc(j), 6, os.path.join(k6, gsv.checkpoint_file_name(j)))
    counts = [int(r[3]) for r in c.sp.plan.call_info()]
    assert any(n % 64 for n in counts)
    delta, consts, inputs, _, _, _ = E._plan_case(gsv, c.sp, c.P, c.seeds)
    monkeypatch.delenv("GSV_MAC_RESIDENT_RECORDS", raising=False)
    sess = gsv.Session(engine, c.sp.plan, c.B, retain_stream=True, concurrent_calls=8)
    assert sess.instances_per_workgroup == ni
    sess.set_garble_inputs(delta, consts, inputs)
    sess.garble()
    assert sess.ciphertext_cbcmac_check(c.d, expected=c.macs) == c.macs  # groups larger than most call blocks
    assert sess.ciphertext_cbcmac_check(k6) == c.macs
    monkeypatch.setenv("GSV_MAC_RESIDENT_RECORDS", "100")
    assert sess.ciphertext_cbcmac_check(k6, indexes=list(range(c.B))) == c.macs
    g = (c.n_ct // 2) >> 6
    _flip_state(os.path.join(k6, gsv.checkpoint_file_name(c.B - 1)), g)
    assert _place(_mismatch(gsv, lambda: sess.ciphertext_cbcmac_check(k6))) == (c.B - 1, g, g << 6)
    assert sess.fallback_count() == 0
    sess.close()
    window = gsv.Session(engine, c.sp.plan, c.B, retain_stream=False)
    with pytest.raises(gsv.GsvError, match="retains only part"):
        window.ciphertext_cbcmac_check(c.d)
    window.close()


def test_resident_refusals_and_the_empty_stream(engine, tmp_path):
    import garbled_snark_verifier_amd as gsv
    p = E._layered()
    d = str(tmp_path)
    for i in range(3):
        gsv.write_gc_file(os.path.join(d, gsv.gc_file_name(i)), p["refs"][i])
        gsv.cbcmac_file_checkpoints(os.path.join(d, gsv.gc_file_name(i)), 4, os.path.join(d, gsv.checkpoint_file_name(i)))
    part = gsv.Session(engine, p["prog"], 3, p["K"], 7)  # ct_capacity_replays < replays: only a ring of the stream is there
    with pytest.raises(gsv.GsvError, match="retains only part"):
        part.ciphertext_cbcmac_check(d)
    part.close()
    full = gsv.Session(engine, p["prog"], 3, p["K"])
    full.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    full.garble()
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*cannot open"):
        full.ciphertext_cbcmac_check(d, first_index=1)  # gc_3.mck is not there
    gsv.cbcmac_file_checkpoints(os.path.join(d, gsv.gc_file_name(2)), 5, os.path.join(d, gsv.checkpoint_file_name(2)))
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*must agree"):
        full.ciphertext_cbcmac_check(d)
    full.close()
    prog = gsv.Program.from_gates(2, [(8, 2, 3, 4), (10, 4, 4, 5)], [4, 5])  # free gates only
    assert prog.info["n_ciphertexts"] == 0
    labs = [gsv.labels_from_seed(s, 2) for s in (1, 2)]
    e = str(tmp_path / "empty")
    os.mkdir(e)
    for i in range(2):
        open(os.path.join(e, gsv.gc_file_name(i)), "wb").close()
        gsv.cbcmac_file_checkpoints(os.path.join(e, gsv.gc_file_name(i)), 3, os.path.join(e, gsv.checkpoint_file_name(i)))
    sess = gsv.Session(engine, prog, 2)
    sess.set_garble_inputs(np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
    sess.garble()
    assert sess.ciphertext_cbcmac_check(e) == [bytes(16), bytes(16)]
    sess.close()


# ---- sharding.evaluate_from(checkpoint_dir=) -------------------------------------------------------------------------------------------------
def test_evaluate_from_with_checkpoints_end_to_end(engine, monkeypatch, tmp_path):
    """fq_mul, 5 instances, as test_mac_check_gpu.test_regarbling_with_checkpoints sets them up: garble_and_commit(checkpoint_dir=) ->
    evaluate_from(checkpoint_dir=) with the default GPU evaluator."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    k = 8
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", str(k))
    circuit, total = "fq_mul", 5
    prog = gsv.Program.from_circuit(circuit)
    gc = str(tmp_path)
    seeds = [int(x) for x in sharding.instance_seeds(78, total)]
    commits = sharding.garble_and_commit(circuit, seeds, list(range(total)), engine=engine, program=prog, gc_dir=gc, checkpoint_dir=gc)
    monkeypatch.delenv("GSV_MAC_GROUP_LOG2")
    keep = [0, 2, 3]
    n_in, n_out = prog.info["n_inputs"], prog.info["n_outputs"]
    bits = np.random.default_rng(5).integers(0, 2, (len(keep), n_in)).astype(np.uint8)
    cases = []
    for j, i in enumerate(keep):
        dl, f, t, inp = gsv.labels_from_seed(seeds[i], n_in)
        cases.append({"index": i, "true_constant_wire": t ^ dl, "false_constant_wire": f, "input_active": np.where(bits[j][:, None] == 1, inp ^ dl[None, :], inp), "input_bits": bits[j]})
    res = sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog, checkpoint_dir=gc)
    plain = sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog)  # the parent's path: MAC workers
    assert [r[0] for r in res] == keep == [r[0] for r in plain]
    for j, (a, b) in enumerate(zip(res, plain)):
        assert (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[2] == o.execute(circuit, bits[j])[0]).all()
    n = os.path.getsize(os.path.join(gc, gsv.gc_file_name(3))) // 16
    r = n // 2
    assert (r >> k) > 0
    E._flip(os.path.join(gc, gsv.gc_file_name(3)), 16 * r + 9)
    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog, checkpoint_dir=gc)
    assert (ei.value.kind, ei.value.index) == ("CiphertextMismatch", 3)
    assert ei.value.details["group"] == r >> k and ei.value.details["first_record"] == (r >> k) << k
    assert gsv.cbcmac_file_check(os.path.join(gc, gsv.gc_file_name(3)), os.path.join(gc, gsv.checkpoint_file_name(3))) == (None, r >> k)
    prog.close()
