"""A plan session's streaming evaluation in slices of whole windows (Session.evaluate_calls: gsv_session_evaluate_streaming_calls /
_source_calls), and the restart points a failed slice rolls the session back to (Session.resume_info, CiphertextMismatch.resume_call).

The plan is the small plan of tests/plan_small_lib.py: 12 calls, 775 ciphertext records per instance, which at 214 records per window
fall into four windows, [0, 214) [214, 422) [422, 609) [609, 775), and at 100 records per drain segment into more segments than
windows.  GSV_B3_SUBTREE_LOG2 = 0: a group is one chunk of 64 records, so every window holds at least two whole groups and the groups
at records 192 and 384 straddle a window boundary.  Every test asserts these facts from the session's own schedule (_layout).
References: plan_small_lib.reference (streams, outputs; tests/gate_list_ref.py, the CPU oracle), the oracle's CBC-MAC over a prefix of
a reference stream, and b3_ref's digests (test_blake3_evaluate.ref_digest).  Tampering is one flipped bit in a file or in a source's
copy of a stream; a source fails by returning nothing.  Nothing here provokes a device fault: the one forced switch is the existing
GSV_FAULT_WITHHOLD_DEP of test_forced_dependency_fault_falls_back_to_the_safe_schedule."""
import os

import numpy as np
import pytest

import oracle_lib as o
import test_blake3_evaluate as E

pytestmark = pytest.mark.gpu
K = 0
WINDOW, SEGMENT = 214, 100


def _setup(gsv, monkeypatch, ni, k=K):
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(k))
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")
    return P, T, sp


class _Case:
    """B = 2 ni + 1 instances reading the reference streams' files gc_<100 + j>.bin (outboards beside them) through a permuted index list."""

    def __init__(self, gsv, engine, monkeypatch, tmp_path, ni=1, k=K, window=WINDOW):
        self.gsv, self.k, self.group = gsv, k, 64 << k
        self.P, self.T, self.sp = _setup(gsv, monkeypatch, ni, k)
        P, T, sp = self.P, self.T, self.sp
        self.d = str(tmp_path)
        self.n_ct = sp.plan.info["n_ciphertexts"]
        self.B = B = 2 * ni + 1
        perm = [int(x) for x in np.random.default_rng(ni).permutation(B)]
        if perm == sorted(perm):
            perm = perm[1:] + perm[:1]
        self.seeds = [T.SEED0 + j for j in perm]
        self.idx = [100 + j for j in perm]
        for j in range(B):
            gsv.write_gc_file(self.gc(100 + j), P.reference(gsv, sp, T.SEED0 + j)[0].ciphertexts)
            gsv.blake3_file_outboard(self.gc(100 + j), k, os.path.join(self.d, gsv.outboard_file_name(100 + j)))
        self.streams = [P.reference(gsv, sp, s)[0].ciphertexts for s in self.seeds]
        self.want = [E.ref_digest(c.tobytes()) for c in self.streams]
        self.macs_want = [P.reference(gsv, sp, s)[0].ct_hash for s in self.seeds]
        _, _, _, self.bits, self.active, self.consts_active = E._plan_case(gsv, sp, P, self.seeds)
        self.ev = gsv.Session(engine, sp.plan, B, retain_stream=False, window_ct_records=window, drain_segment_records=SEGMENT)
        assert self.ev.instances_per_workgroup == ni
        self._layout()

    def gc(self, index):
        return os.path.join(self.d, self.gsv.gc_file_name(index))

    def _layout(self):
        """The facts the tests rest on, from the session's schedule: windows, their first records, groups inside and across them."""
        info = self.ev.schedule_info()
        self.win = [(int(a), int(b)) for a, b, _ in self.ev.windows()]  # gsv_session_plan_window
        self.n_win, self.n_calls = info["n_windows"], info["n_calls"]
        assert self.n_win >= 4 and info["n_segments"] > self.n_win and len(self.win) == self.n_win
        counts = [int(r[3]) for r in self.sp.plan.call_info()]
        self.bounds = [sum(counts[:c0]) for c0, _ in self.win] + [sum(counts)]
        assert self.bounds[-1] == self.n_ct and self.win[0][0] == 0 and sum(n for _, n in self.win) == self.n_calls
        G = self.group
        self.n_groups = (max(1, -(-self.n_ct // 64)) - 1) >> self.k
        self.whole = [[g for g in range(self.n_groups) if a <= g * G and (g + 1) * G <= b] for a, b in zip(self.bounds, self.bounds[1:])]
        self.straddling = {w: b // G for w, b in enumerate(self.bounds[1:-1], 1) if b % G and b // G < self.n_groups}  # window w begins inside this group

    def needs_groups(self):
        assert all(len(g) >= 2 for g in self.whole), self.whole       # every window holds at least two whole groups per instance
        assert self.straddling, self.bounds                            # at least one group straddles a window boundary

    def set_inputs(self):
        self.ev.set_evaluate_inputs(self.consts_active, self.active, self.bits)

    def prefix_macs(self, w):
        """the oracle's CBC-MAC over every stream's records in front of window w"""
        return [bytes(o.cbcmac(c[:self.bounds[w]])) for c in self.streams]

    def files(self, **kw):
        return dict(directory=self.d, indexes=self.idx, **kw)

    def verified(self, **kw):
        return self.files(commitment="blake3", outboard_dir=self.d, expected=self.want, **kw)

    def slice(self, w0, w1, **kw):
        """windows [w0, w1) as one slice"""
        return self.ev.evaluate_calls(self.win[w0][0], sum(n for _, n in self.win[w0:w1]), **kw)

    def outputs_ok(self):
        act, ob = self.ev.read_outputs(with_bits=True)
        for i, s in enumerate(self.seeds):
            e = self.P.reference(self.gsv, self.sp, s)[1]
            assert (ob[i] == e.output_bits).all() and (act[i] == e.output_active).all(), "instance %d" % i
        return act, ob

    def no_outputs(self):
        with pytest.raises(self.gsv.GsvError, match="nothing ran"):
            self.ev.read_outputs()

    def launched(self):
        return self.ev.schedule_info()["windows_launched"]


def _invalid(gsv, call, match):
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*" + match):
        call()


@pytest.mark.parametrize("ni", [1, 4])
def test_slices_equal_the_pass(engine, monkeypatch, tmp_path, ni):
    """One window per slice, then two uneven slices: outputs, bits, MACs and digests are the unsliced call's and the reference's, the MAC
    states after each slice the reference's prefix MACs."""
    import garbled_snark_verifier_amd as gsv
    c = _Case(gsv, engine, monkeypatch, tmp_path, ni)
    c.needs_groups()
    c.set_inputs()
    macs, digests = c.ev.evaluate_streaming_indexed(c.d, c.idx, commitment="both")
    assert digests == c.want and macs == c.macs_want
    act0, ob0 = c.outputs_ok()
    c.set_inputs()
    for w in range(c.n_win):
        macs, digests = c.slice(w, w + 1, **c.files(commitment="both"))
        assert macs == c.prefix_macs(w + 1), w
        assert c.launched() == w + 1
        if w + 1 < c.n_win:
            assert digests is None
            c.no_outputs()
    assert digests == c.want and macs == c.macs_want
    act, ob = c.outputs_ok()
    assert (act == act0).all() and (ob == ob0).all()
    c.set_inputs()
    macs, digests = c.slice(0, 1, **c.files(commitment="both"))
    assert digests is None and macs == c.prefix_macs(1)
    c.no_outputs()
    assert c.slice(1, c.n_win, **c.files(commitment="both")) == (c.macs_want, c.want)
    act, ob = c.outputs_ok()
    assert (act == act0).all() and (ob == ob0).all()
    with pytest.raises(gsv.GsvError, match="nothing to resume"):
        c.ev.resume_info()
    assert c.ev.fallback_count() == 0
    c.ev.close()


def test_chaining_rules(engine, monkeypatch, tmp_path):
    """What a slice may not be — each refusal is GSV_ERR_INVALID and leaves the session usable."""
    import garbled_snark_verifier_amd as gsv
    c = _Case(gsv, engine, monkeypatch, tmp_path)
    both = c.files(commitment="both")
    c.set_inputs()
    c.slice(0, 1, **both)
    _invalid(gsv, lambda: c.slice(2, 3, **both), "previous evaluate slice ended at call %d" % c.win[1][0])  # does not start where the last one ended
    cut = [w for w, (_, n) in enumerate(c.win) if n > 1 and w >= 1][0]
    assert cut == 1
    _invalid(gsv, lambda: c.ev.evaluate_calls(c.win[1][0], 1, **both), "window boundaries")                   # a call range that cuts a window
    _invalid(gsv, lambda: c.slice(1, 2, **c.files(commitment="cbcmac")), "same commitments")                    # a changed commitment
    _invalid(gsv, lambda: c.slice(1, 2, **c.verified()), "same commitments")                                    # ... or kind of verification
    _invalid(gsv, lambda: c.ev.evaluate_calls(c.win[1][0], 0, **both), "an empty slice")                        # n_calls == 0 anywhere but at call 0
    with pytest.raises(ValueError):
        c.ev.evaluate_calls(0, 0, **both)
    with pytest.raises(ValueError):
        c.ev.evaluate_calls(0, 1, commitment="both")
    macs, digests = c.slice(1, 2, **both)  # the pass goes on where it stood
    assert digests is None and macs == c.prefix_macs(2)
    assert c.slice(2, c.n_win, **both) == (c.macs_want, c.want)
    c.outputs_ok()
    # a verified restartable slice smaller than a group: groups of 4 chunks = 256 records, the first window holds fewer
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")
    d2 = str(tmp_path / "k2")
    os.mkdir(d2)
    for j in c.idx:
        gsv.blake3_file_outboard(c.gc(j), 2, os.path.join(d2, gsv.outboard_file_name(j)))
    k2 = c.files(commitment="blake3", outboard_dir=d2, expected=c.want)
    assert c.bounds[1] < 256 <= c.bounds[2]
    c.set_inputs()
    _invalid(gsv, lambda: c.slice(0, 1, restartable=True, **k2), "at least one whole group of 2\\^k chunks")
    assert c.slice(0, 2, restartable=True, **k2) is None
    assert c.slice(2, c.n_win, **k2) == c.want
    c.outputs_ok()
    c.ev.close()
    # a program session
    p = E._layered()
    for i in range(3):
        gsv.write_gc_file(c.gc(10 + i), p["refs"][i])
    sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    sess.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    _invalid(gsv, lambda: sess.evaluate_calls(0, 1, directory=c.d, first_index=10, commitment="blake3"), "not a plan session")
    assert sess.evaluate_streaming(c.d, first_index=10, commitment="blake3") == p["want"]
    sess.close()


def _mismatch(gsv, call):
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        call()
    return ei.value


def test_bad_group_inside_the_current_slice(engine, monkeypatch, tmp_path):
    """Verified and restartable, one window per slice; a flipped bit in a group that lies wholly in window 2."""
    import garbled_snark_verifier_amd as gsv
    c = _Case(gsv, engine, monkeypatch, tmp_path)
    c.needs_groups()
    g = c.whole[2][0]
    bad, record = 1, g * c.group + 2
    path = c.gc(c.idx[bad])
    clean = open(path, "rb").read()
    E._flip(path, record * 16 + 7)
    v = c.verified(restartable=True)
    c.set_inputs()
    assert c.slice(0, 1, **v) is None and c.slice(1, 2, **v) is None
    e = _mismatch(gsv, lambda: c.slice(2, 3, **v))
    assert (e.instance, e.group, e.first_record) == (bad, g, g * c.group) == c.ev.mismatch_info()
    assert e.resume_call == c.win[2][0] and c.ev.resume_info() == (c.win[2][0], c.bounds[2])
    assert c.launched() == 2  # as it stood when slice 2 began
    c.no_outputs()
    open(path, "wb").write(clean)
    assert c.slice(2, 3, **v) is None
    assert c.slice(3, c.n_win, **v) == c.want
    c.outputs_ok()
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
    c = _Case(gsv, engine, monkeypatch, tmp_path)
    c.needs_groups()
    assert 2 in c.straddling, c.bounds  # window 2 begins inside a group
    g = c.straddling[2]
    bad, record = 2, c.bounds[2] - 3
    assert c.bounds[1] <= g * c.group < record < c.bounds[2] < (g + 1) * c.group <= c.bounds[3]
    path = c.gc(c.idx[bad])
    clean = open(path, "rb").read()
    E._flip(path, record * 16 + 1)
    v = c.verified(restartable=True)
    c.set_inputs()
    assert c.slice(0, 1, **v) is None
    assert c.slice(1, 2, **c.verified(restartable=slice_1_restartable)) is None  # the open group's bytes were evaluated before they were verified
    e = _mismatch(gsv, lambda: c.slice(2, 3, **v))
    assert (e.instance, e.group, e.first_record) == (bad, g, g * c.group)
    c.no_outputs()
    open(path, "wb").write(clean)
    if slice_1_restartable:
        assert e.resume_call == c.win[1][0] and c.ev.resume_info() == (c.win[1][0], c.bounds[1])
        assert c.launched() == 1
        first = 1
    else:
        assert e.resume_call == 0 and c.ev.resume_info() == (0, 0)
        _invalid(gsv, lambda: c.slice(1, 2, **v), "previous evaluate slice ended at call 0")  # nothing was rolled back: the pass is over
        c.set_inputs()
        first = 0
    for w in range(first, c.n_win):
        assert c.slice(w, w + 1, **v) == (c.want if w + 1 == c.n_win else None)
    c.outputs_ok()
    assert c.launched() == c.n_win
    c.ev.close()


@pytest.mark.parametrize("where", ["second_slice", "open_group"])
def test_rollback_with_pending_chunk_values(engine, monkeypatch, tmp_path, where):
    """GSV_B3_SUBTREE_LOG2 = 2, two windows per slice: the second slice begins 422 records = 6 chunks into the stream, one group of four
    reduced and two chunk values pending on the device.  Its restart point holds them; after a rollback the group they belong to only
    verifies, and the digests only come out, when they were restored.  A bad bit in a group that begins in the second slice goes back
    to that slice; one in the first slice's part of the group that is open between them goes back to the first."""
    import garbled_snark_verifier_amd as gsv
    c = _Case(gsv, engine, monkeypatch, tmp_path, k=2)
    G = c.group
    assert G == 256 and c.n_win == 4
    cut = c.bounds[2]
    assert (cut // 64) % 4 and all(b - a >= G for a, b in ((0, cut), (cut, c.n_ct)))  # chunk values are pending at the cut; each slice holds a group
    open_g = cut // G
    assert open_g * G < cut < (open_g + 1) * G <= c.n_ct - 64 and (open_g + 2) * G <= (c.n_ct - 1) // 64 * 64  # the open group ends, and a whole one follows, in the second slice
    g, record = (open_g + 1, (open_g + 1) * G + 9) if where == "second_slice" else (open_g, cut - 5)
    bad = 1
    path = c.gc(c.idx[bad])
    clean = open(path, "rb").read()
    E._flip(path, record * 16 + 2)
    v = c.verified(restartable=True)
    c.set_inputs()
    assert c.slice(0, 2, **v) is None
    e = _mismatch(gsv, lambda: c.slice(2, 4, **v))
    assert (e.instance, e.group, e.first_record) == (bad, g, g * G)
    open(path, "wb").write(clean)
    if where == "second_slice":
        assert e.resume_call == c.win[2][0] and c.ev.resume_info() == (c.win[2][0], cut) and c.launched() == 2
    else:
        assert e.resume_call == 0 and c.ev.resume_info() == (0, 0) and c.launched() == 0  # rolled back to the first slice's restart point: no inputs are set again
        assert c.slice(0, 2, **v) is None
    assert c.slice(2, 4, **v) == c.want
    c.outputs_ok()
    assert c.launched() == c.n_win
    c.ev.close()


def test_a_source_that_runs_dry(engine, monkeypatch, tmp_path):
    """Unverified, restartable: the source returns non-zero partway through slice 2."""
    import garbled_snark_verifier_amd as gsv
    c = _Case(gsv, engine, monkeypatch, tmp_path)
    calls, state = [], {"dry_from": c.bounds[2] + SEGMENT + 20}  # behind the slice's first segment
    assert c.bounds[2] + SEGMENT < state["dry_from"] < c.bounds[3]

    def source(inst, first, n):
        calls.append((inst, first, n))
        if inst == 1 and state["dry_from"] is not None and first + n > state["dry_from"]:
            return None
        return c.streams[inst][first:first + n]

    kw = dict(source=source, commitment="both", restartable=True)
    c.set_inputs()
    c.slice(0, 1, **kw)
    macs, _ = c.slice(1, 2, **kw)
    assert macs == c.prefix_macs(2)
    assert min(f for _, f, _ in calls[-c.B:]) >= c.bounds[1]
    with pytest.raises(gsv.GsvError, match="gsv status 4: Ciphertext source exhausted: instance 1"):
        c.slice(2, 3, **kw)
    assert c.ev.resume_info() == (c.win[2][0], c.bounds[2]) and c.launched() == 2
    c.no_outputs()
    state["dry_from"] = None
    del calls[:]
    macs, digests = c.slice(2, 3, **kw)
    assert calls[0][1] == c.bounds[2] and digests is None and macs == c.prefix_macs(3)
    assert c.slice(3, c.n_win, **kw) == (c.macs_want, c.want)
    c.outputs_ok()
    assert c.launched() == c.n_win
    c.ev.close()


@pytest.mark.parametrize("mode", ["up_front", "deferred"])
def test_verified_source_slices(engine, monkeypatch, tmp_path, mode):
    """test_bad_group_inside_the_current_slice through source= with the outboards in memory; deferred mode's wrong commitment has no place."""
    import garbled_snark_verifier_amd as gsv
    c = _Case(gsv, engine, monkeypatch, tmp_path)
    c.needs_groups()
    obs = [open(os.path.join(c.d, gsv.outboard_file_name(j)), "rb").read() for j in c.idx]
    last = [s.tobytes()[(c.n_ct - 1) // 64 * 1024:] for s in c.streams] if mode == "up_front" else None
    served = [s.copy() for s in c.streams]
    g = c.whole[2][1]
    bad, record = 0, g * c.group + 5
    served[bad][record, 3] ^= 0x10
    kw = dict(source=lambda inst, first, n: served[inst][first:first + n], commitment="blake3", outboards=obs, expected=c.want, last_chunks=last, restartable=True)
    c.set_inputs()
    assert c.slice(0, 1, **kw) is None and c.slice(1, 2, **kw) is None
    e = _mismatch(gsv, lambda: c.slice(2, 3, **kw))
    assert (e.instance, e.group, e.first_record) == (bad, g, g * c.group)
    assert e.resume_call == c.win[2][0] and c.ev.resume_info() == (c.win[2][0], c.bounds[2])
    served[bad] = c.streams[bad]
    if mode == "up_front":
        _invalid(gsv, lambda: c.slice(2, 3, **dict(kw, last_chunks=None)), "same commitments")  # deferred is another kind of verification
    assert c.slice(2, 3, **kw) is None
    assert c.slice(3, c.n_win, **kw) == c.want
    c.outputs_ok()
    assert c.launched() == c.n_win
    if mode == "deferred":
        # a clean stream under a wrong commitment: found at the end of the pass, nowhere to resume
        wrong = dict(kw, expected=[c.want[1]] + c.want[1:])
        c.set_inputs()
        for w in range(c.n_win - 1):
            assert c.slice(w, w + 1, **wrong) is None
        e = _mismatch(gsv, lambda: c.slice(c.n_win - 1, c.n_win, **wrong))
        assert e.instance == 0 and e.resume_call is None
        with pytest.raises(gsv.GsvError, match="nothing to resume"):
            c.ev.resume_info()
        c.no_outputs()
    c.ev.close()


def test_fallback_repeats_the_slice_alone(engine, monkeypatch, tmp_path):
    """GSV_FAULT_WITHHOLD_DEP=1 withholds a dependency of the first call that has one; at 208 records per window that call lies in window
    1.  Over files the engine repeats that slice alone, from its restart point, on the safe schedule; over a source the slice fails with
    the remedy, rolled back, and the host's repeat succeeds.  The later slices keep the call ranges of the first schedule."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_FAULT_WITHHOLD_DEP", "1")
    c = _Case(gsv, engine, monkeypatch, tmp_path, window=208)
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "0.5")  # (progress based, as in test_forced_dependency_fault_falls_back_to_the_safe_schedule)
    assert c.n_win >= 4 and c.win[1][1] >= 2
    win = list(c.win)
    kw = c.files(commitment="both", restartable=True)
    c.set_inputs()
    macs, _ = c.slice(0, 1, **kw)
    assert macs == c.prefix_macs(1) and c.ev.fallback_count() == 0
    macs, digests = c.slice(1, 2, **kw)
    assert c.ev.fallback_count() == 1 and digests is None and macs == c.prefix_macs(2)
    after = c.ev.schedule_info()
    assert after["n_windows"] == after["n_calls"] and after["windows_launched"] == 1 + win[1][1]  # window 0 once, then the slice's calls one by one
    for w in range(2, len(win)):
        macs, digests = c.ev.evaluate_calls(win[w][0], win[w][1], **kw)
        assert macs == c.prefix_macs(w + 1)
    assert digests == c.want and macs == c.macs_want and c.ev.fallback_count() == 1
    c.outputs_ok()
    c.ev.close()
    # from a source
    ev = gsv.Session(engine, c.sp.plan, c.B, retain_stream=False, window_ct_records=208, drain_segment_records=SEGMENT)
    c.ev = ev
    skw = dict(source=lambda inst, first, n: c.streams[inst][first:first + n], commitment="both", restartable=True)
    c.set_inputs()
    ev.evaluate_calls(win[0][0], win[0][1], **skw)
    with pytest.raises(gsv.GsvError, match="safe schedule.*repeat the slice"):
        ev.evaluate_calls(win[1][0], win[1][1], **skw)
    assert ev.fallback_count() == 1 and ev.resume_info() == (win[1][0], c.bounds[1])
    for w in range(1, len(win)):
        macs, digests = ev.evaluate_calls(win[w][0], win[w][1], **skw)
        assert macs == c.prefix_macs(w + 1)
    assert digests == c.want and ev.fallback_count() == 1
    c.outputs_ok()
    ev.close()
