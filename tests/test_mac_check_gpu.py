"""CBC-MAC commitments verified on the device against chain checkpoints (include/gsv_engine.h "CBC-MAC checkpoints"): the check kernel
alone over every segmentation and corruption (gsv_engine_cbcmac_streams_check), received files (gsv_engine_cbcmac_files), the garbler
writing checkpoint files while it drains and verifying against them without draining (program and plan sessions), and
sharding.run_regarbling(checkpoint_dir=).

References: the host writer gsv.cbcmac_file_checkpoints and the host checker gsv.cbcmac_file_check (themselves checked against gsv.cbcmac
and the CPU oracle in test_mac_checkpoints_host.py).  A tampered file or stream is data: nothing here provokes a device fault."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KS = (0, 2, 6)
_cache = {}


def _flip(path, byte, bit=0x10):
    with open(path, "r+b") as f:
        f.seek(byte)
        b = f.read(1)
        f.seek(byte)
        f.write(bytes([b[0] ^ bit]))


def _streams():
    """Five random streams of the longest length; a test's streams are prefixes."""
    if "a" not in _cache:
        _cache["a"] = np.random.default_rng(4242).integers(0, 256, (5, 1500, 16), dtype=np.uint8)
    return _cache["a"]


def _checkpoints(gsv, tmp, a, k):
    """the checkpoint files' bytes of the streams a[i], by the host writer"""
    out = []
    for i in range(a.shape[0]):
        p, c = os.path.join(tmp, "s.bin"), os.path.join(tmp, "s.mck")
        open(p, "wb").write(a[i].tobytes())
        gsv.cbcmac_file_checkpoints(p, k, c)
        out.append(open(c, "rb").read())
    return out


def _host_check(gsv, tmp, stream, ck):
    """the host checker's answer for one stream: None or the group"""
    p, c = os.path.join(tmp, "h.bin"), os.path.join(tmp, "h.mck")
    open(p, "wb").write(stream.tobytes())
    open(c, "wb").write(ck)
    return gsv.cbcmac_file_check(p, c, 2)[1]


def _segmentations(n, k):
    """one segment; segments of 1 record (a chain is carried across many segments); of 37; and [2^k - 1, 2^k + 1, rest]: a segment that
    starts exactly on a group boundary and one that ends one record short of it"""
    G = 1 << k
    out = [[n]]
    for step in (1, 37):
        out.append([min(step, n - i) for i in range(0, n, step)])
    if n >= 2 * G and G > 1:
        out.append([G - 1, G + 1] + ([n - 2 * G] if n > 2 * G else []))
    return out


def _record_counts(k):
    G = 1 << k
    return [0, 1, G - 1, G, G + 1, 259, 1500]


def _flip_state(ck, g):
    b = bytearray(ck)
    b[24 + 16 * g + 3] ^= 0x40
    return bytes(b)


@pytest.mark.parametrize("n_streams", [1, 3, 5])
@pytest.mark.parametrize("k", KS)
def test_check_kernel_alone(engine, tmp_path, k, n_streams):
    """Intact streams pass under every segmentation; each corruption, one at a time, yields exactly (stream, group) — the host checker's
    answer, the same under every segmentation."""
    import garbled_snark_verifier_amd as gsv
    tmp, G = str(tmp_path), 1 << k
    full = _streams()
    victim = n_streams // 2
    for n in _record_counts(k):
        a = np.ascontiguousarray(full[:n_streams, :n])
        cks = _checkpoints(gsv, tmp, a, k)
        assert len(cks[0]) == gsv.cbcmac_checkpoints_size(n, k)
        last = (n - 1) >> k if n else 0
        # (what is corrupted, the group it must be blamed on)
        rec_cases = [(r, r >> k) for r in sorted({0, G - 1, G, n - 1}) if 0 <= r < n]
        state_cases = [(g, g) for g in sorted({last // 2, last})] if n else []
        want_host = {}
        for r, g in rec_cases:
            b = a.copy(); b[victim, r, 11] ^= 0x02
            want_host[("r", r)] = _host_check(gsv, tmp, b[victim], cks[victim])
            assert want_host[("r", r)] == g
        for s, g in state_cases:
            want_host[("s", s)] = _host_check(gsv, tmp, a[victim], _flip_state(cks[victim], s))
            assert want_host[("s", s)] == g
        for seg in _segmentations(n, k):
            what = "k = %d, %d streams of %d records, segments of %s" % (k, n_streams, n, seg[:3])
            assert gsv.cbcmac_streams_check(engine, a, seg, cks) is None, what
            for r, g in rec_cases:
                b = a.copy(); b[victim, r, 11] ^= 0x02
                assert gsv.cbcmac_streams_check(engine, b, seg, cks) == (victim, want_host[("r", r)]), what + ", record %d" % r
            for s, g in state_cases:
                bad = list(cks); bad[victim] = _flip_state(cks[victim], s)
                assert gsv.cbcmac_streams_check(engine, a, seg, bad) == (victim, want_host[("s", s)]), what + ", state %d" % s


def test_check_kernel_reports_the_lowest_group_then_the_lowest_stream(engine, tmp_path):
    import garbled_snark_verifier_amd as gsv
    k, n = 2, 259
    a = np.ascontiguousarray(_streams()[:4, :n])
    cks = _checkpoints(gsv, str(tmp_path), a, k)
    for seg in _segmentations(n, k):
        b = a.copy(); b[1, 200, 0] ^= 1; b[3, 90, 0] ^= 1       # groups 50 and 22
        assert gsv.cbcmac_streams_check(engine, b, seg, cks) == (3, 22)
        b = a.copy(); b[3, 101, 0] ^= 1; b[2, 103, 5] ^= 1      # both in group 25
        assert gsv.cbcmac_streams_check(engine, b, seg, cks) == (2, 25)
    found, seconds = gsv.cbcmac_streams_check(engine, a, [n], cks, with_seconds=True)
    assert found is None and 0 < seconds < 10


def test_check_kernel_refusals(engine, tmp_path):
    import garbled_snark_verifier_amd as gsv
    a = np.ascontiguousarray(_streams()[:2, :10])
    cks = _checkpoints(gsv, str(tmp_path), a, 1)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*add up"):
        gsv.cbcmac_streams_check(engine, a, [4, 5], cks)  # the segments must add up
    other = _checkpoints(gsv, str(tmp_path), np.ascontiguousarray(_streams()[:2, :10]), 2)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*agree on k"):
        gsv.cbcmac_streams_check(engine, a, [10], [cks[0], other[1] + bytes(32)])  # (padded to the same length: still another k)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*wrong magic"):
        gsv.cbcmac_streams_check(engine, a, [10], [b"x" + cks[0][1:], cks[1]])
    nine = _checkpoints(gsv, str(tmp_path), np.ascontiguousarray(_streams()[:2, :9]), 1)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*9 records"):
        gsv.cbcmac_streams_check(engine, a, [10], nine)
    assert gsv.cbcmac_streams_check(engine, np.zeros((3, 0, 16), np.uint8), [], _checkpoints(gsv, str(tmp_path), np.zeros((3, 0, 16), np.uint8), 4)) is None


def test_files(engine, monkeypatch, tmp_path):
    """Three files of 1 665 records, k = 3, in segments of 259 records."""
    import garbled_snark_verifier_amd as gsv
    k, n, d = 3, 1665, str(tmp_path)
    monkeypatch.setenv("GSV_DRAIN_SEGMENT_RECORDS", "259")
    data = np.random.default_rng(77).integers(0, 256, (3, n, 16), dtype=np.uint8)
    paths, cks, macs = [], [], []
    for i in range(3):
        paths.append(os.path.join(d, gsv.gc_file_name(i))); cks.append(os.path.join(d, gsv.checkpoint_file_name(i)))
        open(paths[i], "wb").write(data[i].tobytes())
        macs.append(gsv.cbcmac_file_checkpoints(paths[i], k, cks[i]))
        assert macs[i] == gsv.cbcmac(data[i])
    assert gsv.cbcmac_files(engine, paths, cks) == macs
    assert gsv.cbcmac_files(engine, paths, cks, expected=macs) == macs
    wrong = [macs[0], macs[1], macs[0]]
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        gsv.cbcmac_files(engine, paths, cks, expected=wrong)  # before any upload: no place
    assert (ei.value.instance, ei.value.group, ei.value.first_record) == (2, None, None) and "gsv status 5:" in str(ei.value)
    r = 1000
    _flip(paths[1], 16 * r + 2)
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        gsv.cbcmac_files(engine, paths, cks, expected=macs)
    assert (ei.value.instance, ei.value.group, ei.value.first_record) == (1, r >> k, (r >> k) << k)
    assert gsv.cbcmac_file_check(paths[1], cks[1]) == (None, r >> k)
    _flip(paths[1], 16 * r + 2)
    # files of one call that disagree on k; a checkpoint file of another length; an empty file
    k2 = os.path.join(d, "k2.mck")
    gsv.cbcmac_file_checkpoints(paths[2], 2, k2)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*must agree"):
        gsv.cbcmac_files(engine, paths, [cks[0], cks[1], k2])
    short = os.path.join(d, "short.bin")
    open(short, "wb").write(data[0, :100].tobytes())
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*equally long"):
        gsv.cbcmac_files(engine, [paths[0], short], cks[:2])
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*1665 records.*100"):
        gsv.cbcmac_files(engine, [short], [cks[0]])
    empty, empty_ck = os.path.join(d, "empty.bin"), os.path.join(d, "empty.mck")
    open(empty, "wb").close()
    gsv.cbcmac_file_checkpoints(empty, k, empty_ck)
    assert gsv.cbcmac_files(engine, [empty], [empty_ck]) == [bytes(16)]


def _layered():
    import test_blake3_evaluate as E
    return E._layered()


def test_program_session(engine, monkeypatch, tmp_path):
    """The 37-ciphertext layered program: 3 seeds, 45 replays through a ring of 7 (segments of 259 records, 1 665 in all), k = 3."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    p, k = _layered(), 3
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", str(k))
    d, host = str(tmp_path), str(tmp_path / "host")
    os.mkdir(host)
    sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    macs = sess.garble_streaming(directory=d, first_index=10, threads=2, checkpoint_dir=d)
    out0 = sess.read_outputs()
    with pytest.raises(ValueError):
        sess.garble_streaming(directory=d, first_index=10, commitment="blake3", checkpoint_dir=d)  # the files hold the states of the CBC-MAC
    sess.close()
    for i in range(3):
        gc = os.path.join(d, gsv.gc_file_name(10 + i))
        assert macs[i] == o.cbcmac(p["refs"][i]) == gsv.read_gc_file(gc)[1]
        assert gsv.cbcmac_file_checkpoints(gc, k, os.path.join(host, gsv.checkpoint_file_name(i))) == macs[i]
        assert open(os.path.join(d, gsv.checkpoint_file_name(10 + i)), "rb").read() == open(os.path.join(host, gsv.checkpoint_file_name(i)), "rb").read()
    fresh = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    fresh.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    assert fresh.garble_check(d, first_index=10) == macs
    assert (fresh.read_outputs() == out0).all()
    assert fresh.garble_check(d, indexes=[10, 11, 12], expected=macs) == macs
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        fresh.garble_check(d, first_index=10, expected=[macs[0], macs[0], macs[2]])
    assert (ei.value.instance, ei.value.group, ei.value.first_record) == (1, None, None)
    assert fresh.garble_streaming() == macs  # a plain pass afterwards: the CBC-MACs on the host, as ever
    fresh.close()
    # instance 1 garbled from another seed: its stream differs from the first record on
    other = gsv.labels_from_seed(99, 8)
    delta, consts, inputs = p["delta"].copy(), p["consts"].copy(), p["inputs"].copy()
    delta[1], consts[1, 0], consts[1, 1], inputs[1] = other
    bad = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    bad.set_garble_inputs(delta, consts, inputs)
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        bad.garble_check(d, first_index=10)
    assert (ei.value.instance, ei.value.group, ei.value.first_record) == (1, 0, 0) and "gsv status 5:" in str(ei.value)
    assert bad.mismatch_info() == (1, 0, 0)
    bad.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    assert bad.garble_check(d, first_index=10) == macs  # the session is as good as new
    assert bad.garble_streaming() == macs
    bad.close()


def _plan_inputs(gsv, sp, P, seeds):
    labs = [P.labels(gsv, sp, s) for s in seeds]
    return np.stack([x[0] for x in labs]), np.stack([x[1] for x in labs]), np.stack([x[2] for x in labs])


@pytest.mark.parametrize("ni", [1, 2, 4])
def test_plan_session(engine, monkeypatch, tmp_path, ni):
    """The small plan of tests/plan_small_lib.py, 2 ni + 1 instances, windows of n_ct // 2 and segments of n_ct // 8 records, groups larger
    than a segment: they straddle segments and windows.  One pass and two slices cut at a window boundary."""
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    n_ct = sp.plan.info["n_ciphertexts"]
    k = (n_ct // 8).bit_length()  # n_ct / 8 < 2^k <= n_ct / 4
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", str(k))
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")  # (a stall would end the pass with an error after seconds, not a minute)
    seeds = [T.SEED0 + i for i in range(2 * ni + 1)]
    B = len(seeds)
    macs_want = [P.reference(gsv, sp, s)[0].ct_hash for s in seeds]
    one, two, host = str(tmp_path / "one"), str(tmp_path / "two"), str(tmp_path / "host")
    for q in (one, two, host):
        os.mkdir(q)
    opts = dict(retain_stream=False, window_ct_records=n_ct // 2, drain_segment_records=n_ct // 8)
    sess = gsv.Session(engine, sp.plan, B, **opts)
    assert sess.instances_per_workgroup == ni
    info = sess.schedule_info()
    assert info["n_windows"] >= 2 and info["n_segments"] > info["n_windows"] and info["segment_ct_records"] < (1 << k)
    w = sess.windows()
    cut, n_calls = w[len(w) // 2][0], info["n_calls"]
    assert 0 < cut < n_calls
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_streaming(directory=one, checkpoint_dir=one) == macs_want
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    sess.garble_calls(0, cut, directory=two, checkpoint_dir=two)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*same as its first slice"):
        sess.garble_calls(cut, n_calls - cut, directory=two)  # the checkpoint files would miss this slice's states
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    sess.garble_calls(0, cut, directory=two, checkpoint_dir=two)
    assert sess.garble_calls(cut, n_calls - cut, directory=two, checkpoint_dir=two) == macs_want
    for i in range(B):
        gc = os.path.join(one, gsv.gc_file_name(i))
        assert gsv.cbcmac_file_checkpoints(gc, k, os.path.join(host, gsv.checkpoint_file_name(i))) == macs_want[i]
        want = open(os.path.join(host, gsv.checkpoint_file_name(i)), "rb").read()
        assert len(want) > 24 + 3 * 16
        assert open(os.path.join(one, gsv.checkpoint_file_name(i)), "rb").read() == want
        assert open(os.path.join(two, gsv.checkpoint_file_name(i)), "rb").read() == want
    # verified where it is garbled: one pass, then two slices
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_check(one, expected=macs_want) == macs_want
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_check(one, first_call=0, n_calls=cut) is None
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*same as its first slice"):
        sess.garble_calls(cut, n_calls - cut)  # another check than the slice before it
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_check(one, first_call=0, n_calls=cut) is None
    assert sess.garble_check(one, first_call=cut, n_calls=n_calls - cut) == macs_want
    # a stream that differs in the second slice only: the last instance's file states from the middle on
    last = B - 1
    ck = os.path.join(one, gsv.checkpoint_file_name(last))
    n_states = (os.path.getsize(ck) - 24) // 16
    g = n_states - 2
    _flip(ck, 24 + 16 * g + 1)
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        sess.garble_check(one)
    assert (ei.value.instance, ei.value.group, ei.value.first_record) == (last, g, g << k)
    assert sess.fallback_count() == 0
    sess.close()
    ring = gsv.Session(engine, sp.plan, B, retain_stream="ring", concurrent_calls=8, drain_segment_records=n_ct // 4)
    ring.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*ring"):
        ring.garble_check(two)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*ring"):
        ring.garble_streaming(checkpoint_dir=host)
    ring.close()


def test_regarbling_with_checkpoints(engine, monkeypatch, tmp_path):
    """garble_and_commit(checkpoint_dir=) -> run_regarbling(engine=, checkpoint_dir=): finalized files verified on the device, opened
    instances re-garbled and verified where they are garbled."""
    import garbled_snark_verifier_amd as gsv
    from garbled_snark_verifier_amd import sharding
    k = 8
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", str(k))
    circuit, total = "fq_mul", 5
    prog = gsv.Program.from_circuit(circuit)
    gc = str(tmp_path)
    seeds = [int(x) for x in sharding.instance_seeds(78, total)]
    commits = sharding.garble_and_commit(circuit, seeds, list(range(total)), engine=engine, program=prog, gc_dir=gc, checkpoint_dir=gc)
    for i in range(total):
        host = os.path.join(gc, "host.mck")
        assert gsv.cbcmac_file_checkpoints(os.path.join(gc, gsv.gc_file_name(i)), k, host) == bytes(commits[i, 8:24])
        assert open(host, "rb").read() == open(os.path.join(gc, gsv.checkpoint_file_name(i)), "rb").read()
    keep, opened = [0, 2, 3], {1: seeds[1], 4: seeds[4]}
    assert sharding.run_regarbling(commits, keep, opened, circuit, gc, engine=engine, program=prog, checkpoint_dir=gc) == (True, {})
    assert sharding.run_regarbling(commits, keep, opened, circuit, gc, engine=engine, program=prog) == (True, {})  # today's path
    n = os.path.getsize(os.path.join(gc, gsv.gc_file_name(3))) // 16
    r = n // 2
    assert (r >> k) > 0
    _flip(os.path.join(gc, gsv.gc_file_name(3)), 16 * r + 9)
    ok, errors = sharding.run_regarbling(commits, keep, opened, circuit, gc, engine=engine, program=prog, checkpoint_dir=gc)
    assert not ok and errors == {3: "ciphertext corrupted (group %d)" % (r >> k)}
    _flip(os.path.join(gc, gsv.gc_file_name(3)), 16 * r + 9)
    ok, errors = sharding.run_regarbling(commits, keep, {1: seeds[1], 4: seeds[4] + 1}, circuit, gc, engine=engine, program=prog, checkpoint_dir=gc)
    assert not ok and errors == {4: "regarbling failed"}
    prog.close()
