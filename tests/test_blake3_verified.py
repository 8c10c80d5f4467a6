"""Received ciphertext files verified per group of chunks against a BLAKE3 outboard (include/gsv_engine.h "BLAKE3 outboards"), on the
device: the garbler writes the outboards while it commits (gsv_session_garble_streaming_commit_outboard), the streaming evaluator checks
them against the commitments before it uploads anything and stops at the first group that differs
(gsv_session_evaluate_streaming_verified), and gsv_engine_blake3_files verifies files without evaluating them.

References: gsv.blake3_file_outboard / blake3_file on the host (themselves checked against tests/b3_ref.py in test_blake3_outboard.py),
b3_ref's digests of the reference streams and the CPU oracle's outputs (test_blake3_evaluate's fixtures).  GSV_B3_SUBTREE_LOG2=2
throughout: groups of 4 chunks = 256 records = 4 096 bytes, so that tiny streams have many groups.  A tampered file is data: nothing
here provokes a device fault."""
import os

import numpy as np
import pytest

import test_blake3_evaluate as E

pytestmark = pytest.mark.gpu
K = 2
GROUP_RECORDS = 64 << K


def _b3o(gsv, d, i):
    return os.path.join(d, gsv.outboard_file_name(i))


def _gc(gsv, d, i):
    return os.path.join(d, gsv.gc_file_name(i))


def _mismatch(gsv, call):
    with pytest.raises(gsv.CiphertextMismatch) as ei:
        call()
    assert "gsv status 5:" in str(ei.value)
    return ei.value


def _no_outputs(gsv, sess):
    with pytest.raises(gsv.GsvError, match="nothing ran"):
        sess.read_outputs()


def _program_files(gsv, engine, d):
    """The layered program garbled into d: gc_10 .. gc_12 with their outboards; returns (fixture, digests, garbler's outputs)."""
    p = E._layered()
    sess = gsv.Session(engine, p["prog"], 3, p["K"], 7)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    digests = sess.garble_streaming(directory=d, first_index=10, commitment="blake3", outboard_dir=d)
    out0 = sess.read_outputs()
    with pytest.raises(ValueError):
        sess.garble_streaming(directory=d, first_index=10, outboard_dir=d)  # an outboard belongs to a BLAKE3 commitment
    sess.close()
    return p, digests, out0


def test_program_session_outboards_and_verified_streaming(engine, monkeypatch, tmp_path):
    """1 665 records per instance in rings of 259: six groups, two pending chunk values and a last chunk of one record."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    d, host = str(tmp_path), str(tmp_path / "host")
    os.mkdir(host)
    p, digests, out0 = _program_files(gsv, engine, d)
    assert digests == p["want"]
    for i in range(3):
        assert open(_gc(gsv, d, 10 + i), "rb").read() == p["refs"][i].tobytes()
        assert gsv.blake3_file_outboard(_gc(gsv, d, 10 + i), K, _b3o(gsv, host, i)) == digests[i]
        ob = open(_b3o(gsv, d, 10 + i), "rb").read()
        assert ob == open(_b3o(gsv, host, i), "rb").read() and len(ob) == 24 + 32 * (6 + 2)

    def evaluator():
        ev = gsv.Session(engine, p["prog"], 3, p["K"], 7)
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
        return ev

    def outputs_ok(ev):
        act, ob = ev.read_outputs(with_bits=True)
        assert (act == np.where(ob[:, :, None] == 1, out0 ^ p["delta"][:, None, :], out0)).all()

    ev = evaluator()
    assert ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests) == digests
    outputs_ok(ev)
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    macs, got = ev.evaluate_streaming(d, first_index=10, commitment="both", outboard_dir=d, expected=[x[:16] for x in digests])  # expected_len = 16
    assert got == digests and len(macs) == 3
    outputs_ok(ev)
    with pytest.raises(gsv.GsvError, match="no mismatch"):
        ev.mismatch_info()
    with pytest.raises(ValueError):
        ev.evaluate_streaming(d, first_index=10, outboard_dir=d, expected=digests)  # the CBC-MAC alone has no outboard
    with pytest.raises(ValueError):
        ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d)
    ev.close()
    # a wrong commitment: refused up front, by instance, and nothing ran
    ev = evaluator()
    wrong = [digests[0], digests[1], digests[1]]
    e = _mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=wrong))
    assert (e.instance, e.group, e.first_record) == (2, None, None) and "outboard or last chunk of instance 2 does not match the commitment" in str(e)
    _no_outputs(gsv, ev)
    ev.close()
    # one flipped bit of instance 1's file
    clean = open(_gc(gsv, d, 11), "rb").read()
    assert len(clean) == 1665 * 16
    for byte, group, record, up_front in ((5, 0, 0, False), (3 * 4096 + 100, 3, 3 * 256, False), (5 * 4096 + 50, 5, 5 * 256, False), (6 * 4096 + 1024 + 10, 6, 6 * 256 + 64, False),
                                          (1664 * 16 + 3, None, None, True)):
        E._flip(_gc(gsv, d, 11), byte)
        ev = evaluator()
        e = _mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests))
        assert (e.instance, e.group, e.first_record) == (1, group, record), byte  # the other instances' files are never blamed
        assert ev.mismatch_info() == (1, group, record)
        assert ("does not match the commitment" in str(e)) == up_front
        _no_outputs(gsv, ev)
        # the session is usable again: the clean files verify
        open(_gc(gsv, d, 11), "wb").write(clean)
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
        assert ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests) == digests
        outputs_ok(ev)
        ev.close()
    # a flipped bit in the outboard instead (a group value, the header's n_records): before any upload
    ob = open(_b3o(gsv, d, 11), "rb").read()
    ev = evaluator()
    E._flip(_b3o(gsv, d, 11), 24 + 32 * 4 + 9)
    e = _mismatch(gsv, lambda: ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests))
    assert (e.instance, e.group) == (1, None)
    _no_outputs(gsv, ev)
    open(_b3o(gsv, d, 11), "wb").write(ob)
    E._flip(_b3o(gsv, d, 11), 16, 1)
    with pytest.raises(gsv.GsvError, match="1664 records, the stream here holds 1665"):
        ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests)
    open(_b3o(gsv, d, 11), "wb").write(ob[:-32])
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*holds"):
        ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests)
    open(_b3o(gsv, d, 11), "wb").write(ob)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "3")  # the pass's k against the outboards': both values are named
    with pytest.raises(gsv.GsvError, match=r"gsv status 1: .*2\^2 chunks.*2\^3"):
        ev.evaluate_streaming(d, first_index=10, commitment="blake3", outboard_dir=d, expected=digests)
    ev.close()


def _plan_setup(gsv, monkeypatch, ni):
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")
    return P, T, sp


def _window_bounds(sess, sp):
    """first record of every window of the session's schedule, and the stream's length behind them"""
    counts = [int(r[3]) for r in sp.plan.call_info()]
    return [sum(counts[:w[0]]) for w in sess.windows()] + [sum(counts)]


@pytest.mark.parametrize("ni", [1, 4])
def test_plan_session_verified_streaming(engine, monkeypatch, tmp_path, ni):
    """The small plan, 2 ni + 1 instances reading the reference streams' files through a permuted index list, in launch windows."""
    import garbled_snark_verifier_amd as gsv
    P, T, sp = _plan_setup(gsv, monkeypatch, ni)
    d = str(tmp_path)
    n_ct = sp.plan.info["n_ciphertexts"]
    B = 2 * ni + 1
    perm = [int(x) for x in np.random.default_rng(ni).permutation(B)]
    if perm == sorted(perm):
        perm = perm[1:] + perm[:1]
    seeds = [T.SEED0 + j for j in perm]
    for j in range(B):
        gsv.write_gc_file(_gc(gsv, d, 100 + j), P.reference(gsv, sp, T.SEED0 + j)[0].ciphertexts)
        gsv.blake3_file_outboard(_gc(gsv, d, 100 + j), K, _b3o(gsv, d, 100 + j))
    want = [E.ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    idx = [100 + j for j in perm]
    _, _, _, bits, active, consts_active = E._plan_case(gsv, sp, P, seeds)
    ev = gsv.Session(engine, sp.plan, B, **E._plan_opts("windows", n_ct))
    assert ev.instances_per_workgroup == ni
    info = ev.schedule_info()
    assert info["n_windows"] >= 2 and info["n_segments"] > info["n_windows"]
    ev.set_evaluate_inputs(consts_active, active, bits)
    assert ev.evaluate_streaming_indexed(d, idx, commitment="blake3", outboard_dir=d, expected=want) == want
    assert ev.schedule_info()["windows_launched"] == info["n_windows"]
    act, ob = ev.read_outputs(with_bits=True)
    for i, s in enumerate(seeds):
        e = P.reference(gsv, sp, s)[1]
        assert (ob[i] == e.output_bits).all() and (act[i] == e.output_active).all(), "instance %d" % i
    # where the windows lie in the stream: the second window starts inside a group (so that group straddles the boundary) and holds
    # that group's end
    w = _window_bounds(ev, sp)
    g = w[1] // GROUP_RECORDS
    assert w[1] % GROUP_RECORDS and w[1] < (g + 1) * GROUP_RECORDS <= w[2] and (g + 1) * GROUP_RECORDS <= n_ct, w
    bad = 1  # the instance whose file is tampered with: it reads gc_<idx[1]>.bin
    path = _gc(gsv, d, idx[bad])
    clean = open(path, "rb").read()
    for record in (w[1] + 3, w[1] - 2):  # inside the second window's records; in the straddling group's part of the first window
        assert record // GROUP_RECORDS == g
        E._flip(path, record * 16 + 7)
        ev.set_evaluate_inputs(consts_active, active, bits)
        e = _mismatch(gsv, lambda: ev.evaluate_streaming_indexed(d, idx, commitment="blake3", outboard_dir=d, expected=want))
        assert (e.instance, e.group, e.first_record) == (bad, g, g * GROUP_RECORDS), record
        assert ev.schedule_info()["windows_launched"] == 1 < info["n_windows"]  # the group ends in the second window: that window was not launched, nor any later one
        _no_outputs(gsv, ev)
        open(path, "wb").write(clean)
    ev.set_evaluate_inputs(consts_active, active, bits)
    assert ev.evaluate_streaming_indexed(d, idx, commitment="blake3", outboard_dir=d, expected=[x[:16] for x in want]) == want
    assert ev.fallback_count() == 0
    ev.close()
    ring = gsv.Session(engine, sp.plan, B, **E._plan_opts("ring", n_ct))
    ring.set_evaluate_inputs(consts_active, active, bits)
    with pytest.raises(gsv.GsvError, match="gsv status 1: verified streaming is not available for plan sessions over a ciphertext ring"):
        ring.evaluate_streaming_indexed(d, idx, commitment="blake3", outboard_dir=d, expected=want)
    assert ring.evaluate_streaming_indexed(d, idx, commitment="blake3") == want  # unverified, the ring serves as ever
    ring.close()


def test_sliced_garbling_writes_the_same_outboards(engine, monkeypatch, tmp_path):
    """Two slices on a window boundary, a whole pass, and a drained sample: the outboards are the host writer's of the gc files."""
    import garbled_snark_verifier_amd as gsv
    import test_blake3_commit as C
    P, T, sp = _plan_setup(gsv, monkeypatch, 1)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(3)]
    whole, sliced, sample, host = (str(tmp_path / x) for x in ("whole", "sliced", "sample", "host"))
    for x in (whole, sliced, sample, host):
        os.mkdir(x)
    sess = gsv.Session(engine, sp.plan, 3, **E._plan_opts("windows", n_ct))
    sess.set_garble_inputs(*C._plan_inputs(gsv, sp, P, seeds))
    digests = sess.garble_streaming(directory=whole, commitment="blake3", outboard_dir=whole)
    assert digests == [E.ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    win = sess.windows()
    cut, n_calls = win[len(win) // 2][0], sess.schedule_info()["n_calls"]
    assert 0 < cut < n_calls
    sess.set_garble_inputs(*C._plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_calls(0, cut, directory=sliced, commitment="blake3", outboard_dir=sliced) is None
    with pytest.raises(gsv.GsvError, match="same commitments"):
        sess.garble_calls(cut, n_calls - cut, directory=sliced, commitment="blake3")  # a slice that would leave the outboards behind
    sess.set_garble_inputs(*C._plan_inputs(gsv, sp, P, seeds))
    assert sess.garble_calls(0, cut, directory=sliced, commitment="blake3", outboard_dir=sliced) is None  # the restart truncates
    assert sess.garble_calls(cut, n_calls - cut, directory=sliced, commitment="blake3", outboard_dir=sliced) == digests
    sess.close()
    for i in range(3):
        assert gsv.blake3_file_outboard(_gc(gsv, whole, i), K, _b3o(gsv, host, i)) == digests[i]
        ob = open(_b3o(gsv, host, i), "rb").read()
        assert open(_b3o(gsv, whole, i), "rb").read() == ob == open(_b3o(gsv, sliced, i), "rb").read()
    part = gsv.Session(engine, sp.plan, 3, **E._plan_opts("windows", n_ct))
    part.set_drain_instances(2)
    part.set_garble_inputs(*C._plan_inputs(gsv, sp, P, seeds))
    assert part.garble_streaming(commitment="blake3", outboard_dir=sample) == digests[:2]  # nothing but the values leaves the device
    part.close()
    assert sorted(os.listdir(sample)) == [gsv.outboard_file_name(0), gsv.outboard_file_name(1)]
    for i in range(2):
        assert open(_b3o(gsv, sample, i), "rb").read() == open(_b3o(gsv, host, i), "rb").read()


@pytest.mark.parametrize("segment", [None, 600, 37])
def test_blake3_files(engine, monkeypatch, tmp_path, segment):
    """The program case's files (26 640 bytes each) and the plan case's, hashed on the device without a session: in one segment, in
    segments of 600 records (group 2, records 512 .. 767, straddles the first two) and of 37 (smaller than a chunk)."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(K))
    if segment is None:
        monkeypatch.delenv("GSV_DRAIN_SEGMENT_RECORDS", raising=False)
    else:
        monkeypatch.setenv("GSV_DRAIN_SEGMENT_RECORDS", str(segment))
    d = str(tmp_path)
    p = E._layered()
    files = [_gc(gsv, d, 10 + i) for i in range(3)]
    obs = [_b3o(gsv, d, 10 + i) for i in range(3)]
    for i in range(3):
        gsv.write_gc_file(files[i], p["refs"][i])
        assert gsv.blake3_file_outboard(files[i], K, obs[i]) == p["want"][i]
    assert gsv.blake3_files(engine, files) == p["want"] == [gsv.blake3_file(f) for f in files]
    assert gsv.blake3_files(engine, files, obs) == p["want"]
    assert gsv.blake3_files(engine, files[1:2], obs[1:2]) == p["want"][1:2]
    clean = open(files[1], "rb").read()
    for byte, group in ((5, 0), (3 * 4096 + 100, 3), (5 * 4096 + 50, 5), (6 * 4096 + 1024 + 10, 6)):
        E._flip(files[1], byte)
        e = _mismatch(gsv, lambda: gsv.blake3_files(engine, files, obs))
        assert (e.instance, e.group) == (1, group), byte
        tampered = gsv.blake3_files(engine, files)  # without outboards: the digests of what is there
        assert tampered[1] == gsv.blake3_file(files[1]) != p["want"][1] and tampered[0] == p["want"][0] and tampered[2] == p["want"][2]
        open(files[1], "wb").write(clean)
    E._flip(files[1], 1664 * 16 + 3)  # the last chunk: no value of the outboard covers it, the digest does
    got = gsv.blake3_files(engine, files, obs)
    assert got[1] == gsv.blake3_file(files[1]) != p["want"][1] and got[0] == p["want"][0]
    open(files[1], "wb").write(clean)
    # refusals: unequal lengths, an outboard of another k, a truncated outboard
    open(files[2], "wb").write(clean[:-16])
    with pytest.raises(gsv.GsvError, match="gsv status 1: the files must be equally long"):
        gsv.blake3_files(engine, files)
    gsv.write_gc_file(files[2], p["refs"][2])
    gsv.blake3_file_outboard(files[2], K + 1, obs[2])
    with pytest.raises(gsv.GsvError, match=r"gsv status 1: .*2\^3 chunks"):
        gsv.blake3_files(engine, files, obs)
    open(obs[2], "wb").write(open(obs[1], "rb").read()[:-1])
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*holds"):
        gsv.blake3_files(engine, files, obs)
    if segment == 600:
        # the plan case's files (775 records: three groups and a last chunk of seven records), and the empty file
        import plan_small_lib as P
        import test_plan_small as T
        _, sp = T.small_plan()
        pf, po = [], []
        for j in range(3):
            pf.append(_gc(gsv, d, 100 + j)); po.append(_b3o(gsv, d, 100 + j))
            gsv.write_gc_file(pf[j], P.reference(gsv, sp, T.SEED0 + j)[0].ciphertexts)
            gsv.blake3_file_outboard(pf[j], K, po[j])
        want = [E.ref_digest(P.reference(gsv, sp, T.SEED0 + j)[0].ciphertexts.tobytes()) for j in range(3)]
        assert gsv.blake3_files(engine, pf, po) == want
        E._flip(pf[2], 700 * 16)
        e = _mismatch(gsv, lambda: gsv.blake3_files(engine, pf, po))
        assert (e.instance, e.group) == (2, 2)
        empty = _gc(gsv, d, 200)
        open(empty, "wb").close()
        gsv.blake3_file_outboard(empty, K, _b3o(gsv, d, 200))
        assert gsv.blake3_files(engine, [empty], [_b3o(gsv, d, 200)]) == [E.ref_digest(b"")]


def test_cut_and_choose_with_outboards_end_to_end(engine, tmp_path):
    """garble_and_commit(outboard_dir=) -> run_regarbling(engine=, outboard_dir=) -> evaluate_from(outboard_dir=): the receiving side of a
    run committed with BLAKE3, verified per group (k = 10, the default: 1 MiB groups)."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    circuit, total = "fq_mul", 4
    prog = gsv.Program.from_circuit(circuit)
    gc = str(tmp_path)
    seeds = [int(x) for x in sharding.instance_seeds(77, total)]
    n_in, n_out = prog.info["n_inputs"], prog.info["n_outputs"]
    commits = sharding.garble_and_commit(circuit, seeds, list(range(total)), engine=engine, program=prog, gc_dir=gc, commitment="blake3", outboard_dir=gc)
    for i in range(total):
        host = os.path.join(gc, "host.b3o")
        assert gsv.blake3_file_outboard(_gc(gsv, gc, i), 10, host)[:16] == bytes(commits[i, 8:24])
        assert open(host, "rb").read() == open(_b3o(gsv, gc, i), "rb").read()
    keep = [0, 2, 3]
    assert sharding.run_regarbling(commits, keep, {1: seeds[1]}, circuit, gc, engine=engine, program=prog, commitment="blake3", outboard_dir=gc) == (True, {})
    assert sharding.run_regarbling(commits, keep, {1: seeds[1]}, circuit, gc, engine=engine, program=prog, commitment="blake3") == (True, {})
    rng = np.random.default_rng(9)

    def case(i):
        d, f, t, inp = gsv.labels_from_seed(seeds[i], n_in)
        bits = rng.integers(0, 2, n_in).astype(np.uint8)
        return {"index": i, "true_constant_wire": t ^ d, "false_constant_wire": f, "input_active": np.where(bits[:, None] == 1, inp ^ d[None, :], inp), "input_bits": bits}

    cases = [case(i) for i in (2, 0, 3)]
    res = sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog, commitment="blake3", outboard_dir=gc)
    assert [r[0] for r in res] == [2, 0, 3]
    for c, (i, act, ob) in zip(cases, res):
        eb, _, _ = o.execute(circuit, c["input_bits"])
        assert (ob == eb).all()
    n_bytes = os.path.getsize(_gc(gsv, gc, 3))
    in_group_0 = n_bytes > 5 * 1024  # byte 4321 lies in chunk 4: covered by a value of the outboard unless that is the stream's last chunk
    E._flip(_gc(gsv, gc, 3), 4321, 4)
    ok, errors = sharding.run_regarbling(commits, keep, {1: seeds[1]}, circuit, gc, engine=engine, program=prog, commitment="blake3", outboard_dir=gc)
    assert not ok and set(errors) == {3} and errors[3].startswith("ciphertext corrupted")
    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog, commitment="blake3", outboard_dir=gc)
    assert (ei.value.kind, ei.value.index) == ("CiphertextMismatch", 3) and "group" in str(ei.value)
    if in_group_0:
        assert errors[3] == "ciphertext corrupted (group 0)" and ei.value.details["group"] == 0
    prog.close()
