"""The evaluator's half of the BLAKE3 ciphertext commitment (DESIGN.md §3 "Commitment stage"):

  * streaming evaluation (gsv_session_evaluate_streaming_commit / _source_commit): the segments uploaded to the gate-order buffer go
    through the garbler's chunk, reduce and carry kernels on the stream that scatters them — program sessions (rings), plan sessions in
    windows and over a ciphertext ring;
  * resident streams (gsv_session_ciphertext_blake3): the program-order stream is hashed where it lies, through the position table
    (b3_chunk_indexed_kernel), in launch ranges of GSV_B3_RESIDENT_RECORDS records — program sessions (one ring) and plan sessions (one
    range per call block);
  * sharding.evaluate_from(commitment="blake3"): a cut-and-choose run committed with BLAKE3, finished.

References: tests/b3_ref.py over the reference streams (tests/gate_list_ref.py, the CPU oracle) or the files' bytes, and the garbler's
digests from the drain.  The device under test is never its own reference.
"""
import os

import numpy as np
import pytest

import b3_ref

_ref = {}


def ref_digest(data):
    """b3_ref.blake3, computed once per distinct input of a test session."""
    data = bytes(data)
    if data not in _ref:
        _ref[data] = b3_ref.blake3(data)
    return _ref[data]


def _flip(path, byte, bit=0x10):
    with open(path, "r+b") as f:
        f.seek(byte)
        b = f.read(1)
        f.seek(byte)
        f.write(bytes([b[0] ^ bit]))


# ---- CPU half --------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_from_refuses_an_unknown_commitment(tmp_path):
    """... before anything else happens: neither the table nor the stand-in is looked at."""
    from garbled_snark_verifier_amd import sharding
    called = []
    with pytest.raises(ValueError):
        sharding.evaluate_from(None, [{"index": 0}], "u254_add", str(tmp_path), 1, evaluate=lambda *a: called.append(a), commitment="sha256")
    assert not called


def test_evaluate_from_with_blake3_records_through_the_stand_in(tmp_path):
    """commitment="blake3" on the CPU: the stand-in keeps its signature and returns the hash it chooses, the truncated digest here; the
    default (CBC-MAC) on the same table reports CiphertextMismatch."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    circuit, seed = "u254_add", 5
    g = o.garble(circuit, seed)
    gsv.write_gc_file(os.path.join(str(tmp_path), gsv.gc_file_name(0)), g.ciphertexts)
    digest = ref_digest(g.ciphertexts.tobytes())
    table = np.stack([sharding.commit_record(0, digest[:16], g.output_label0, g.delta, g.false_label0, g.true_label0, g.input_label0)])
    n_in, n_out = g.input_label0.shape[0], g.output_label0.shape[0]
    bits = np.random.default_rng(1).integers(0, 2, n_in).astype(np.uint8)
    case = {"index": 0, "true_constant_wire": g.true_label0 ^ g.delta, "false_constant_wire": g.false_label0,
            "input_active": np.where(bits[:, None] == 1, g.input_label0 ^ g.delta[None, :], g.input_label0), "input_bits": bits}
    ob, _, _ = o.execute(circuit, bits)
    act = np.where(ob[:, None] == 1, g.output_label0 ^ g.delta[None, :], g.output_label0)

    def stand_in(hash_):
        return lambda index, t, f, a, b: (act, ob, hash_)

    res = sharding.evaluate_from(table, [case], circuit, str(tmp_path), n_out, evaluate=stand_in(digest[:16]), commitment="blake3")
    assert [r[0] for r in res] == [0] and (res[0][2] == ob).all()
    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(table, [case], circuit, str(tmp_path), n_out, evaluate=stand_in(g.ct_hash.tobytes()))
    assert (ei.value.kind, ei.value.index) == ("CiphertextMismatch", 0)


# ---- GPU half --------------------------------------------------------------------------------------------------------------------------------
_prog = {}


def _layered():
    """The 37-ciphertext layered program of test_blake3_commit.test_program_session_both_commitments: three instances, 45 replays, and
    their reference streams (1 665 records each) with b3_ref's digests."""
    if "p" not in _prog:
        import garbled_snark_verifier_amd as gsv
        import gate_list_ref as G
        import test_kernel_step_shapes as S
        gates, outputs, _ = S.build_layered([(20, 5), (17, 9)], n_inputs=8)
        prog = gsv.Program.from_gates(8, gates, outputs)
        assert prog.info["n_ciphertexts"] == 37
        seeds, K = [31, 32, 33], 45
        labs = [gsv.labels_from_seed(s, 8) for s in seeds]
        delta = np.stack([x[0] for x in labs]); consts = np.stack([np.stack([x[1], x[2]]) for x in labs]); inputs = np.stack([x[3] for x in labs])
        refs = [np.concatenate([G.garble(gates, delta[i], consts[i], inputs[i], outputs, gate_id_base=r * len(gates)).ciphertexts for r in range(K)]) for i in range(3)]
        bits = np.random.default_rng(31).integers(0, 2, (3, 8)).astype(np.uint8)
        _prog["p"] = dict(prog=prog, K=K, delta=delta, consts=consts, inputs=inputs, refs=refs, bits=bits, want=[ref_digest(r.tobytes()) for r in refs],
                          active=np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs), consts_active=np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1))
    return _prog["p"]


@pytest.mark.gpu
def test_program_session_streaming(engine, monkeypatch, tmp_path):
    """A ring of 7 replays: segments of 259 records, 1 665 in all = 26 chunks and one record; with groups of 4 chunks the device reduces
    six groups, two chunk values stay pending and the host hashes the last, partial chunk."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")
    p = _layered()
    prog, K = p["prog"], p["K"]
    gc = str(tmp_path)
    sess = gsv.Session(engine, prog, 3, K, 7)
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    macs, digests = sess.garble_streaming(directory=gc, first_index=10, commitment="both")
    out0 = sess.read_outputs()
    sess.close()
    files = [os.path.join(gc, gsv.gc_file_name(10 + i)) for i in range(3)]
    for i in range(3):
        assert open(files[i], "rb").read() == p["refs"][i].tobytes() and macs[i] == o.cbcmac(p["refs"][i])
    assert digests == p["want"]

    def evaluator():
        ev = gsv.Session(engine, prog, 3, K, 7)
        ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
        return ev

    ev = evaluator()
    got_macs, got = ev.evaluate_streaming(gc, first_index=10, commitment="both")
    assert got == digests == [ref_digest(open(f, "rb").read()) for f in files] and got_macs == macs
    act, ob = ev.read_outputs(with_bits=True)
    assert (act == np.where(ob[:, :, None] == 1, out0 ^ p["delta"][:, None, :], out0)).all()
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    assert ev.evaluate_streaming(gc, first_index=10, commitment="blake3") == digests  # alone: no MAC worker; a second pass starts afresh
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    assert ev.evaluate_streaming(gc, first_index=10) == macs  # the default is the CBC-MAC, as ever
    with pytest.raises(ValueError):
        ev.evaluate_streaming(gc, first_index=10, commitment="sha256")
    ev.close()
    # one flipped bit of instance 1's file: in the first chunk, in a middle group, in the last partial chunk (the carry the host hashes)
    clean = open(files[1], "rb").read()
    assert len(clean) == 1665 * 16
    for byte in (5, 3 * 4096 + 100, 1664 * 16 + 3):
        _flip(files[1], byte)
        tampered = open(files[1], "rb").read()
        assert tampered != clean
        ev = evaluator()
        got = ev.evaluate_streaming(gc, first_index=10, commitment="blake3")  # the evaluation completes
        ev.close()
        assert got[1] == ref_digest(tampered) and got[1] != digests[1], "byte %d" % byte
        assert got[0] == digests[0] and got[2] == digests[2]
        open(files[1], "wb").write(clean)
    # a file cut short by one record: the source runs dry and both arrays stay as they were
    open(files[2], "wb").write(p["refs"][2].tobytes()[:-16])
    ev = evaluator()
    with pytest.raises(gsv.GsvError, match="exhausted"):
        ev.evaluate_streaming(gc, first_index=10, commitment="both")
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "21")
    with pytest.raises(gsv.GsvError, match="GSV_B3_SUBTREE_LOG2"):
        ev.evaluate_streaming(gc, first_index=10, commitment="blake3")
    ev.close()


def _plan_case(gsv, sp, P, seeds):
    labs = [P.labels(gsv, sp, s) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([x[1] for x in labs]); inputs = np.stack([x[2] for x in labs]); bits = np.stack([x[3] for x in labs])
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    return delta, consts, inputs, bits, active, np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)


def _plan_opts(kind, n_ct):
    """The options of test_blake3_commit.test_plan_session_commitments"""
    if kind == "ring":
        return dict(retain_stream="ring", concurrent_calls=8, drain_segment_records=n_ct // 4)
    return dict(retain_stream=False, window_ct_records=n_ct // 2, drain_segment_records=n_ct // 8)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["windows", "ring"])
@pytest.mark.parametrize("ni", [1, 2, 4])
def test_plan_session_streaming(engine, monkeypatch, tmp_path, ni, kind):
    """The small plan of tests/plan_small_lib.py, 2 ni + 1 instances reading the reference streams' files through a permuted index list."""
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")
    n_ct = sp.plan.info["n_ciphertexts"]
    B = 2 * ni + 1
    perm = [int(x) for x in np.random.default_rng(ni).permutation(B)]
    if perm == sorted(perm):
        perm = perm[1:] + perm[:1]
    seeds = [T.SEED0 + j for j in perm]  # instance i evaluates the stream of seed SEED0 + perm[i], read from gc_<100 + perm[i]>.bin
    for j in range(B):
        gsv.write_gc_file(os.path.join(str(tmp_path), gsv.gc_file_name(100 + j)), P.reference(gsv, sp, T.SEED0 + j)[0].ciphertexts)
    want = [ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    macs_want = [P.reference(gsv, sp, s)[0].ct_hash for s in seeds]
    assert len(set(want)) == B
    _, _, _, bits, active, consts_active = _plan_case(gsv, sp, P, seeds)
    ev = gsv.Session(engine, sp.plan, B, **_plan_opts(kind, n_ct))
    assert ev.instances_per_workgroup == ni
    info = ev.schedule_info()
    if kind == "ring":
        assert info["ct_ring_records"] > 0 and info["n_windows"] == 1 and info["n_segments"] >= 3
    else:
        assert info["n_windows"] >= 2 and info["n_segments"] > info["n_windows"]
    ev.set_evaluate_inputs(consts_active, active, bits)
    macs, digests = ev.evaluate_streaming_indexed(str(tmp_path), [100 + j for j in perm], commitment="both")
    assert digests == want and macs == macs_want
    act, ob = ev.read_outputs(with_bits=True)
    for i, s in enumerate(seeds):
        e = P.reference(gsv, sp, s)[1]
        assert (ob[i] == e.output_bits).all() and (act[i] == e.output_active).all(), "instance %d" % i
    ev.set_evaluate_inputs(consts_active, active, bits)
    assert ev.evaluate_streaming_indexed(str(tmp_path), [100 + j for j in perm], commitment="blake3") == want
    assert ev.fallback_count() == 0
    ev.close()


@pytest.mark.gpu
def test_plan_session_from_a_source(engine, monkeypatch):
    """The generic source with BLAKE3 alone, over a ciphertext ring, with the BLAKE3 gate hasher (one instance per workgroup)."""
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", "1")
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0, T.SEED0 + 1, T.SEED0 + 2]
    streams = [P.reference(gsv, sp, s, 0, "blake3")[0].ciphertexts for s in seeds]
    _, _, _, bits, active, consts_active = _plan_case(gsv, sp, P, seeds)
    ev = gsv.Session(engine, sp.plan, 3, **_plan_opts("ring", n_ct))
    ev.set_hasher("blake3")
    ev.set_evaluate_inputs(consts_active, active, bits)
    got = ev.evaluate_from_source(lambda inst, first, n: streams[inst][first:first + n], commitment="blake3")
    assert got == [ref_digest(s.tobytes()) for s in streams]
    act, ob = ev.read_outputs(with_bits=True)
    for i, s in enumerate(seeds):
        e = P.reference(gsv, sp, s, 0, "blake3")[1]
        assert (ob[i] == e.output_bits).all() and (act[i] == e.output_active).all(), "instance %d" % i
    assert ev.fallback_count() == 0
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [37, 259, None])
@pytest.mark.parametrize("k", [0, 2, 10])
def test_resident_program_session(engine, monkeypatch, k, resident):
    """Launch ranges of 37 records (smaller than a chunk: no range boundary is a chunk boundary), of 259 (groups of 256 records straddle
    them) and the default (one range); a replay holds 37 records, so every lane's 64 records wrap the position table once or twice."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(k))
    if resident is None:
        monkeypatch.delenv("GSV_B3_RESIDENT_RECORDS", raising=False)
    else:
        monkeypatch.setenv("GSV_B3_RESIDENT_RECORDS", str(resident))
    p = _layered()
    sess = gsv.Session(engine, p["prog"], 3, p["K"])
    sess.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    sess.garble()  # asynchronous: the hash kernels queue behind it
    assert sess.ciphertext_blake3() == p["want"]
    out0 = sess.read_outputs()
    sess.close()
    ev = gsv.Session(engine, p["prog"], 3, p["K"])
    ev.set_evaluate_inputs(p["consts_active"], p["active"], p["bits"])
    for i in range(2):
        ev.upload_ciphertexts(i, p["refs"][i])
    with pytest.raises(gsv.GsvError, match="exhausted"):
        ev.ciphertext_blake3()  # instance 2 has not been uploaded
    ev.upload_ciphertexts(2, p["refs"][2])
    assert ev.ciphertext_blake3() == p["want"]
    ev.evaluate()
    ev.sync()
    act, ob = ev.read_outputs(with_bits=True)
    assert (act == np.where(ob[:, :, None] == 1, out0 ^ p["delta"][:, None, :], out0)).all()
    ev.close()


@pytest.mark.gpu
def test_resident_refusals_and_the_empty_stream(engine, monkeypatch):
    import garbled_snark_verifier_amd as gsv
    p = _layered()
    part = gsv.Session(engine, p["prog"], 3, p["K"], 7)  # ct_capacity_replays < replays: only a ring of the stream is there
    with pytest.raises(gsv.GsvError, match="retains only part"):
        part.ciphertext_blake3()
    part.close()
    full = gsv.Session(engine, p["prog"], 3, p["K"])
    full.set_garble_inputs(p["delta"], p["consts"], p["inputs"])
    full.garble()
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "-1")
    with pytest.raises(gsv.GsvError, match="GSV_B3_SUBTREE_LOG2"):
        full.ciphertext_blake3()
    monkeypatch.delenv("GSV_B3_SUBTREE_LOG2")
    assert full.ciphertext_blake3() == p["want"]
    full.close()
    prog = gsv.Program.from_gates(2, [(8, 2, 3, 4), (10, 4, 4, 5)], [4, 5])  # free gates only
    assert prog.info["n_ciphertexts"] == 0
    labs = [gsv.labels_from_seed(s, 2) for s in (1, 2)]
    sess = gsv.Session(engine, prog, 2)
    sess.set_garble_inputs(np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
    sess.garble()
    empty = ref_digest(b"")
    assert empty.hex() == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
    assert sess.ciphertext_blake3() == [empty, empty]
    sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 4])
def test_resident_plan_session(engine, monkeypatch, ni):
    """One launch range per call block (or several: ranges of 100 records); the calls' ciphertext counts are no multiples of 64, so
    chunks straddle the blocks through the carry, and the all-free call in the middle contributes nothing."""
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")
    monkeypatch.delenv("GSV_B3_RESIDENT_RECORDS", raising=False)
    counts = [int(r[3]) for r in sp.plan.call_info()]
    assert any(c % 64 for c in counts) and sum(counts) == sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(2 * ni + 1)]
    B = len(seeds)
    want = [ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    delta, consts, inputs, _, _, _ = _plan_case(gsv, sp, P, seeds)
    sess = gsv.Session(engine, sp.plan, B, retain_stream=True, concurrent_calls=8)
    assert sess.instances_per_workgroup == ni
    sess.set_garble_inputs(delta, consts, inputs)
    sess.garble()
    sess.sync()
    assert sess.ciphertext_blake3() == want
    monkeypatch.setenv("GSV_B3_RESIDENT_RECORDS", "100")
    assert sess.ciphertext_blake3() == want
    assert sess.fallback_count() == 0
    sess.close()
    window = gsv.Session(engine, sp.plan, B, retain_stream=False)
    with pytest.raises(gsv.GsvError, match="retains only part"):
        window.ciphertext_blake3()
    window.close()


@pytest.mark.gpu
def test_cut_and_choose_with_blake3_end_to_end(engine, tmp_path):
    """garble_and_commit(commitment="blake3") -> evaluate_from(commitment="blake3"): a run committed with BLAKE3 can be finished; the
    default evaluator's CBC-MAC is not what these records commit to."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    circuit, total = "fq_mul", 4
    prog = gsv.Program.from_circuit(circuit)
    gc = str(tmp_path)
    seeds = [int(x) for x in sharding.instance_seeds(77, total)]
    n_in, n_out = prog.info["n_inputs"], prog.info["n_outputs"]
    commits = sharding.garble_and_commit(circuit, seeds, list(range(total)), engine=engine, program=prog, gc_dir=gc, commitment="blake3")
    rng = np.random.default_rng(9)

    def case(i):
        d, f, t, inp = gsv.labels_from_seed(seeds[i], n_in)
        bits = rng.integers(0, 2, n_in).astype(np.uint8)
        return {"index": i, "true_constant_wire": t ^ d, "false_constant_wire": f, "input_active": np.where(bits[:, None] == 1, inp ^ d[None, :], inp), "input_bits": bits}

    cases = [case(i) for i in (2, 0, 3, 1)]
    res = sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog, commitment="blake3")
    assert [r[0] for r in res] == [2, 0, 3, 1]
    for c, (i, act, ob) in zip(cases, res):
        eb, _, _ = o.execute(circuit, c["input_bits"])
        assert (ob == eb).all()
    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog)
    assert (ei.value.kind, ei.value.index) == ("CiphertextMismatch", 2)
    _flip(os.path.join(gc, gsv.gc_file_name(3)), 4321, 4)
    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(commits, cases, circuit, gc, n_out, engine=engine, program=prog, commitment="blake3")
    assert (ei.value.kind, ei.value.index) in (("CiphertextMismatch", 3), ("OutputLabelMismatch", 3))
    prog.close()
