"""The BLAKE3 ciphertext commitment: commit_i = BLAKE3(gc_<i>.bin bytes), plain hash mode, computed on the device by the chunk / reduce /
carry kernels of blake3_device.hpp and finished by the host hasher of host_crypto.hpp (DESIGN.md §3 "Commitment stage").

Three implementations meet here, none derived from another: tests/b3_ref.py (pure Python, recursive tree split), the engine's host hasher
(incremental, chaining-value stack, takes pre-reduced subtrees) and LLVM's copy of the official C code (the recorded digests of
tests/golden/blake3_known_answers.json, and live where the toolchain's library can be loaded).

  * CPU half: both implementations against the fixture and against LLVM; gsv_blake3_update in random pieces; the subtree-absorbing form —
    the host's half of the device split — against b3_ref for group sizes 2^k, k = 0, 1, 2, 3, 5, on lengths around every group boundary;
    blake3_file on a gc file; sharding's commit records and file check with commitment="blake3".
  * GPU half: (a) the kernels alone on random streams, every segmentation that moves a chunk, carry or group boundary; (b) a program
    session with both commitments and gc files in one pass; (c) plan sessions: several windows and segments, a ciphertext ring, a pass
    in two slices, a drained sample; (d) an empty stream.

Not covered: chunk counters above 2^32 (4 TiB of stream per instance).
"""
import json
import os

import numpy as np
import pytest

import b3_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "blake3_known_answers.json")
LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 6144, 7168, 8192, 8193, 16384, 31744, 102400]


def pattern(n):
    return bytes(i % 251 for i in range(n))


_ref = {}


def ref_digest(data):
    """b3_ref.blake3, computed once per distinct input of a test session."""
    data = bytes(data)
    if data not in _ref:
        _ref[data] = b3_ref.blake3(data)
    return _ref[data]


def _llvm():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_blake3_golden", os.path.join(HERE, "golden", "make_blake3_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- CPU half --------------------------------------------------------------------------------------------------------------------------------
def test_reference_and_host_hasher_match_the_recorded_digests():
    import garbled_snark_verifier_amd as gsv
    gold = json.load(open(GOLDEN))["digests"]
    assert sorted(int(n) for n in gold) == LENGTHS == _llvm().LENGTHS
    for n in LENGTHS:
        want = bytes.fromhex(gold[str(n)])
        assert ref_digest(pattern(n)) == want, "b3_ref, %d bytes" % n
        assert gsv.blake3(pattern(n)) == want, "gsv.blake3, %d bytes" % n
    # the anchors of the official test vectors that tests/test_blake3_hasher.py carries for n <= 64
    assert gold["0"] == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
    assert gold["64"] == "4eed7141ea4a5cd4b788606bd23f46e212af9cacebacdc7d1f4c6dc7f2511b98"


def test_reference_and_host_hasher_match_llvm_blake3():
    import garbled_snark_verifier_amd as gsv
    h = _llvm().llvm_blake3()
    if h is None:
        pytest.skip("LLVM's BLAKE3 (libclang-cpp.so of the ROCm toolchain) cannot be loaded here")
    rng = np.random.default_rng(7)
    for n in LENGTHS[:-1] + [1024 * 9 + 16, 1024 * 21]:
        for data in (pattern(n), rng.integers(0, 256, n, dtype=np.uint8).tobytes()):
            want = h(data)
            assert ref_digest(data) == want and gsv.blake3(data) == want, n


def test_update_in_random_pieces_equals_one_shot():
    import garbled_snark_verifier_amd as gsv
    rng = np.random.default_rng(11)
    for n in (0, 1, 1024, 5 * 1024 + 1, 40_000, 102400):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        want = gsv.blake3(data)
        for _ in range(4):
            h, off = gsv.Blake3(), 0
            while off < n:
                m = int(rng.integers(1, 5 * 1024 + 1))
                h.update(data[off:off + m])
                off += m
            assert h.digest() == want, n
    assert gsv.Blake3().update(b"").digest() == gsv.blake3(b"")


def _absorb_split(gsv, data, k):
    """The device split, with b3_ref standing in for the device: all chunks but the last, aligned groups of 2^k of them as one value."""
    G = 1 << k
    n_chunks = max(1, -(-len(data) // 1024))
    dev = n_chunks - 1
    h = gsv.Blake3()
    for g in range(dev // G):
        h.absorb_subtree(b3_ref.subtree_cv(data[g * G * 1024:(g + 1) * G * 1024], g * G), k)
    for c in range(dev // G * G, dev):
        h.absorb_subtree(b3_ref.chunk_cv(data[c * 1024:(c + 1) * 1024], c), 0)
    h.update(data[dev * 1024:])
    return h.digest()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5])
def test_absorbing_subtrees_equals_hashing_the_bytes(k):
    import garbled_snark_verifier_amd as gsv
    G = 1 << k
    lengths = set(LENGTHS)
    for m in (1, 2, 3):  # 16-byte-multiple lengths around every boundary of m groups, and of m groups + the last chunk
        for d in (-16, 0, 16):
            lengths |= {m * G * 1024 + d, (m * G + 1) * 1024 + d}
    data = np.random.default_rng(100 + k).integers(0, 256, max(lengths), dtype=np.uint8).tobytes()
    for n in sorted(lengths):
        assert _absorb_split(gsv, data[:n], k) == ref_digest(data[:n]), "k = %d, %d bytes" % (k, n)


def test_absorb_subtree_rejects_what_is_not_a_subtree_boundary():
    import garbled_snark_verifier_amd as gsv
    cv = bytes(32)
    with pytest.raises(gsv.GsvError):
        gsv.Blake3().update(b"x").absorb_subtree(cv, 0)  # inside a chunk
    with pytest.raises(gsv.GsvError):
        gsv.Blake3().absorb_subtree(cv, 0).absorb_subtree(cv, 1)  # chunk count 1 is no multiple of 2
    with pytest.raises(gsv.GsvError):
        gsv.Blake3().absorb_subtree(cv, 0).digest()  # the last chunk must be bytes


def test_blake3_file_on_a_gc_file(tmp_path):
    import garbled_snark_verifier_amd as gsv
    cts = np.random.default_rng(3).integers(0, 256, (64 * 5 + 9, 16), dtype=np.uint8)
    path = os.path.join(str(tmp_path), gsv.gc_file_name(4))
    gsv.write_gc_file(path, cts)
    assert gsv.blake3_file(path) == ref_digest(cts.tobytes()) == gsv.blake3(cts)
    empty = os.path.join(str(tmp_path), gsv.gc_file_name(5))
    open(empty, "wb").close()
    assert gsv.blake3_file(empty) == ref_digest(b"")
    with pytest.raises(gsv.GsvError):
        gsv.blake3_file(os.path.join(str(tmp_path), "missing.bin"))


def test_sharding_commit_records_with_blake3(tmp_path):
    """cut_and_choose_commit and run_regarbling with commitment="blake3", through the CPU stand-in for the GPU garbler (the CPU oracle's
    garbling here): the record's 16-byte hash field is the truncated digest of the stream, the file check hashes the same way."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    circuit, total = "u254_add", 3
    seen = []

    def garble(c, seeds, indexes, commitment="cbcmac"):
        seen.append(commitment)
        recs = []
        for sd, idx in zip(seeds, indexes):
            g = o.garble(c, sd)
            gsv.write_gc_file(os.path.join(str(tmp_path), gsv.gc_file_name(idx)), g.ciphertexts)
            h = gsv.blake3(g.ciphertexts)[:16] if commitment == "blake3" else g.ct_hash.tobytes()
            recs.append(sharding.commit_record(idx, h, g.output_label0, g.delta, g.false_label0, g.true_label0, g.input_label0))
        return np.stack(recs)

    table, seeds = sharding.cut_and_choose_commit(circuit, 99, total, 0, 1, garble=garble, commitment="blake3")
    assert seen == ["blake3"]
    for i in range(total):
        g = o.garble(circuit, int(seeds[i]))
        exp = sharding.commit_record(i, ref_digest(g.ciphertexts.tobytes())[:16], g.output_label0, g.delta, g.false_label0, g.true_label0, g.input_label0)
        assert (table[i] == exp).all()
    assert sharding.run_regarbling(table, [0, 1, 2], {}, circuit, str(tmp_path), commitment="blake3") == (True, {})
    ok, errors = sharding.run_regarbling(table, [0, 1, 2], {}, circuit, str(tmp_path))  # the CBC-MAC of the file is not what these records commit to
    assert not ok and set(errors) == {0, 1, 2}
    with open(os.path.join(str(tmp_path), gsv.gc_file_name(1)), "r+b") as f:
        f.seek(100)
        b = f.read(1)
        f.seek(100)
        f.write(bytes([b[0] ^ 0x80]))
    ok, errors = sharding.run_regarbling(table, [0, 1, 2], {}, circuit, str(tmp_path), commitment="blake3")
    assert not ok and errors == {1: "ciphertext corrupted"}
    table2, _ = sharding.cut_and_choose_commit(circuit, 99, total, 0, 1, garble=garble)  # the default: called without the keyword, CBC-MAC records
    assert seen == ["blake3", "cbcmac"] and (table2[:, 8:24] != table[:, 8:24]).any()
    with pytest.raises(ValueError):
        sharding.cut_and_choose_commit(circuit, 99, total, 0, 1, garble=garble, commitment="sha256")


# ---- GPU half --------------------------------------------------------------------------------------------------------------------------------
RECORDS = [0, 1, 63, 64, 65, 127, 128, 129, 64 * 4 - 1, 64 * 4, 64 * 4 + 1, 64 * 8 + 1, 64 * 37 + 5]
_streams = {}


def _random_streams():
    """Five random streams of the longest length; a test's streams are prefixes (in both directions), references are cached by content."""
    if "a" not in _streams:
        _streams["a"] = np.random.default_rng(2024).integers(0, 256, (5, max(RECORDS), 16), dtype=np.uint8)
    return _streams["a"]


def _segmentations(n):
    """one segment; segments of 1 record; of 37 (no boundary is a chunk boundary, several hold less than a chunk); of 259 (with k = 2: groups
    of 256 records straddle them)"""
    out = [[n]]
    for step in (1, 37, 259):
        out.append([min(step, n - i) for i in range(0, n, step)])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams", [1, 3, 5])
@pytest.mark.parametrize("k", [0, 2, 10])
def test_device_kernels_alone(engine, monkeypatch, k, n_streams):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", str(k))
    full = _random_streams()
    for n in RECORDS:
        a = np.ascontiguousarray(full[:n_streams, :n])
        want = [ref_digest(a[i].tobytes()) for i in range(n_streams)]
        for seg in _segmentations(n):
            got = gsv.blake3_streams(engine, a, seg)
            assert got == want, "k = %d, %d streams of %d records, segments of %s" % (k, n_streams, n, seg[:3])
    with pytest.raises(gsv.GsvError):
        gsv.blake3_streams(engine, full[:1, :10], [4, 5])  # the segments must add up


@pytest.mark.gpu
def test_device_kernels_cross_the_default_group_size(engine, monkeypatch):
    """64 * 1100 + 7 records = 1100 chunks + a tail: one complete group of 2^10 chunks, 75 chunk values behind it, the last chunk on the host."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.delenv("GSV_B3_SUBTREE_LOG2", raising=False)
    n = 64 * 1100 + 7
    a = np.random.default_rng(5).integers(0, 256, (2, n, 16), dtype=np.uint8)
    want = [ref_digest(a[i].tobytes()) for i in range(2)]
    assert gsv.blake3_streams(engine, a, [n]) == want
    assert gsv.blake3_streams(engine, a, [64 * 700 + 3, 64 * 400 + 4]) == want  # the group straddles the two segments


@pytest.mark.gpu
def test_program_session_both_commitments(engine, tmp_path):
    """37 AND-family gates a replay (no multiple of 64), 45 replays through a ring of 7: segments of 259 records, 1 665 in all."""
    import garbled_snark_verifier_amd as gsv
    import gate_list_ref as G
    import test_kernel_step_shapes as S
    gates, outputs, _ = S.build_layered([(20, 5), (17, 9)], n_inputs=8)
    prog = gsv.Program.from_gates(8, gates, outputs)
    n_ct = prog.info["n_ciphertexts"]
    assert n_ct == 37 and prog.info["n_gates"] == len(gates)
    seeds, K = [31, 32, 33], 45
    labs = [gsv.labels_from_seed(s, 8) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([np.stack([x[1], x[2]]) for x in labs]); inputs = np.stack([x[3] for x in labs])
    refs = [np.concatenate([G.garble(gates, delta[i], consts[i], inputs[i], outputs, gate_id_base=r * len(gates)).ciphertexts for r in range(K)]) for i in range(3)]
    d_both, d_both2 = str(tmp_path / "both"), str(tmp_path / "b3")
    os.mkdir(d_both); os.mkdir(d_both2)
    sess = gsv.Session(engine, prog, 3, K, 7)
    sess.set_garble_inputs(delta, consts, inputs)
    macs, digests = sess.garble_streaming(directory=d_both, first_index=10, threads=2, commitment="both")
    sess.close()
    import oracle_lib as o
    for i in range(3):
        data, file_mac = gsv.read_gc_file(os.path.join(d_both, gsv.gc_file_name(10 + i)))
        assert data.shape == (K * n_ct, 16) and (data == refs[i]).all(), "stream of instance %d" % i
        assert macs[i] == o.cbcmac(refs[i]) == file_mac
        assert digests[i] == ref_digest(data.tobytes()) == gsv.blake3_file(os.path.join(d_both, gsv.gc_file_name(10 + i)))
    fresh = gsv.Session(engine, prog, 3, K, 7)
    fresh.set_garble_inputs(delta, consts, inputs)
    assert fresh.garble_streaming(commitment="blake3") == digests
    assert fresh.garble_streaming(directory=d_both2, commitment="blake3") == digests  # a second pass starts afresh; files without MAC workers
    assert open(os.path.join(d_both2, gsv.gc_file_name(1)), "rb").read() == refs[1].tobytes()
    assert fresh.garble_streaming() == macs  # the default is the CBC-MAC, as ever
    fresh.close()


def _plan_inputs(gsv, sp, P, seeds):
    labs = [P.labels(gsv, sp, s) for s in seeds]
    return np.stack([x[0] for x in labs]), np.stack([x[1] for x in labs]), np.stack([x[2] for x in labs])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["windows", "ring", "slices"])
@pytest.mark.parametrize("ni", [1, 2, 4])
def test_plan_session_commitments(engine, monkeypatch, tmp_path, ni, kind):
    """The small plan of tests/plan_small_lib.py (AES): the digests equal b3_ref over the flat reference stream."""
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")   # 256-record groups: several per stream, straddling the segments
    monkeypatch.setenv("GSV_DEP_WAIT_SECONDS", "5")  # (a stall would end the pass with an error after seconds, not a minute)
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(2 * ni + 1)]
    B = len(seeds)
    want = [ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    macs_want = [P.reference(gsv, sp, s)[0].ct_hash for s in seeds]
    if kind == "ring":
        opts = dict(retain_stream="ring", concurrent_calls=8, drain_segment_records=n_ct // 4)
    else:
        opts = dict(retain_stream=False, window_ct_records=n_ct // 2, drain_segment_records=n_ct // 8)
    sess = gsv.Session(engine, sp.plan, B, **opts)
    assert sess.instances_per_workgroup == ni
    info = sess.schedule_info()
    if kind == "ring":
        assert info["ct_ring_records"] > 0 and info["n_windows"] == 1 and info["n_segments"] >= 3
    else:
        assert info["n_windows"] >= 2 and info["n_segments"] > info["n_windows"]
    sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    if kind == "slices":
        w = sess.windows()
        cut = w[len(w) // 2][0]
        n_calls = info["n_calls"]
        assert 0 < cut < n_calls
        assert sess.garble_calls(0, cut, commitment="blake3") is None  # reported by the slice that ends the pass only
        with pytest.raises(gsv.GsvError, match="same commitments"):
            sess.garble_calls(cut, n_calls - cut, commitment="both")  # the MAC states have not seen the first slice
        sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
        macs, digests = sess.garble_calls(0, cut, commitment="both")
        assert digests is None
        macs, digests = sess.garble_calls(cut, n_calls - cut, commitment="both")
        assert digests == want and macs == macs_want
        sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
        assert sess.garble_streaming(commitment="blake3") == want  # one slice: the same digests
    else:
        macs, digests = sess.garble_streaming(directory=str(tmp_path), commitment="both")
        assert digests == want and macs == macs_want
        for i in range(B):
            assert gsv.blake3_file(os.path.join(str(tmp_path), gsv.gc_file_name(i))) == want[i]
        sess.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
        assert sess.garble_streaming(commitment="blake3") == want  # alone: nothing of the stream leaves the device
    assert sess.fallback_count() == 0
    sess.close()


@pytest.mark.gpu
def test_plan_session_drained_sample(engine, monkeypatch):
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_plan_small as T
    _, sp = T.small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", "1")
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "2")
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0 + i for i in range(4)]
    want = [ref_digest(P.reference(gsv, sp, s)[0].ciphertexts.tobytes()) for s in seeds]
    opts = dict(retain_stream=False, window_ct_records=n_ct // 2, drain_segment_records=n_ct // 8)
    full = gsv.Session(engine, sp.plan, 4, **opts)
    full.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert full.garble_streaming(commitment="blake3") == want
    full.close()
    sample = gsv.Session(engine, sp.plan, 4, **opts)
    sample.set_drain_instances(2)
    sample.set_garble_inputs(*_plan_inputs(gsv, sp, P, seeds))
    assert sample.garble_streaming(commitment="blake3") == want[:2]
    sample.close()


@pytest.mark.gpu
def test_empty_stream(engine):
    """A program of free gates only: no ciphertexts, every instance commits to BLAKE3 of the empty string."""
    import garbled_snark_verifier_amd as gsv
    prog = gsv.Program.from_gates(2, [(8, 2, 3, 4), (10, 4, 4, 5)], [4, 5])
    assert prog.info["n_ciphertexts"] == 0
    labs = [gsv.labels_from_seed(s, 2) for s in (1, 2)]
    sess = gsv.Session(engine, prog, 2)
    sess.set_garble_inputs(np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
    empty = ref_digest(b"")
    assert empty.hex() == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
    assert sess.garble_streaming(commitment="blake3") == [empty, empty]
    macs, digests = sess.garble_streaming(commitment="both")
    assert digests == [empty, empty] and macs == [bytes(16), bytes(16)]
    sess.close()
    assert gsv.blake3_streams(engine, np.zeros((3, 0, 16), np.uint8), []) == [empty] * 3
    with pytest.raises(gsv.GsvError):
        gsv.blake3_streams(engine, np.zeros((0, 4, 16), np.uint8), [4])  # no streams


@pytest.mark.gpu
def test_contradictory_arguments_are_refused(engine, monkeypatch):
    import garbled_snark_verifier_amd as gsv
    prog = gsv.Program.from_gates(2, [(0, 2, 3, 4)], [4])
    labs = [gsv.labels_from_seed(1, 2)]
    sess = gsv.Session(engine, prog, 1)
    sess.set_garble_inputs(np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
    with pytest.raises(ValueError):
        sess.garble_streaming(discard=True, commitment="blake3")
    with pytest.raises(ValueError):
        sess.garble_streaming(discard=True, commitment="sha256")
    with pytest.raises(ValueError):
        sess.garble_streaming(commitment="sha256")
    monkeypatch.setenv("GSV_B3_SUBTREE_LOG2", "100")
    with pytest.raises(gsv.GsvError, match="GSV_B3_SUBTREE_LOG2"):
        sess.garble_streaming(commitment="blake3")
    with pytest.raises(gsv.GsvError, match="GSV_B3_SUBTREE_LOG2"):
        gsv.blake3_streams(engine, np.zeros((1, 4, 16), np.uint8), [4])
    monkeypatch.delenv("GSV_B3_SUBTREE_LOG2")
    assert len(sess.garble_streaming(commitment="blake3")[0]) == 32
    sess.close()
