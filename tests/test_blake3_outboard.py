"""BLAKE3 outboards on the host (include/gsv_engine.h "BLAKE3 outboards", csrc/engine/outboard.hpp): the format, gsv_blake3_file_outboard
and gsv_blake3_outboard_root against tests/b3_ref.py, the independent pure-Python BLAKE3 — group and chunk values are derived there —
what is refused, the drain-side writer in its stand-alone harness (tests/drain_pipeline/outboard_writer_test.cpp), and
sharding.run_regarbling / evaluate_from with outboard_dir through the CPU stand-ins.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import b3_ref

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (0, 1, 3)


def lengths(k):
    G = 1 << k
    return [0, 1, 63, 64, 65, 64 * G, 64 * G + 1, 64 * (2 * G) + 64, 64 * (3 * G + 2) + 5]


_streams = {}


def stream(n_records):
    """n_records x 16 bytes, the same for every test of the session"""
    if n_records not in _streams:
        _streams[n_records] = np.random.default_rng(1000 + n_records).integers(0, 256, n_records * 16, dtype=np.uint8).tobytes()
    return _streams[n_records]


_expected = {}


def expected_outboard(n_records, k):
    """(outboard bytes, last chunk, digest) from b3_ref alone"""
    key = (n_records, k)
    if key not in _expected:
        data, G = stream(n_records), 1 << k
        N = max(1, -(-n_records // 64))
        n_groups, n_pend = (N - 1) // G, (N - 1) % G
        ob = b"GSVB3OB\n" + struct.pack("<IIQ", 1, k, n_records)
        for g in range(n_groups):
            ob += b3_ref.subtree_cv(data[g * G * 1024:(g + 1) * G * 1024], g * G)
        for c in range(n_groups * G, n_groups * G + n_pend):
            ob += b3_ref.chunk_cv(data[c * 1024:(c + 1) * 1024], c)
        _expected[key] = (ob, data[(N - 1) * 1024:], b3_ref.blake3(data))
    return _expected[key]


def _invalid(gsv, outboard, last):
    with pytest.raises(gsv.GsvError, match="gsv status 1:") as ei:
        gsv.blake3_outboard_root(outboard, last)
    return str(ei.value)


@pytest.mark.parametrize("k", KS)
def test_file_outboard_and_root_against_the_reference(tmp_path, k):
    """For every length: the host writer writes exactly the reference's bytes and returns the reference's digest, and the outboard
    folds, with the last chunk, to that digest."""
    import garbled_snark_verifier_amd as gsv
    assert gsv.outboard_file_name(12) == "gc_12.b3o"
    for L in lengths(k):
        ob, last, digest = expected_outboard(L, k)
        assert len(last) == (16 * L - 1024 * (max(1, -(-L // 64)) - 1)) and (len(last) > 0) == (L > 0)
        path, ob_path = str(tmp_path / "gc.bin"), str(tmp_path / gsv.outboard_file_name(0))
        open(path, "wb").write(stream(L))
        assert gsv.blake3_file_outboard(path, k, ob_path) == digest == gsv.blake3_file(path), L
        assert open(ob_path, "rb").read() == ob, L
        assert gsv.blake3_outboard_root(ob, last) == digest, L
        assert gsv.blake3_file_outboard(path, k) == digest  # nowhere to write: the digest alone


@pytest.mark.parametrize("k", KS)
def test_a_flipped_bit_changes_the_root_or_is_refused(k):
    """... in every byte of the header, in each group value, in a pending chunk value and in the last chunk"""
    import garbled_snark_verifier_amd as gsv
    G = 1 << k
    L = 64 * (3 * G + 1) + 5  # 3 G + 1 chunks in front of the last: three groups and one pending chunk value; k = 0: four groups, none pending
    ob, last, digest = expected_outboard(L, k)
    n_values = (len(ob) - 24) // 32
    assert n_values == 4

    def flipped(data, byte, bit):
        a = bytearray(data)
        a[byte] ^= bit
        return bytes(a)

    def differs(outboard, chunk):
        try:
            return gsv.blake3_outboard_root(outboard, chunk) != digest
        except gsv.GsvError as e:
            assert "gsv status 1:" in str(e)
            return True

    for byte in range(24):
        for bit in (1, 0x80):
            assert differs(flipped(ob, byte, bit), last), (byte, bit)
    for v in range(n_values):
        for off in (0, 13, 31):
            assert gsv.blake3_outboard_root(flipped(ob, 24 + 32 * v + off, 4), last) != digest, (v, off)
    for byte in (0, len(last) // 2, len(last) - 1):
        assert gsv.blake3_outboard_root(ob, flipped(last, byte, 0x20)) != digest


def test_malformed_outboards_are_refused():
    import garbled_snark_verifier_amd as gsv
    k = 3
    L = 64 * (3 * 8 + 2) + 5
    ob, last, digest = expected_outboard(L, k)
    assert gsv.blake3_outboard_root(ob, last) == digest
    assert "holds" in _invalid(gsv, ob[:-1], last) and "holds" in _invalid(gsv, ob[:-32], last)       # truncated
    assert "holds" in _invalid(gsv, ob + b"\0", last) and "holds" in _invalid(gsv, ob + ob[-32:], last)  # extended
    assert "header" in _invalid(gsv, ob[:23], last) and "header" in _invalid(gsv, b"", last)
    assert "magic" in _invalid(gsv, b"X" + ob[1:], last)
    assert "version" in _invalid(gsv, ob[:8] + struct.pack("<I", 2) + ob[12:], last)
    assert "2^21" in _invalid(gsv, ob[:12] + struct.pack("<I", 21) + ob[16:], last)                    # k = 21
    assert "2^" in _invalid(gsv, ob[:12] + struct.pack("<I", 0xFFFFFFFF) + ob[16:], last)
    for n in (L + 64, L - 64, 0, 1 << 59, (1 << 64) - 1):                                               # n_records against the length
        assert _invalid(gsv, ob[:16] + struct.pack("<Q", n) + ob[24:], last)
    assert "last chunk" in _invalid(gsv, ob[:16] + struct.pack("<Q", L + 1) + ob[24:], last)           # same length, another last chunk
    for bad_last in (b"", last[:-16], last + bytes(16), last[:-1], bytes(1040)):
        assert "last chunk" in _invalid(gsv, ob, bad_last)
    empty, _, d0 = expected_outboard(0, k)
    assert gsv.blake3_outboard_root(empty, b"") == d0 == b3_ref.blake3(b"")
    assert "last chunk" in _invalid(gsv, empty, bytes(16))


def test_file_outboard_refusals(tmp_path):
    import garbled_snark_verifier_amd as gsv
    path = str(tmp_path / "gc.bin")
    open(path, "wb").write(stream(65))
    with pytest.raises(gsv.GsvError, match="k in"):
        gsv.blake3_file_outboard(path, 21)
    with pytest.raises(gsv.GsvError, match="cannot open"):
        gsv.blake3_file_outboard(str(tmp_path / "none.bin"), 3)
    with pytest.raises(gsv.GsvError, match="cannot create"):
        gsv.blake3_file_outboard(path, 3, str(tmp_path / "none" / "x.b3o"))
    open(path, "ab").write(b"\1")
    with pytest.raises(gsv.GsvError, match="whole 16-byte records"):
        gsv.blake3_file_outboard(path, 3)


def test_outboard_writer_against_stand_ins():
    """OutboardFiles behind the B3Absorbers, as the drain drives them: values arriving in several submissions, a later slice and a slice
    restart, removal on failure, and the writer fed with real values against the host writer."""
    d = os.path.join(HERE, "drain_pipeline")
    subprocess.check_call(["make", "-C", d, "-f", "outboard.mk"], stdout=subprocess.DEVNULL)
    exe = os.path.join(d, "outboard_writer_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("outboard_writer: ok")
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "amdhip" not in needed and "gsv_engine" not in needed


def _oracle_table(tmp_path, circuit, seeds):
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    gs, recs = [], []
    for i, seed in enumerate(seeds):
        g = o.garble(circuit, seed)
        path = os.path.join(str(tmp_path), gsv.gc_file_name(i))
        gsv.write_gc_file(path, g.ciphertexts)
        digest = gsv.blake3_file_outboard(path, 0, os.path.join(str(tmp_path), gsv.outboard_file_name(i)))
        assert digest == b3_ref.blake3(g.ciphertexts.tobytes())
        recs.append(sharding.commit_record(i, digest[:16], g.output_label0, g.delta, g.false_label0, g.true_label0, g.input_label0))
        gs.append(g)
    return gs, np.stack(recs)


def _flip(path, byte, bit=0x10):
    with open(path, "r+b") as f:
        f.seek(byte)
        b = f.read(1)
        f.seek(byte)
        f.write(bytes([b[0] ^ bit]))


def test_run_regarbling_with_outboards_on_the_host(tmp_path):
    """Without an engine the finalized files are hashed on the host; with outboard_dir a corrupted file is reported with its group."""
    import garbled_snark_verifier_amd as gsv
    from garbled_snark_verifier_amd import sharding
    circuit = "u254_add"
    gs, table = _oracle_table(tmp_path, circuit, [5, 6, 7])
    d = str(tmp_path)
    n_bytes = gs[0].ciphertexts.size
    assert n_bytes > 3 * 1024  # groups of one chunk (k = 0 in _oracle_table): the byte below lies in group 1
    assert sharding.run_regarbling(table, [0, 1, 2], {}, circuit, d, commitment="blake3", outboard_dir=d) == (True, {})
    with pytest.raises(ValueError):
        sharding.run_regarbling(table, [0, 1, 2], {}, circuit, d, outboard_dir=d)
    _flip(os.path.join(d, gsv.gc_file_name(1)), 1024 + 100)
    ok, errors = sharding.run_regarbling(table, [0, 1, 2], {}, circuit, d, commitment="blake3", outboard_dir=d)
    assert not ok and errors == {1: "ciphertext corrupted (group 1)"}
    assert sharding.run_regarbling(table, [0, 1, 2], {}, circuit, d, commitment="blake3")[1] == {1: "ciphertext corrupted"}
    _flip(os.path.join(d, gsv.gc_file_name(1)), 1024 + 100)
    _flip(os.path.join(d, gsv.gc_file_name(2)), n_bytes - 3)  # the last chunk: no value of the outboard covers it, the digest does
    ok, errors = sharding.run_regarbling(table, [0, 1, 2], {}, circuit, d, commitment="blake3", outboard_dir=d)
    assert not ok and errors == {2: "ciphertext corrupted"}
    os.remove(os.path.join(d, gsv.outboard_file_name(0)))
    ok, errors = sharding.run_regarbling(table, [0, 1], {}, circuit, d, commitment="blake3", outboard_dir=d)
    assert not ok and errors[0].startswith("failed to get ciphertext source") and 1 not in errors
    assert errors[2] == "failed to find seed" and len(errors) == 2  # (instance 2 is not kept here: it counts as opened, and no seed was given)


def test_evaluate_from_with_outboards_through_the_stand_in(tmp_path):
    """outboard_dir with a stand-in: the outboard and the last chunk are checked against the committed hash on the host before the
    stand-in is called; a stand-in that raises CiphertextMismatch is reported as the ConsistencyError of its case, with the group."""
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    circuit = "u254_add"
    gs, table = _oracle_table(tmp_path, circuit, [5, 6])
    d = str(tmp_path)
    n_out = gs[0].output_label0.shape[0]
    rng = np.random.default_rng(3)
    called = []

    def case(i):
        g = gs[i]
        bits = rng.integers(0, 2, g.input_label0.shape[0]).astype(np.uint8)
        return {"index": i, "true_constant_wire": g.true_label0 ^ g.delta, "false_constant_wire": g.false_label0,
                "input_active": np.where(bits[:, None] == 1, g.input_label0 ^ g.delta[None, :], g.input_label0), "input_bits": bits}

    def stand_in(index, t, f, a, b):
        called.append(index)
        g = gs[index]
        ob, _, _ = o.execute(circuit, b)
        return np.where(ob[:, None] == 1, g.output_label0 ^ g.delta[None, :], g.output_label0), ob, bytes(table[index, 8:24])

    cases = [case(0), case(1)]
    res = sharding.evaluate_from(table, cases, circuit, d, n_out, evaluate=stand_in, commitment="blake3", outboard_dir=d)
    assert [r[0] for r in res] == [0, 1] and called == [0, 1]
    with pytest.raises(ValueError):
        sharding.evaluate_from(table, cases, circuit, d, n_out, evaluate=stand_in, outboard_dir=d)

    def refused(*a, **kw):
        del called[:]
        with pytest.raises(sharding.ConsistencyError) as ei:
            sharding.evaluate_from(table, *a, commitment="blake3", outboard_dir=d, **kw)
        return ei.value

    def raising(index, t, f, a, b):
        if index == 1:
            raise gsv.CiphertextMismatch("the ciphertext stream of instance 0 does not match its outboard in group 3", 0, 3, 3 * 2 * 64)
        return stand_in(index, t, f, a, b)

    e = refused(cases, circuit, d, n_out, evaluate=raising)
    assert (e.kind, e.index) == ("CiphertextMismatch", 1) and e.details["group"] == 3 and "group 3" in str(e)
    _flip(os.path.join(d, gsv.outboard_file_name(1)), 24 + 32 + 7)  # a group value of instance 1's outboard
    e = refused(cases, circuit, d, n_out, evaluate=stand_in)
    assert (e.kind, e.index) == ("CiphertextMismatch", 1) and not called  # before anything is evaluated
    _flip(os.path.join(d, gsv.outboard_file_name(1)), 24 + 32 + 7)
    _flip(os.path.join(d, gsv.gc_file_name(0)), gs[0].ciphertexts.size - 1)  # the last chunk of instance 0's file
    e = refused(cases, circuit, d, n_out, evaluate=stand_in)
    assert (e.kind, e.index) == ("CiphertextMismatch", 0) and not called
    # the case in front of the bad one still gets its own check first: a wrong input label of case 1 in front of the bad case 0
    bad_in = dict(cases[1])
    bad_in["input_active"] = bad_in["input_active"].copy()
    bad_in["input_active"][2] ^= gs[1].delta
    e = refused([bad_in, cases[0]], circuit, d, n_out, evaluate=stand_in)
    assert (e.kind, e.index) == ("InputLabelsMismatch", 1)
