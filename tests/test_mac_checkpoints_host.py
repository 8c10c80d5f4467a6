"""CBC-MAC checkpoints on the host (include/gsv_engine.h "CBC-MAC checkpoints", csrc/engine/mac_checkpoints.hpp): the format and the host
writer against gsv.cbcmac and the CPU oracle's CBC-MAC, the host checker (intact files, flipped records, flipped states, 1 and 4
threads), what is refused, and sharding.run_regarbling(checkpoint_dir=) without an engine.  No GPU."""
import os
import struct

import numpy as np
import pytest

import oracle_lib as o

KS = (0, 2, 6)


def lengths(k):
    G = 1 << k
    return [0, 1, G - 1, G, G + 1, 3 * G, 3 * G + 5]


_streams = {}


def stream(n_records):
    """[n_records, 16] uint8, the same for every test of the session"""
    if n_records not in _streams:
        _streams[n_records] = np.random.default_rng(7000 + n_records).integers(0, 256, (n_records, 16), dtype=np.uint8)
    return _streams[n_records]


def n_states(n, k):
    return -(-n // (1 << k))


def header(k, n, magic=b"GSVMACK\n", version=1):
    return magic + struct.pack("<IIQ", version, k, n)


def write_pair(gsv, tmp_path, cts, k, name="gc"):
    """gc file + checkpoint file of `cts`; returns (path, checkpoint path, CBC-MAC)"""
    path, ck = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".mck"))
    open(path, "wb").write(cts.tobytes())
    return path, ck, gsv.cbcmac_file_checkpoints(path, k, ck)


def flip(path, offset, bit=0x10):
    with open(path, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ bit]))


@pytest.mark.parametrize("k", KS)
def test_writer_states_are_the_chain_states(tmp_path, k):
    """Every state is the CBC-MAC of the records in front of it — by gsv.cbcmac and by the oracle — the last one is the file's MAC, and
    the file is as long as cbcmac_checkpoints_size says."""
    import garbled_snark_verifier_amd as gsv
    assert gsv.checkpoint_file_name(12) == "gc_12.mck"
    G = 1 << k
    for n in lengths(k):
        cts = stream(n)
        path, ck, mac = write_pair(gsv, tmp_path, cts, k)
        got = open(ck, "rb").read()
        assert len(got) == gsv.cbcmac_checkpoints_size(n, k) == 24 + 16 * n_states(n, k), n
        assert got[:24] == header(k, n)
        for g in range(n_states(n, k)):
            end = min((g + 1) * G, n)
            state = got[24 + 16 * g:40 + 16 * g]
            assert state == gsv.cbcmac(cts[:end]) == o.cbcmac(cts[:end]), (n, g)
        assert mac == gsv.read_gc_file(path)[1] == (got[-16:] if n else bytes(16)), n
        assert gsv.cbcmac_file_checkpoints(path, k) == mac  # nowhere to write: the MAC alone


def test_default_group_size_is_the_knob(tmp_path, monkeypatch):
    import garbled_snark_verifier_amd as gsv
    path = str(tmp_path / "gc.bin")
    open(path, "wb").write(stream(37).tobytes())
    monkeypatch.delenv("GSV_MAC_GROUP_LOG2", raising=False)
    assert gsv.cbcmac_checkpoints_size(1 << 20) == 24 + 16 * (1 << 12)  # k = 8
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", "3")
    gsv.cbcmac_file_checkpoints(path, None, str(tmp_path / "gc.mck"))
    assert open(str(tmp_path / "gc.mck"), "rb").read()[:24] == header(3, 37)
    monkeypatch.setenv("GSV_MAC_GROUP_LOG2", "31")
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*GSV_MAC_GROUP_LOG2"):
        gsv.cbcmac_checkpoints_size(100)


@pytest.mark.parametrize("threads", (1, 4))
@pytest.mark.parametrize("k", KS)
def test_host_checker(tmp_path, k, threads):
    """An intact file passes; a flipped bit in record r names group r >> k; a flipped state g names group g when it is the last one
    and else the lower of the two groups it belongs to — g: it is what group g must arrive at, and what group g + 1 starts from."""
    import garbled_snark_verifier_amd as gsv
    G = 1 << k
    for n in lengths(k) + [40 * G + 3]:  # (the last: more groups than one thread advances side by side)
        cts = stream(n)
        path, ck, mac = write_pair(gsv, tmp_path, cts, k)
        assert gsv.cbcmac_file_check(path, ck, threads) == (mac, None), n
        last = n_states(n, k) - 1
        for r in sorted(set(q for q in (0, G - 1, G, n // 2, n - 1) if 0 <= q < n)):
            flip(path, 16 * r + 5)
            assert gsv.cbcmac_file_check(path, ck, threads) == (None, r >> k), (n, r)
            flip(path, 16 * r + 5)
        for g in sorted(set(q for q in (0, last // 2, last - 1, last) if 0 <= q <= last)):
            flip(ck, 24 + 16 * g + 9)
            assert gsv.cbcmac_file_check(path, ck, threads) == (None, g), (n, g)
            flip(ck, 24 + 16 * g + 9)
        assert gsv.cbcmac_file_check(path, ck, threads) == (mac, None), n


def test_malformed_checkpoint_files_are_refused(tmp_path):
    import garbled_snark_verifier_amd as gsv
    k, n = 2, 13
    cts = stream(n)
    path, ck, _ = write_pair(gsv, tmp_path, cts, k)
    good = open(ck, "rb").read()
    bad = str(tmp_path / "bad.mck")

    def refused(content, match):
        open(bad, "wb").write(content)
        with pytest.raises(gsv.GsvError, match="gsv status 1:.*" + match):
            gsv.cbcmac_file_check(path, bad)

    refused(header(k, n, magic=b"GSVB3OB\n") + good[24:], "wrong magic")
    refused(header(k, n, version=2) + good[24:], "version 2")
    refused(header(31, n) + good[24:], "2\\^31")
    refused(good[:-16], "holds %d bytes" % (len(good) - 16))
    refused(good + bytes(16), "holds %d bytes" % (len(good) + 16))
    refused(good[:10], "shorter than its 24-byte header")
    # a well-formed checkpoint file of a stream of another length
    other, other_ck, _ = write_pair(gsv, tmp_path, stream(14), k, "other")
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*14 records.*13"):
        gsv.cbcmac_file_check(path, other_ck)
    # a header whose n_records would make an absurd size is refused by the length check, nothing is allocated for it
    refused(header(0, 1 << 57) + good[24:], "holds %d bytes" % len(good))
    refused(header(0, 1 << 60) + good[24:], "out of range")
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*k in \\[0, 30\\]|gsv status 1:.*GSV_MAC_GROUP_LOG2"):
        gsv.cbcmac_file_checkpoints(path, 31)
    with pytest.raises(gsv.GsvError, match="gsv status 1:.*whole 16-byte records"):
        open(bad, "wb").write(b"x" * 17)
        gsv.cbcmac_file_checkpoints(bad, 2)


def test_run_regarbling_with_checkpoints_on_the_host(tmp_path):
    """sharding.run_regarbling(checkpoint_dir=) without an engine: finalized files go through the host checker, a corrupted one is
    named with its group; a checkpoint file whose last state is not the committed hash is "ciphertext corrupted"; an instance
    without a checkpoint file takes the plain path."""
    import garbled_snark_verifier_amd as gsv
    from garbled_snark_verifier_amd import sharding
    d, k, recs = str(tmp_path), 4, []
    for i, seed in enumerate([5, 6, 7]):
        g = o.garble("u254_add", seed)
        path = os.path.join(d, gsv.gc_file_name(i))
        h = gsv.write_gc_file(path, g.ciphertexts)
        if i < 2:
            assert gsv.cbcmac_file_checkpoints(path, k, os.path.join(d, gsv.checkpoint_file_name(i))) == h
        recs.append(sharding.commit_record(i, h, g.output_label0, g.delta, g.false_label0, g.true_label0, g.input_label0))
    commits = np.stack(recs)
    n = os.path.getsize(os.path.join(d, gsv.gc_file_name(1))) // 16
    assert n > 3 << k
    assert sharding.run_regarbling(commits, [0, 1, 2], {}, "u254_add", d, checkpoint_dir=d) == (True, {})
    with pytest.raises(ValueError):
        sharding.run_regarbling(commits, [0, 1, 2], {}, "u254_add", d, commitment="blake3", checkpoint_dir=d)
    r = (2 << k) + 3
    flip(os.path.join(d, gsv.gc_file_name(1)), 16 * r + 1)
    flip(os.path.join(d, gsv.gc_file_name(2)), 40)
    ok, errors = sharding.run_regarbling(commits, [0, 1, 2], {}, "u254_add", d, checkpoint_dir=d)
    assert not ok and errors == {1: "ciphertext corrupted (group 2)", 2: "ciphertext corrupted"}
    assert sharding.run_regarbling(commits, [0, 1, 2], {}, "u254_add", d)[1] == {1: "ciphertext corrupted", 2: "ciphertext corrupted"}
    flip(os.path.join(d, gsv.gc_file_name(1)), 16 * r + 1)
    # a consistent file / checkpoint pair that is not what was committed to: the checkpoints of ANOTHER stream beside that stream
    open(os.path.join(d, gsv.gc_file_name(0)), "wb").write(open(os.path.join(d, gsv.gc_file_name(1)), "rb").read())
    open(os.path.join(d, gsv.checkpoint_file_name(0)), "wb").write(open(os.path.join(d, gsv.checkpoint_file_name(1)), "rb").read())
    ok, errors = sharding.run_regarbling(commits[:2], [0, 1], {}, "u254_add", d, checkpoint_dir=d)
    assert not ok and errors == {0: "ciphertext corrupted"}
