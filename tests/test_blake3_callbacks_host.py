"""The host side of the commitments on the callback paths (include/gsv_engine.h "Commitments on the callback paths"), without a device:
gsv_blake3_outboard_size against the header's formula and against what the host writer writes, what it refuses, and the arguments
Session.garble_to_sink / Session.evaluate_from_source refuse before they touch anything of a session."""
import os

import numpy as np
import pytest

LENGTHS = (0, 1, 64, 65, 256, 257, 320, 1665)
KS = (0, 2, 10)


def _formula(n_records, k):
    """24 + 32 (floor((N - 1) / G) + (N - 1) mod G) bytes with N = max(1, ceil(L / 64)) chunks and G = 2^k; the last chunk is what
    lies behind the first N - 1 chunks"""
    N = max(1, -(-n_records // 64))
    return 24 + 32 * (((N - 1) >> k) + ((N - 1) & ((1 << k) - 1))), (n_records - 64 * (N - 1)) * 16


@pytest.mark.parametrize("k", KS)
def test_outboard_size_against_the_formula_and_the_host_writer(tmp_path, k):
    import garbled_snark_verifier_amd as gsv
    for n in LENGTHS:
        data = np.random.default_rng(n).integers(0, 256, n * 16, dtype=np.uint8).tobytes()
        gc, ob = str(tmp_path / ("gc_%d.bin" % n)), str(tmp_path / ("gc_%d.b3o" % n))
        open(gc, "wb").write(data)
        gsv.blake3_file_outboard(gc, k, ob)
        got = gsv.blake3_outboard_size(n, k)
        assert got == _formula(n, k), (n, k)
        assert got[0] == len(open(ob, "rb").read()) == os.path.getsize(ob), (n, k)
        assert 0 <= got[1] <= 1024 and (got[1] == 0) == (n == 0)
        # the outboard and that many last bytes fold to the digest
        assert gsv.blake3_outboard_root(open(ob, "rb").read(), data[len(data) - got[1]:]) == gsv.blake3(data)


def test_outboard_size_refusals():
    import garbled_snark_verifier_amd as gsv
    assert gsv.blake3_outboard_size(1665, 20) == _formula(1665, 20)
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*k in \\[0, 20\\]"):
        gsv.blake3_outboard_size(1665, 21)
    with pytest.raises(gsv.GsvError, match="gsv status 1: .*out of range"):
        gsv.blake3_outboard_size((1 << 58) + 1, 2)
    # either output may be left out
    import ctypes as C
    a = C.c_uint64()
    assert gsv.lib().gsv_blake3_outboard_size(65, 0, C.byref(a), None) == 0 and a.value == 24 + 32
    assert gsv.lib().gsv_blake3_outboard_size(65, 0, None, C.byref(a)) == 0 and a.value == 16
    assert set(("blake3_outboard_size", "SinkCommit")) <= set(gsv.__all__)
    assert gsv.SinkCommit._fields == ("cbcmac", "blake3", "outboards", "last_chunks")


class _NoDevice:
    """Stands where the session's handle is: any use of it is a test failure."""

    def __bool__(self):
        return False  # (Session.close, which runs when the object goes away, then leaves it alone)

    def __getattr__(self, name):
        raise AssertionError("the session's handle was used")

    @property
    def _as_parameter_(self):
        raise AssertionError("the session's handle was handed to the library")


def _bare_session(gsv, n=3):
    s = object.__new__(gsv.Session)  # no engine, no device: the checks under test come before either is needed
    s.n, s.h, s.program, s.replays = n, _NoDevice(), None, 1
    return s


def test_garble_to_sink_refuses_before_anything_touches_a_device():
    import garbled_snark_verifier_amd as gsv
    s = _bare_session(gsv)
    called = []
    handler = lambda *a: called.append(a)  # noqa: E731
    with pytest.raises(ValueError, match="outboards=True needs commitment"):
        s.garble_to_sink(handler, commitment="cbcmac", outboards=True)
    with pytest.raises(ValueError, match="outboards=True needs commitment"):
        s.garble_to_sink(handler, outboards=True)
    with pytest.raises(ValueError, match="commitment must be"):
        s.garble_to_sink(handler, commitment="sha256")
    with pytest.raises(ValueError):
        s.garble_to_sink(None)  # nothing to do: no handler and no commitment
    assert not called


def test_evaluate_from_source_refuses_before_anything_touches_a_device():
    import garbled_snark_verifier_amd as gsv
    s = _bare_session(gsv)
    called = []

    def source(*a):
        called.append(a)

    ob = [b"GSVB3OB\n" + bytes(16)] * 3
    d32, d16 = [bytes(32)] * 3, [bytes(16)] * 3
    with pytest.raises(ValueError, match="need commitment"):
        s.evaluate_from_source(source, outboards=ob, expected=d32)  # the CBC-MAC alone has no outboard
    with pytest.raises(ValueError, match="need commitment"):
        s.evaluate_from_source(source, commitment="cbcmac", last_chunks=[b""] * 3)
    with pytest.raises(ValueError, match="together"):
        s.evaluate_from_source(source, commitment="blake3", outboards=ob)
    with pytest.raises(ValueError, match="together"):
        s.evaluate_from_source(source, commitment="both", expected=d32)
    with pytest.raises(ValueError, match="together"):
        s.evaluate_from_source(source, commitment="blake3", last_chunks=[b""] * 3)
    with pytest.raises(ValueError, match="one per instance"):
        s.evaluate_from_source(source, commitment="blake3", outboards=ob[:2], expected=d32)
    with pytest.raises(ValueError, match="16 or of 32 bytes"):
        s.evaluate_from_source(source, commitment="blake3", outboards=ob, expected=[bytes(20)] * 3)
    with pytest.raises(ValueError, match="16 or of 32 bytes"):
        s.evaluate_from_source(source, commitment="blake3", outboards=ob, expected=d32[:2] + d16[:1])
    with pytest.raises(ValueError, match="last_chunks"):
        s.evaluate_from_source(source, commitment="blake3", outboards=ob, expected=d16, last_chunks=[b""] * 2)
    with pytest.raises(ValueError, match="last_chunks"):
        s.evaluate_from_source(source, commitment="blake3", outboards=ob, expected=d16, last_chunks=[bytes(1025)] * 3)
    with pytest.raises(ValueError):
        s.evaluate_from_source(source, commitment="sha256")
    assert not called
