"""bindings/rust/ and the commitments on the callback paths.  tests/test_rust_shim.py maps every C parameter type to ONE Rust type, which
the two new session calls do not fit — their callbacks may be NULL (`Option<fn>` in Rust, where gsv_session_garble_streaming_sink takes
a plain `GsvCtSinkFn`) and the outboards come as `const uint8_t* const*` — so gpu_ffi.rs declares them in a block of their own behind
wrappers, and this file checks that block the same way: every declaration against include/gsv_engine.h, parameter by parameter; the
wrappers hand every parameter on; the mode files call the wrappers; the callback type has the C typedef's parameters."""
import os
import re

import test_rust_shim as R

NULLABLE = dict(R.C2RUST)
NULLABLE.update({"gsv_ct_sink_fn": "Option<GsvCtSinkFn>", "gsv_outboard_sink_fn": "Option<GsvOutboardSinkFn>", "const uint8_t* const*": "*const *const u8"})
CALLS = {"gsv_session_garble_streaming_sink_commit": "garble_streaming_sink_commit", "gsv_session_evaluate_streaming_source_verified": "evaluate_streaming_source_verified"}


def _ffi():
    return R.strip_comments(open(os.path.join(R.RUST, "src", "gpu_ffi.rs")).read())


def _params(text):
    return [p.strip().split(":", 1) for p in text.split(",") if p.strip()]


def test_callback_commit_declarations_match_the_header():
    c, src = R.c_functions(), _ffi()
    block = src[src.index("mod callback_commit"):]
    found = {m.group(1): _params(m.group(2)) for m in re.finditer(r"pub\(super\) fn (gsv_[a-z_0-9]+)\s*\(([^)]*)\)\s*->\s*c_int", block)}
    assert sorted(found) == sorted(CALLS)
    for name, params in found.items():
        ctypes_ = c[name]
        assert len(ctypes_) == len(params), (name, ctypes_, params)
        for ct, (_, rt) in zip(ctypes_, params):
            assert NULLABLE[ct] == rt.strip(), (name, ct, rt)
    assert R.rust_functions()["gsv_blake3_outboard_size"] == ["u64", "u32", "*mut u64", "*mut u64"]
    assert c["gsv_blake3_outboard_size"] == ["uint64_t", "uint32_t", "uint64_t*", "uint64_t*"]


def test_wrappers_hand_every_parameter_on():
    src = _ffi()
    block = src[src.index("mod callback_commit"):]
    for cname, wrapper in CALLS.items():
        decl = _params(re.search(r"pub\(super\) fn %s\s*\(([^)]*)\)" % cname, block).group(1))
        m = re.search(r"pub unsafe fn %s\s*\(([^)]*)\)\s*->\s*c_int\s*\{\s*callback_commit::%s\(([^)]*)\)\s*\}" % (wrapper, cname), src)
        assert m, wrapper
        assert [(n.strip(), t.strip()) for n, t in _params(m.group(1))] == [(n.strip(), t.strip()) for n, t in decl]
        assert [a.strip() for a in m.group(2).split(",")] == [n.strip() for n, _ in decl]


def test_outboard_callback_type_matches_the_typedef():
    hdr = R.strip_comments(open(os.path.join(R.ROOT, "include", "gsv_engine.h")).read())
    c = re.search(r"typedef int \(\*gsv_outboard_sink_fn\)\(([^)]*)\);", hdr).group(1)
    ctypes_ = [re.sub(r"\s*\*", "*", re.sub(r"\s*\b[A-Za-z_][A-Za-z_0-9]*$", "", p.strip())).strip() for p in c.split(",")]
    r = re.search(r"pub type GsvOutboardSinkFn = unsafe extern \"C\" fn\(([^)]*)\) -> c_int;", _ffi()).group(1)
    assert [R.C2RUST[t] for t in ctypes_] == [t.strip() for _, t in _params(r)]


def test_modes_use_the_wrappers_behind_an_option():
    g = R.strip_comments(open(os.path.join(R.RUST, "src", "gpu_garble_mode.rs")).read())
    e = R.strip_comments(open(os.path.join(R.RUST, "src", "gpu_evaluate_mode.rs")).read())
    assert "garble_streaming_sink_commit(" in g and "pub fn with_blake3_commitment" in g and "if self.commit_blake3" in g
    assert "gsv_session_garble_streaming_sink(" in g  # the default is the call of before
    assert "evaluate_streaming_source_verified(" in e and "pub fn with_verification" in e and "GSV_ERR_MISMATCH" in e and "gsv_session_mismatch_info(" in e
    assert "gsv_session_evaluate_streaming_source(" in e
