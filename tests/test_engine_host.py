"""CPU-side tests of the engine: the C ABI library loads and exports every symbol include/gsv_engine.h
declares, the recorder/compiler keep the reference's gate-id / dead-gate semantics, and the compiled
device schedule (interpreted on the host by tests/hostsim, never by the product) is bit-exact against
the oracle.  No GPU compute here; the GPU parity tests are in test_gpu_parity.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hostsim_lib as h
import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_match_header():
    import garbled_snark_verifier_amd as gsv
    hdr = open(os.path.join(ROOT, "include", "gsv_engine.h")).read()
    declared = set(re.findall(r"\b(gsv_[a-z_0-9]+)\s*\(", hdr))
    L = gsv.lib()
    for sym in sorted(declared):
        assert hasattr(L, sym), "libgsv_engine.so does not export %s" % sym
    assert declared == set(gsv.EXPORTS), declared ^ set(gsv.EXPORTS)


def test_no_cpu_fallback_without_device():
    import torch
    import garbled_snark_verifier_amd as gsv
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    with pytest.raises(gsv.GsvError, match="no CPU fallback"):
        gsv.Engine(0)


def test_recorder_gate_id_and_dead_gate_semantics():
    import garbled_snark_verifier_amd as gsv
    # gate 0: AND live; gate 1: XOR live; gate 2: NAND dead (wire_c UNREACHABLE) -> consumes a gate id, no ciphertext
    p = gsv.Program.from_gates(2, [(0, 2, 3, 4), (8, 4, 2, 5), (1, 5, 3, None), (7, 5, 4, 6)], [6, 5])
    assert p.info["n_gates"] == 4 and p.info["n_dead"] == 1 and p.info["n_ciphertexts"] == 2
    assert p.info["gate_count"][:2] == [1, 1] and p.info["gate_count"][7] == 1 and p.info["gate_count"][8] == 1
    assert p.info["n_inputs"] == 2 and p.info["n_outputs"] == 2
    with pytest.raises(gsv.GsvError):
        gsv.Program.from_gates(1, [(0, 2, 9, 3)], [3])  # reads a wire that was never written
    L = gsv.lib()
    r = C.c_void_p()
    assert L.gsv_recorder_create(C.byref(r)) == 0
    w = C.c_uint64()
    assert L.gsv_recorder_allocate_wire(r, 0, C.byref(w)) == 0 and w.value == 0xFFFFFFFFFFFFFFFF  # storage.rs:119-133
    assert L.gsv_recorder_allocate_wire(r, 3, C.byref(w)) == 0 and w.value == 2                    # WireId::MIN
    L.gsv_recorder_destroy(r)


def test_labels_from_seed_and_cbcmac_match_oracle():
    import garbled_snark_verifier_amd as gsv
    for seed in (0, 1, 2**63 + 5):
        d, f, t, inp = gsv.labels_from_seed(seed, 7)
        ref = o.chacha_labels(seed, 10)
        assert (ref[0] == d).all() and (ref[1] == f).all() and (ref[2] == t).all() and (ref[3:] == inp).all()
    cts = np.random.default_rng(0).integers(0, 256, (1000, 16), dtype=np.uint8)
    assert gsv.cbcmac(cts) == o.cbcmac(cts)
    assert gsv.cbcmac(cts[500:], state=np.frombuffer(gsv.cbcmac(cts[:500]), np.uint8)) == o.cbcmac(cts)
    assert gsv.cbcmac(np.zeros((0, 16), np.uint8)) == bytes(16)


def test_product_host_crypto_matches_oracle():
    K = bytes([0x42] * 16)
    sb = h.sbox()
    assert sb[0] == 0x63 and sb[0x53] == 0xED and len(set(sb.tolist())) == 256  # FIPS-197 fig. 7
    for i in range(64):
        b = os.urandom(16)
        assert h.aes_ttable(b) == o.aes128_encrypt(K, b) == h.aes_portable(b)
        g = int.from_bytes(os.urandom(8), "little")
        assert h.hash_with_gate(b, g) == o.hash_with_gate(b, g)
    assert (h.labels_from_seed(7, 10) == o.chacha_labels(7, 10)).all()


def _hostsim_check(spec, seed, replays=1, oracle_spec=None):
    sp = h.SimProgram(spec, chain_feedback=replays > 1)
    n_in = sp.info["n_inputs"]
    labs = h.labels_from_seed(seed, 3 + n_in)
    delta, consts, inputs = labs[0], labs[1:3], labs[3:]
    out, cts = sp.garble(delta, consts, inputs, replays=replays)
    ref = o.garble(oracle_spec or spec, seed)
    assert ref.n_ciphertexts == cts.shape[0] and (ref.ciphertexts == cts).all() and (ref.output_label0 == out).all()
    assert h.cbcmac(cts) == ref.ct_hash.tobytes()
    assert int(ref.gate_counts.sum()) == sp.info["n_gates"] * replays
    bits = np.random.default_rng(seed).integers(0, 2, n_in).astype(np.uint8)
    act = np.where(bits[:, None] == 1, inputs ^ delta[None, :], inputs)
    oa, ob = sp.evaluate(np.stack([consts[0], consts[1] ^ delta]), act, bits, cts, replays=replays)
    eo, _, _ = o.execute(oracle_spec or spec, bits)
    assert (ob == eo).all() and (oa == np.where(ob[:, None] == 1, out ^ delta[None, :], out)).all()
    return sp


def test_four_wire_and_records(monkeypatch):
    """program.hpp pack_and4 / compile_program 0.: an AND input may be the XOR of up to FOUR wires in the records of a latency-bound
    program (fewer than 600 fused gates per step), so free gates that only feed ANDs stop costing a step of their own — the Fq
    multiplication drops from 1 771 to 987 steps, the random circuits and the driver's component mix keep interpreting to the oracle's
    ciphertexts, labels and bits in either form (forced with GSV_AND_TERMS), with chained replays too; a wide program (an Fq12
    multiplication: 1 100 gates per step) keeps the two-wire records, whose extra label loads it cannot afford."""
    steps = {}
    for terms in ("2", "4", "0"):
        monkeypatch.setenv("GSV_AND_TERMS", terms)
        for spec, seed in (("fq_mul", 1), ("random_circuit:5", 3), ("driver_mix", 2), ("random_circuit:11", 4)):
            steps[(spec, terms)] = _hostsim_check(spec, seed).info["n_steps"]
    assert steps[("fq_mul", "2")] == 1771 and steps[("fq_mul", "4")] == steps[("fq_mul", "0")] == 987
    for spec in ("random_circuit:5", "driver_mix", "random_circuit:11"):
        assert steps[(spec, "4")] <= steps[(spec, "2")]
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_AND_TERMS", "0")
    wide = gsv.Program.from_circuit("fq12_mul").info
    assert wide["n_steps"] == 8197 and wide["and_terms"] == 2 and gsv.Program.from_circuit("fq_mul").info["and_terms"] == 4
    monkeypatch.setenv("GSV_AND_TERMS", "4")
    forced = gsv.Program.from_circuit("fq12_mul").info
    assert forced["n_steps"] == 7164 and forced["and_terms"] == 4


@pytest.mark.parametrize("t", range(11))
def test_compiled_schedule_every_gate_type(t):
    _hostsim_check("gate:%d" % t, 42)


@pytest.mark.parametrize("spec,seed", [("driver_mix", 5), ("u254_add", 0), ("bigint_mul:22", 3), ("fq_add", 1), ("fq_div6", 2), ("fq_mul", 0), ("fq_complex", 99)])
def test_compiled_schedule_matches_oracle(spec, seed):
    sp = _hostsim_check(spec, seed)
    if spec == "fq_mul":
        assert sp.info["n_gates"] == 414284 and sp.info["and_depth"] == 764
        assert sp.info["reads_lds"] > sp.info["reads_hbm"]  # the LDS window takes most operand reads


def test_compiled_chain_replay_matches_streamed_chain():
    # small stand-in for the Fq12 chain: Fq2 mul has 1016 inputs / 508 outputs -> feedback out[i] -> in[i]
    sp = h.SimProgram("fq2_mul", chain_feedback=True)
    assert sp.info["n_gates"] == 1_264_926
    # no oracle circuit chains fq2 muls, so check the replay against two separate oracle garblings glued by hand
    n_in = sp.info["n_inputs"]
    labs = h.labels_from_seed(9, 3 + n_in)
    delta, consts, inputs = labs[0], labs[1:3], labs[3:]
    out2, cts2 = sp.garble(delta, consts, inputs, replays=2)
    sp1 = h.SimProgram("fq2_mul")
    out_a, cts_a = sp1.garble(delta, consts, inputs, replays=1, gid_base=0)
    inputs_b = inputs.copy()
    inputs_b[:508] = out_a
    out_b, cts_b = sp1.garble(delta, consts, inputs_b, replays=1, gid_base=sp.info["n_gates"])
    assert (out2 == out_b).all() and (cts2 == np.concatenate([cts_a, cts_b])).all()


def test_gc_file_format_roundtrip(tmp_path):
    """gc_{i}.bin = bare 16-byte records (ciphertext_repository.rs:94-106); reading re-derives the CBC-MAC."""
    import garbled_snark_verifier_amd as gsv
    g = o.garble("fq_add", 3)
    path = tmp_path / gsv.gc_file_name(7)
    h = gsv.write_gc_file(str(path), g.ciphertexts)
    assert path.name == "gc_7.bin" and path.stat().st_size == 16 * g.n_ciphertexts
    assert h == g.ct_hash.tobytes()
    cts, h2 = gsv.read_gc_file(str(path))
    assert (cts == g.ciphertexts).all() and h2 == h
    # the oracle evaluator (FileSource semantics) accepts the bytes as they are
    bits = np.random.default_rng(0).integers(0, 2, g.n_in).astype(np.uint8)
    act = np.where(bits[:, None] == 1, g.input_label0 ^ g.delta[None, :], g.input_label0)
    e = o.evaluate("fq_add", (g.true_label0 ^ g.delta).tobytes(), g.false_label0.tobytes(), act, bits, cts)
    assert e.ct_hash.tobytes() == h and e.n_consumed == g.n_ciphertexts
    with open(path, "ab") as f:
        f.write(b"\x00" * 5)
    with pytest.raises(gsv.GsvError):
        gsv.read_gc_file(str(path))


@pytest.mark.parametrize("seed", range(8))
def test_compiled_schedule_random_circuits(seed):
    """Differential test on pseudo-random DAGs: ~5000 gates of all ten binary types, ~30 % dead gates, constants,
    repeated operands, ~100 nested component calls with pass-through / constant outputs."""
    sp = _hostsim_check("random_circuit:%d" % seed, seed)
    assert sp.info["n_dead"] > 500 and sp.info["component_calls"] > 50


def test_gate_fusion_shapes_and_unfused_path(monkeypatch):
    """Gate fusion (program.hpp fuse_trace): the reference's ripple-carry adder (gadgets/basic.rs:7-32: half adder + 253 full
    adders = 254 AND + 1013 XOR on 760 dependent levels) must compile to 254 fused ANDs on 254 levels plus the 254 sum bits
    as 3-input XORs; the unfused compilation of the same trace stays available (GSV_FUSE=0) and both interpret to the
    oracle's ciphertexts, labels and bits."""
    sp = _hostsim_check("u254_add", 7)
    assert sp.info["n_ct"] == 254 and sp.info["n_steps"] == 254 and sp.info["n_fused_free"] == 254
    fused = {spec: h.SimProgram(spec).info for spec in ("fq_mul", "driver_mix")}
    monkeypatch.setenv("GSV_FUSE", "0")
    sp0 = _hostsim_check("u254_add", 7)
    assert sp0.info["n_steps"] > 700 and sp0.info["n_fused_free"] == 1013
    for spec, seed in (("fq_mul", 1), ("driver_mix", 2), ("random_circuit:5", 3)):
        sp0 = _hostsim_check(spec, seed)
        if spec in fused:
            assert sp0.info["n_ct"] == fused[spec]["n_ct"] and sp0.info["n_gates"] == fused[spec]["n_gates"]
            assert sp0.info["n_steps"] >= fused[spec]["n_steps"] and sp0.info["n_fused_free"] >= fused[spec]["n_fused_free"]
    # all-HBM compilation (no LDS window): absent operands then name the HBM zero slot
    monkeypatch.setenv("GSV_LDS_SLOTS", "0")
    monkeypatch.delenv("GSV_FUSE")
    _hostsim_check("fq_add", 4)


def test_width_capped_list_schedule_matches_oracle(monkeypatch):
    """compile_program's width-capped list scheduler (CompileOptions::and_cap / xor_cap, GSV_AND_CAP / GSV_XOR_CAP; off by default:
    measured slower on the GPU, profiles/r02_verifier): labels depend on gate ids and dataflow, never on the schedule, so every
    cap must interpret to the oracle's ciphertexts, labels and bits — including the degenerate one gate of each kind per step."""
    asap = {spec: h.SimProgram(spec).info["n_steps"] for spec in ("fq_mul", "random_circuit:5")}
    for cap_and, cap_xor in ((64, 64), (1, 1), (0, 16)):
        monkeypatch.setenv("GSV_AND_CAP", str(cap_and))
        monkeypatch.setenv("GSV_XOR_CAP", str(cap_xor))
        for spec, seed in (("fq_mul", 1), ("random_circuit:5", 3), ("driver_mix", 2)):
            sp = _hostsim_check(spec, seed)
            if spec in asap:
                assert sp.info["n_steps"] >= asap[spec]  # never shorter than the critical path
                if cap_and == 1:
                    assert sp.info["n_steps"] >= max(sp.info["n_ct"], sp.info["n_fused_free"])


@pytest.mark.parametrize("spec,units,seed", [
    ("driver_mix", ["test::mixed_outputs"], 5),           # unit with pass-through / constant / internal outputs, nested child flattened
    ("driver_mix", ["test::inner"], 5),                   # unit nested inside a flattened component; one of its outputs is dead
    ("driver_mix", ["test::inner", "bigint::add"], 6),    # the same component with two output-liveness patterns (add / add_without_carry)
    ("random_circuit:3", ["test::random_block"], 1),      # 145 calls, 72 distinct unit programs, glue in between
    ("random_circuit:8", ["test::random_block"], 2),
    ("fq_complex", ["fp254::montgomery_reduce", "bigint::mul_karatsuba"], 2),  # two units reused (3 programs for 5 calls)
    ("g1_mux_add", ["bigint::multiplexer", "g1::add_montgomery"], 3),  # unit inputs that are the constant wires (MSM tables, constant point)
])
def test_plan_builder_matches_flat_stream(spec, units, seed):
    """plan_builder.hpp: the circuit recorded with some components as CALLS of separately compiled programs must give the
    reference's stream exactly — ciphertexts in gate order across call boundaries, CBC-MAC, output labels, and on evaluation the
    oracle's plaintext bits — including components whose outputs are dead / constants / passed-through inputs in the parent."""
    sp = h.SimPlan(spec, units)
    ref = o.garble(spec, seed)
    n_in = ref.n_in
    labs = h.labels_from_seed(seed, 3 + n_in)
    delta, consts, inputs = labs[0], labs[1:3], labs[3:]
    out, cts = sp.garble(delta, consts, inputs)
    assert sp.info["n_gates"] == int(ref.gate_counts.sum()) and sp.info["n_calls"] >= 3
    assert ref.n_ciphertexts == cts.shape[0] and (ref.ciphertexts == cts).all() and (ref.output_label0 == out).all()
    assert h.cbcmac(cts) == ref.ct_hash.tobytes()
    bits = np.random.default_rng(seed).integers(0, 2, n_in).astype(np.uint8)
    act = np.where(bits[:, None] == 1, inputs ^ delta[None, :], inputs)
    oa, ob = sp.evaluate(np.stack([consts[0], consts[1] ^ delta]), act, bits, cts)
    eo, _, _ = o.execute(spec, bits)
    assert (ob == eo).all() and (oa == np.where(ob[:, None] == 1, out ^ delta[None, :], out)).all()


@pytest.mark.parametrize("spec,units,seed,sched", [
    ("random_circuit:3", ["test::random_block"], 1, dict(max_calls=64)),                       # 145 calls side by side where the data flow allows
    ("random_circuit:8", ["test::random_block"], 2, dict(max_calls=4, window_calls=16)),       # few calls in flight, windows of 16 calls
    ("fq_complex", ["fp254::montgomery_reduce", "bigint::mul_karatsuba"], 2, dict(max_calls=8)),
    ("g1_mux_add", ["bigint::multiplexer", "g1::add_montgomery"], 3, dict(max_calls=16)),      # three independent multiplexers, then the addition
    ("g1_mux_add", ["bigint::multiplexer", "g1::add_montgomery"], 3, dict(max_calls=16, max_slots=1)),  # scratch ring of ONE region: every call waits for its predecessor
    ("driver_mix", ["test::inner", "bigint::add"], 6, dict(max_calls=32, window_ct=300)),      # ciphertext windows
    ("driver_mix", ["test::inner", "bigint::add"], 6, dict(max_calls=3, max_slots=400)),       # a small ring: regions are reused while other calls are in flight
    ("g1_mux_add", ["bigint::multiplexer", "g1::add_montgomery"], 3, dict(max_calls=1, window_calls=1, safe=True)),  # the safe layout: one call per window, no dependency
    ("driver_mix", ["test::inner", "bigint::add"], 6, dict(max_calls=32, retain=False, ring=(3, 9))),  # a ciphertext ring of 9 records under a stream of 12: ct_off = ring_off, the last call wraps
    ("driver_mix", ["test::inner", "bigint::add"], 6, dict(max_calls=32, window_ct=300, retain=False)),  # not retained: ct_off relative to the window's first record
    ("driver_mix", ["test::inner", "bigint::add"], 6, dict(max_calls=32, window_ct=5, retain=False)),    # ... in three windows
])
def test_scheduled_plan_matches_flat_stream(spec, units, seed, sched):
    """schedule.hpp and plan_layout.hpp — the code engine.cpp runs at session creation — over a plan: windows of consecutive calls,
    inside a window a dataflow over the RAW / WAW / WAR hazards on the (recycled) global ids, the in-flight bound and the scratch ring.
    The schedule is verified by brute force (every hazard and every scratch overlap covered by a dependency path) and the host
    interpreter executes the ENGINE'S TABLES for it (call descriptors, hand-over lists with the constants' copies, window-relative
    dependency lists, the three forms of ct_off) as far from the stream order as the dependencies allow (always the ready call with the
    LARGEST index), all calls in one wire file: the stream, its CBC-MAC, the output labels and the evaluation must still be the oracle's."""
    sp = h.SimPlan(spec, units)
    sched = dict(sched)
    ring = sched.pop("ring", None)  # (drain segment records, ring records)
    info = sp.ring(*ring, **sched)[0] if ring else sp.schedule(**sched)
    assert info["critical_steps"] <= info["total_steps"]
    if sched.get("safe"):
        assert info["n_windows"] == sp.info["n_calls"] and info["n_dependencies"] == 0
    ref = o.garble(spec, seed)
    n_in = ref.n_in
    labs = h.labels_from_seed(seed, 3 + n_in)
    delta, consts, inputs = labs[0], labs[1:3], labs[3:]
    out, cts = sp.garble(delta, consts, inputs)
    assert ref.n_ciphertexts == cts.shape[0] and (ref.ciphertexts == cts).all() and (ref.output_label0 == out).all()
    assert h.cbcmac(cts) == ref.ct_hash.tobytes()
    bits = np.random.default_rng(seed).integers(0, 2, n_in).astype(np.uint8)
    act = np.where(bits[:, None] == 1, inputs ^ delta[None, :], inputs)
    oa, ob = sp.evaluate(np.stack([consts[0], consts[1] ^ delta]), act, bits, cts)
    eo, _, _ = o.execute(spec, bits)
    assert (ob == eo).all() and (oa == np.where(ob[:, None] == 1, out ^ delta[None, :], out)).all()


def test_withheld_dependency_deadlocks_the_interpreter():
    """withhold_first_dep (plan_layout.hpp; GSV_FAULT_WITHHOLD_DEP=1 in the engine) points the first dependency of the first call that
    has one at the flag nobody sets: the interpreter, which takes readiness from the engine's dependency lists, finds no ready call.
    The safe layout has no dependency to withhold and runs."""
    sp = h.SimPlan("driver_mix", ["test::inner", "bigint::add"])
    labs = h.labels_from_seed(6, 3 + sp.info["n_inputs"])
    assert sp.schedule(max_calls=32, withhold_first_dep=True)["n_dependencies"] > 0
    with pytest.raises(RuntimeError, match="schedule deadlocks"):
        sp.garble(labs[0], labs[1:3], labs[3:])
    ref_out, ref_cts = (sp.schedule(max_calls=32), sp.garble(labs[0], labs[1:3], labs[3:]))[1]
    sp.schedule(max_calls=1, window_calls=1, safe=True, withhold_first_dep=True)
    out, cts = sp.garble(labs[0], labs[1:3], labs[3:])
    assert (out == ref_out).all() and (cts == ref_cts).all()


def test_schedule_finds_the_independent_calls():
    """Width is found where the circuit has it: the three coordinate multiplexers of g1::multiplexer are independent; one call in
    flight is the stream order itself (depth = all steps); an Fq12 multiplication cut into Fq2-level units is much shallower than
    the sum of its calls."""
    sp = h.SimPlan("g1_mux_add", ["bigint::multiplexer", "g1::add_montgomery"])
    info = sp.schedule(max_calls=16)
    assert info["max_width"] >= 3 and info["critical_steps"] < info["total_steps"]
    seq = sp.schedule(max_calls=1)
    assert seq["max_width"] == 1 and seq["critical_steps"] == seq["total_steps"] and info["critical_steps"] < seq["critical_steps"]
    sp = h.SimPlan("fq12_mul", ["fq2::mul_montgomery"])
    info = sp.schedule(max_calls=64)
    assert info["max_width"] >= 5 and info["critical_steps"] < info["total_steps"] // 2


def test_drain_segments_partition_the_windows():
    """schedule.hpp, SchedParams::segment_ct: a window (one launch, the scope in which calls overlap) is cut into drain segments of
    consecutive calls — the unit in which the stream leaves the device while the window runs.  The segments of a window partition its
    calls in stream order, their ciphertext ranges are contiguous and add up to the window's, none exceeds the limit unless it is a
    single call, and cutting segments changes neither the windows nor the dependencies."""
    sp = h.SimPlan("fq12_mul", ["fq2::mul_montgomery"])
    base = sp.schedule(max_calls=16, window_ct=1_500_000)
    n_ct = sp.info["n_ct"]
    for seg_ct in (0, 50_000, 400_000, 10**9):
        info, segs = sp.segments(seg_ct, max_calls=16, window_ct=1_500_000)
        assert info == base
        assert [s[0] for s in segs] == sorted(s[0] for s in segs) and len({s[0] for s in segs}) == info["n_windows"]
        call, ct = 0, 0
        for w, c0, c1, ct0, n in segs:
            assert c0 == call and c1 > c0 and ct0 == ct
            call, ct = c1, ct + n
            assert seg_ct == 0 or n <= seg_ct or c1 - c0 == 1
        assert ct == n_ct and call == sp.info["n_calls"]
        if seg_ct in (0, 10**9):
            assert len(segs) == info["n_windows"]  # one segment per window
        else:
            assert len(segs) > info["n_windows"]


def test_ciphertext_ring_placement():
    """schedule.hpp, SchedParams::ring_ct: the device keeps a RING of a few segments' ciphertexts instead of a window's, so that one
    launch can span the whole pass.  schedule_calls places every call's block in the ring and says what the call has to wait for;
    verify_schedule simulates the ring record by record (nothing is overwritten before the segment that holds it has left the device,
    no call waits for its own segment, the overwritten calls lie in [ovl0, ovl1)).  Here additionally: blocks of one lap are disjoint and
    ascending, the first lap waits for nothing, later laps do, and a ring smaller than two segments + a call is refused by the check."""
    sp = h.SimPlan("fq12_mul", ["fq2::mul_montgomery"])
    n_ct, n_calls = sp.info["n_ct"], sp.info["n_calls"]
    info, segs, ring = sp.ring(300_000, 1_000_000, max_calls=16)
    assert info["n_windows"] == 1 and len(ring) == n_calls and len(segs) > 4
    offs = [r[0] for r in ring]
    laps = 1 + sum(1 for a, b in zip(offs, offs[1:]) if b < a)
    assert laps >= 3 and n_ct > 3 * 1_000_000
    first_wrap = next(i for i, (a, b) in enumerate(zip(offs, offs[1:])) if b < a) + 1
    assert all(r[1] == 0 for r in ring[:first_wrap]) and any(r[1] > 0 for r in ring[first_wrap:])
    seg_ends = sorted({s[3] + s[4] for s in segs})
    assert all(r[1] in (0, *seg_ends) and r[2] in seg_ends for r in ring)
    with pytest.raises(RuntimeError, match="ring"):
        sp.ring(1_000_000, 700_000, max_calls=16)  # a ring smaller than a segment: some call would wait for its own segment to leave the device


def test_warmup_recorders_give_the_same_plan(monkeypatch):
    """plan_builder.hpp record_plan: a circuit's warm-up mini-circuits (circuits.hpp NamedCircuit::warmups; the verifier's 178 constant
    line functions, here fq12_mix's square and multiplication) are recorded by other threads while the driver walks the circuit, with
    the units compiled on the pool as in the engine.  The plan must be the same with and without them — same calls, same programs —
    and must interpret to the oracle's stream; the half-dead multiplication the warm-ups do not cover is recorded by the driver."""
    import garbled_snark_verifier_amd as gsv
    units = ["fq12::mul_montgomery", "fq12::square_montgomery"]
    infos = []
    for threads in ("0", "2"):
        monkeypatch.setenv("GSV_PLAN_WARMUP_THREADS", threads)
        plan = gsv.Plan.from_circuit("fq12_mix", units, window_div=4)
        infos.append((dict(plan.info), plan.image_bytes(), plan.call_info().tobytes()))
        plan.close()
    assert infos[0] == infos[1] and infos[0][0]["n_calls"] >= 4
    monkeypatch.setenv("HOSTSIM_PLAN_BACKGROUND", "1")
    sp = h.SimPlan("fq12_mix", units)
    ref = o.garble("fq12_mix", 4)
    labs = h.labels_from_seed(4, 3 + ref.n_in)
    out, cts = sp.garble(labs[0], labs[1:3], labs[3:])
    assert (ref.ciphertexts == cts).all() and (ref.output_label0 == out).all() and h.cbcmac(cts) == ref.ct_hash.tobytes()


def test_oracle_prefix_mac_equals_the_stream_before_every_call_boundary():
    """oracle_lib.bench_garble_prefix(circuit, N) stops in front of gate N of the flat stream and returns the CBC-MAC state reached:
    with N = a call's gate offset (Plan.call_info: gid_off, gates, ct_off, n_ct, n_steps) that is the MAC of the ciphertexts of the
    calls before it — what Session.garble_calls returns after a slice that ends there (the GPU form:
    test_gpu_parity.py::test_verifier_lockstep_two_instances_per_workgroup).  Checked on the host interpreter's stream of fq12_mix at
    EVERY call boundary and at the end, and one gate to either side of a boundary whose neighbours are AND-family gates."""
    import garbled_snark_verifier_amd as gsv
    units = ["fq12::mul_montgomery", "fq12::square_montgomery"]
    seed = 4
    plan = gsv.Plan.from_circuit("fq12_mix", units)
    ci = plan.call_info()
    sp = h.SimPlan("fq12_mix", units)
    assert sp.info["n_calls"] == len(ci) >= 4 and sp.info["n_gates"] == plan.info["n_gates"] == int(ci[-1, 0] + ci[-1, 1])
    assert (ci[1:, 0] == ci[:-1, 0] + ci[:-1, 1]).all() and (ci[1:, 2] == ci[:-1, 2] + ci[:-1, 3]).all() and ci[0, 0] == 0 and ci[0, 2] == 0
    labs = h.labels_from_seed(seed, 3 + sp.info["n_inputs"])
    _, cts = sp.garble(labs[0], labs[1:3], labs[3:])
    assert cts.shape[0] == sp.info["n_ct"] == int(ci[-1, 2] + ci[-1, 3])
    for k in range(1, len(ci)):
        _, gates, mac = o.bench_garble_prefix("fq12_mix", int(ci[k, 0]), seed)
        assert gates == int(ci[k, 0]) and mac == h.cbcmac(cts[:int(ci[k, 2])]), "boundary in front of call %d" % k
    _, gates, mac = o.bench_garble_prefix("fq12_mix", sp.info["n_gates"], seed)
    assert gates == sp.info["n_gates"] and mac == h.cbcmac(cts) == o.garble("fq12_mix", seed, capture_ct=False).ct_hash.tobytes()
    assert o.bench_garble_prefix("fq12_mix", 0, seed)[2] == bytes(16)
    # the limit gate itself is NOT garbled: N + 1 adds at most one ciphertext, N - 1 drops at most one
    k = len(ci) // 2
    n, c = int(ci[k, 0]), int(ci[k, 2])
    assert o.bench_garble_prefix("fq12_mix", n + 1, seed)[2] in (h.cbcmac(cts[:c]), h.cbcmac(cts[:c + 1]))
    assert o.bench_garble_prefix("fq12_mix", n - 1, seed)[2] in (h.cbcmac(cts[:c]), h.cbcmac(cts[:c - 1]))
    plan.close()


@pytest.mark.skipif(os.environ.get("GSV_SLOW_TESTS") != "1", reason="slow (two Miller-loop plan builds, ~45 GB of host memory): set GSV_SLOW_TESTS=1")
def test_warmup_recorders_give_the_same_miller_loop_plan(monkeypatch):
    """The case the warm-ups exist for: the Miller loop's 178 constant line functions (circuits.hpp add_ell_warmups) recorded by the
    warm-up recorders while the driver walks the loop.  Same calls, same per-call gates / ciphertexts / steps, same program images as
    the serial build."""
    import hashlib
    import garbled_snark_verifier_amd as gsv
    units = ["fq12::square_montgomery", "fq12::mul_montgomery", "fq12::mul_by_034_montgomery", "pairing::ell_by_constant_montgomery",
             "pairing::double_in_place_circuit_montgomery", "pairing::add_in_place_montgomery", "pairing::mul_by_char_montgomery"]
    seen = []
    for threads in ("0", "2"):
        monkeypatch.setenv("GSV_PLAN_WARMUP_THREADS", threads)
        plan = gsv.Plan.from_circuit("miller_loop", units, window_div=4)
        seen.append((dict(plan.info), plan.image_bytes(), hashlib.sha256(plan.call_info().tobytes()).hexdigest()))
        plan.close()
    assert seen[0] == seen[1] and seen[0][0]["n_gates"] == 6_909_061_143


def test_plan_from_circuit_builds_without_a_device_and_in_both_modes():
    """gsv_plan_from_circuit is host-only work: units are compiled on a worker pool while the driver records (plan_builder.hpp
    CompilePool), with GSV_PLAN_WINDOW_DIV once for half / a quarter of the LDS window.  Every mode gives the reference's counts; the
    plan of the square-root ladder has one program per distinct four-bit chunk of the exponent (fp254::exp_chunk, <= 16 + tail)."""
    import garbled_snark_verifier_amd as gsv
    ref = o.garble("fq12_mix", 1, capture_ct=False)
    for kw in ({}, {"half_window": True}, {"window_div": 4}):
        plan = gsv.Plan.from_circuit("fq12_mix", ["fq12::mul_montgomery", "fq12::square_montgomery"], **kw)
        assert plan.info["n_gates"] == int(ref.gate_counts.sum()) and plan.info["n_ciphertexts"] == ref.n_ciphertexts and plan.info["n_calls"] >= 4
        plan.close()
    assert "GSV_PLAN_HALF_WINDOW" not in os.environ and "GSV_PLAN_WINDOW_DIV" not in os.environ
    with pytest.raises(ValueError):
        gsv.Plan.from_circuit("fq12_mix", ["fq12::mul_montgomery"], window_div=3)
    plan = gsv.Plan.from_circuit("fq_sqrt", ["fp254::exp_chunk"], half_window=True)
    assert plan.info["n_gates"] == 148_727_956 and plan.info["n_ciphertexts"] == 36_651_387 and 60 <= plan.info["n_calls"] <= 70
    plan.close()


FQ12_MIX_UNITS = ["fq12::mul_montgomery", "fq12::square_montgomery"]
_explicit_fq12_mix = {}


def _plan_file_digest(path):
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import plan_digest
    return plan_digest.digest(path)["digest"]


def _fq12_mix_fingerprint(tmp_path, **kw):
    """(info, image bytes, per-call table, digest of the saved plan) of the fq12_mix plan Plan.from_circuit builds with `kw` in the
    environment as it stands.  The first three do not depend on the window share; the saved plan (tools/plan_digest.py) does."""
    import garbled_snark_verifier_amd as gsv
    plan = gsv.Plan.from_circuit("fq12_mix", FQ12_MIX_UNITS, **kw)
    path = os.path.join(str(tmp_path), "fingerprint.gsvplan")
    plan.save(path)
    fp = (dict(plan.info), plan.image_bytes(), plan.call_info().tobytes(), _plan_file_digest(path))
    os.remove(path)
    plan.close()
    return fp


def _explicit_fingerprint(tmp_path, div):
    """... with window_div=div as an argument (it wins over the environment: test_explicit_window_div_wins...); built once per process."""
    if div not in _explicit_fq12_mix:
        _explicit_fq12_mix[div] = _fq12_mix_fingerprint(tmp_path, window_div=div)
    return _explicit_fq12_mix[div]


@pytest.mark.parametrize("div,env", [(4, {"GSV_PLAN_WINDOW_DIV": "4"}), (2, {"GSV_PLAN_HALF_WINDOW": "1"})])
def test_explicit_window_div_equals_the_environment(monkeypatch, tmp_path, div, env):
    """window_div as a parameter (gsv_plan_from_circuit_div) builds the plan that GSV_PLAN_WINDOW_DIV / GSV_PLAN_HALF_WINDOW and no argument build."""
    for k in ("GSV_PLAN_WINDOW_DIV", "GSV_PLAN_HALF_WINDOW"):
        monkeypatch.delenv(k, raising=False)
    explicit = _explicit_fingerprint(tmp_path, div)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _fq12_mix_fingerprint(tmp_path) == explicit
    assert explicit[3] != _explicit_fingerprint(tmp_path, 6 - div)[3]  # (the two shares of the window are different images: the comparison can fail)


def test_explicit_window_div_wins_and_leaves_the_environment_alone(monkeypatch, tmp_path):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.delenv("GSV_PLAN_HALF_WINDOW", raising=False)
    monkeypatch.delenv("GSV_PLAN_WINDOW_DIV", raising=False)
    clean, under = os.path.join(str(tmp_path), "clean.gsvplan"), os.path.join(str(tmp_path), "under.gsvplan")
    gsv.Plan.build_file("fq12_mix", FQ12_MIX_UNITS, clean, window_div=1)
    div4 = _explicit_fingerprint(tmp_path, 4)
    monkeypatch.setenv("GSV_PLAN_WINDOW_DIV", "2")
    assert _fq12_mix_fingerprint(tmp_path, window_div=4) == div4 and div4[3] != _explicit_fingerprint(tmp_path, 2)[3]
    gsv.Plan.build_file("fq12_mix", FQ12_MIX_UNITS, under, window_div=1)  # explicit, 1 included
    assert _plan_file_digest(under) == _plan_file_digest(clean)
    assert os.environ["GSV_PLAN_WINDOW_DIV"] == "2" and "GSV_PLAN_HALF_WINDOW" not in os.environ


class _FrozenEnviron(dict):
    """os.environ's content; any mutation raises."""

    def _refuse(self, *a, **kw):
        raise AssertionError("the package wrote the process environment")

    __setitem__ = __delitem__ = pop = popitem = clear = update = setdefault = __ior__ = _refuse


def test_the_package_does_not_write_the_environment(monkeypatch, tmp_path):
    """Plan.from_circuit / Plan.build_file pass window_div as an argument: bench.py builds plan files on a thread beside running launches,
    and a setenv beside the engine's getenv is a data race."""
    import garbled_snark_verifier_amd as gsv
    gsv.lib()
    frozen = _FrozenEnviron(os.environ)
    with pytest.raises(AssertionError):
        frozen["GSV_PLAN_WINDOW_DIV"] = "4"
    with pytest.raises(AssertionError):
        frozen.pop("GSV_PLAN_HALF_WINDOW", None)
    path = os.path.join(str(tmp_path), "frozen.gsvplan")
    with monkeypatch.context() as m:  # (undone before pytest's own bookkeeping writes PYTEST_CURRENT_TEST)
        m.setattr(os, "environ", frozen)
        for kw in ({"window_div": 4}, {"half_window": True}):
            plan = gsv.Plan.from_circuit("fq12_mix", FQ12_MIX_UNITS, **kw)
            assert plan.info["n_calls"] >= 4
            plan.close()
        gsv.Plan.build_file("fq12_mix", FQ12_MIX_UNITS, path, window_div=4)
        assert os.environ is frozen
    assert os.path.getsize(path) > 0


def test_window_div_entry_points_reject_a_bad_value(tmp_path):
    import ctypes as C
    import garbled_snark_verifier_amd as gsv
    L, h = gsv.lib(), C.c_void_p()
    units = ",".join(FQ12_MIX_UNITS).encode()
    path = os.path.join(str(tmp_path), "bad.gsvplan")
    GSV_ERR_INVALID = 1
    assert L.gsv_plan_from_circuit_div(b"fq12_mix", units, 3, C.byref(h)) == GSV_ERR_INVALID and not h.value
    assert L.gsv_plan_build_file_div(b"fq12_mix", units, os.fsencode(path), 3) == GSV_ERR_INVALID
    assert b"window_div" in L.gsv_last_error() and not os.listdir(str(tmp_path))


def test_step_barrier_isa_check():
    """build.check_step_barrier_isa: the step barrier of run_program_kernel is `s_waitcnt lgkmcnt(0); s_barrier` with the record
    prefetch issued right in front of it — no wait for vector memory: label stores to the HBM wire file are ordered for the
    workgroup by its CU's L1 (kernels.hip).  Verified on the gfx950 ISA of every instantiation at build time; the check passes
    on the built object and trips on doctored listings.  build.check_workgroup_release_model pins the memory-model fact itself
    on the toolchain: hipcc's own `global store; __syncthreads(); global load` waits for no store acknowledgement either."""
    from garbled_snark_verifier_amd import build
    asm = build.disassemble_kernels()
    res = build.check_step_barrier_isa(asm)
    # (garble / evaluate x 1, 2, 4 instances per workgroup + the two Blake3 kernels) x (two-wire only / four-wire capable); the four-wire capable
    # instantiations with several instances per workgroup use the per-GROUP barrier since round 6 (two LDS arrival counters' worth of
    # `ds_add_u32` instead of the two `s_barrier`s, equally free of vector-memory waits: checked by the same function)
    assert len(res) == 16 and sorted(res.values()) == [0] * 4 + [2] * 12
    assert all((v == 0) == ("ELb1EEE" in k and ("ELi2ELi0" in k or "ELi4ELi0" in k)) for k, v in res.items())
    lines = asm.splitlines()
    k = next(i for i, l in enumerate(lines) if "s_waitcnt lgkmcnt(0)" in l and "s_barrier" in lines[i + 1] and "global_load_dwordx4" in lines[i - 1])
    # something scheduled between the prefetch and the barrier
    bad = lines[:k] + ["\tglobal_store_dwordx4 v[4:5], v[0:3], off    // doctored"] + lines[k:]
    with pytest.raises(RuntimeError, match="found 1 step barriers"):
        build.check_step_barrier_isa("\n".join(bad))
    # a wait for vector memory put back in front of a barrier
    bad = lines[:k + 2] + ["\ts_waitcnt vmcnt(0)    // doctored", "\ts_barrier"] + lines[k + 2:]
    with pytest.raises(RuntimeError, match="waits for vector memory"):
        build.check_step_barrier_isa("\n".join(bad))
    probe = build.check_workgroup_release_model()
    st, ba, ld = (next(i for i, t in enumerate(probe) if t.startswith(x)) for x in ("global_store", "s_barrier", "global_load"))
    assert st < ba < ld and not any("vmcnt" in t or t.startswith("buffer_") for t in probe[st:ld])
    # a per-group barrier that waits for the step's stores (what the compiler made of the C++ form: profiles/r06_kernel/) trips the check too
    g = next(i for i, l in enumerate(lines) if "s_mov_b64 exec, 1" in l and "ds_add_u32" in lines[i + 1])
    bad = lines[:g - 1] + ["\ts_waitcnt vmcnt(1)    // doctored"] + lines[g - 1:]
    with pytest.raises(RuntimeError, match="per-group barrier"):
        build.check_step_barrier_isa("\n".join(bad))
    # the correctness precondition itself — the kernels object is NOT built for threadgroup-split mode — is what build() enforces
    # (the instruction-adjacency properties above are performance properties: build() only warns about them)
    assert build.check_not_tgsplit() is True
    # the dataflow epilogue's agent-scope release (buffer_wbl2 ; s_waitcnt vmcnt(0) ; s_barrier) is the one vmcnt wait in front of a barrier
    funcs = build._functions(asm)
    for name, ins in funcs.items():
        if "run_program_kernel" in name:
            assert sum(1 for i, t in enumerate(ins) if t.startswith("buffer_wbl2") and ins[i + 1].startswith("s_waitcnt vmcnt(0)")) >= 1, name


def test_step_loop_of_the_garbling_kernels_holds_no_spill_traffic():
    """tools/spill_audit.py on the compiler's own assembly of kernels.hip (hipcc cross-compiles without a GPU): sixteen instantiations of
    run_program_kernel, no VGPR spill and no scratch instruction anywhere, and in the step loop — the smallest loop that holds both step
    barriers, what a replay executes per step — of the production garbling kernels (two and four instances per workgroup, with and
    without four-wire programs) not one v_readlane / v_writelane: their SGPR spills live in the prologue, the dataflow epilogue and the
    replay loop.  A regression here would put spill traffic on every one of a verifier pass's 8.6 M steps."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_audit
    rows = spill_audit.audit()
    assert len(rows) == 16 and {(r["eval"], r["ni"], r["hash"], r["fw"]) for r in rows} == {(e, n, h, f) for e in (False, True) for f in (False, True) for n, h in ((1, 0), (2, 0), (4, 0), (1, 1))}
    for r in rows:
        assert r["vgpr_spills"] == 0 and r["kernel"]["scratch"] == 0 and r["vgprs"] <= 128, r  # 16 waves per CU need <= 128 VGPRs
        assert r["loop"]["ins"] > 3000, r  # the step loop was found
        if not r["eval"] and r["hash"] == 0 and r["ni"] in (2, 4):
            # nothing is spilled INSIDE the loop (no v_writelane), nothing touches scratch; the instantiations without four-wire programs —
            # every window of the Miller loop and the final exponentiation — re-read nothing, those with them re-read a handful of
            # loop-invariant scalars at the top of a step (round 4: the wave-aligned free-gate lanes of a narrow step cost 6 re-reads, the
            # ciphertext-ring wait in the prologue another 14 — the one-instance-per-workgroup form of the same kernel has 26)
            assert r["loop"]["writelane"] == 0 and r["loop"]["scratch"] == 0, r
            assert r["loop"]["readlane"] <= (24 if r["fw"] else 0), r


@pytest.mark.parametrize("no_vaes", [False, True])
def test_interleaved_cbcmac_equals_single_chains(no_vaes):
    """gsv_cbcmac_update_many / CbcMacHost::update_many (the drain hashes four instances' streams side by side per host thread — sixteen
    where the host has VAES + AVX-512, update_interleaved16_vaes): every chain equals the single-chain CBC-MAC of the oracle, for chain
    counts around both group sizes, with and without a starting state, and across two calls (chaining).  GSV_NO_VAES=1 (read once per
    process, hence the child) pins the AES-NI path on a VAES host."""
    if no_vaes:
        env = dict(os.environ, GSV_NO_VAES="1")
        code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_engine_host as t, garbled_snark_verifier_amd as gsv; "
                "assert gsv.cbcmac_chains_per_step() <= 4; t.test_interleaved_cbcmac_equals_single_chains(False)" % (ROOT, os.path.join(ROOT, "tests")))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return
    import garbled_snark_verifier_amd as gsv
    assert gsv.cbcmac_chains_per_step() in (1, 4, 16)
    rng = np.random.default_rng(4)
    for n_chains in (1, 3, 4, 5, 8, 11, 16, 17, 37):
        for n_rec in (1, 2, 257):
            streams = [rng.integers(0, 256, n_rec * 16, dtype=np.uint8) for _ in range(n_chains)]
            got = gsv.cbcmac_many(streams)
            assert got == [o.cbcmac(s.tobytes()) for s in streams]
            more = [rng.integers(0, 256, 5 * 16, dtype=np.uint8) for _ in range(n_chains)]
            got2 = gsv.cbcmac_many(more, np.stack([np.frombuffer(g, np.uint8) for g in got]))
            assert got2 == [o.cbcmac(np.concatenate([a, b]).tobytes()) for a, b in zip(streams, more)]
