"""Window launches of run_program_kernel (`ka.calls != nullptr`) and the host code around them, on a small synthetic plan, against a
reference that knows nothing of calls.

What a plan session adds around the kernel's step loop — the per-call descriptor (gate-id and ciphertext offsets, scratch base, record
form), the pre / post hand-over copies between the global wires and a call's scratch region, the completion flags and dependency waits,
the host-visible completion counters the drain follows — otherwise runs only under real circuits of 30 M to 11 G gates with one hasher;
their inputs decide which edges they reach and a failure names no call.  Here a plan of ~3.5 k gates is recorded through gsv.PlanRecorder
from four unit programs (Program.from_gates, compiled once for a quarter of the LDS window so that the SAME images — and record forms — run
at every layout) and glue gates, and the same circuit is garbled and evaluated as ONE flat gate list by tests/gate_list_ref.py
(tests/plan_small_lib.py holds the flattening, written once).

  * CPU half (default non-GPU set): the plan's counts and per-call offsets equal the flat list's, the record forms are the intended ones,
    the reference's own garble -> evaluate round trip holds with a gate-id base whose carry out of 32 bits lands inside the plan, and the
    plan has every property the GPU half relies on (test_plan_has_every_property_the_gpu_half_needs) — a change that voids the coverage
    fails here.
  * GPU half: per instance of a ragged batch of 2 ni + 1 distinct seeds, the whole ciphertext stream, the CBC-MAC, the output label0s, the
    active labels, the plaintext bits and active == select(label0, bit) — with AES and BLAKE3, at 1, 2 and 4 instances per workgroup
    requested, for four session kinds: stream retained with calls one after the other (a) and side by side (b); one window of the stream
    on the device, several windows, garble_streaming into gc files read back by an evaluating session of the same shape (c); one window
    drained in several segments, the path that follows the completion counters (d).  A failure names the call and the flat gate.

BLAKE3 launches one instance per workgroup whatever layout the session was created for (gsvk_launch_batch); a session created for 2 or 4
and then switched to BLAKE3 used to size its flag rows and count its finished workgroups for the layout it no longer ran (fixed with
gsv_session::launch_ni).  The BLAKE3 runs at 2 and 4 requested are the tests of that fix; sess.instances_per_workgroup reports 1 there.

The same file holds two program-session edges the harness reaches cheaply: HBM slots at the top of the 21-bit slot fields in every
operand position of both record forms, and a feedback list whose sources are its destinations.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gate_list_ref as G
import oracle_lib as o
import plan_small_lib as P
import test_kernel_step_shapes as S

BT = S.BLOCK_THREADS
LAYOUTS = [1, 2, 4]
# Session kinds of the GPU half; the two sizes in records are fractions of the plan's stream, checked against the schedule on the device
KINDS = {
    "a": lambda sp: dict(concurrent_calls=1),
    "b": lambda sp: dict(concurrent_calls=8),
    "c": lambda sp: dict(retain_stream=False, window_ct_records=sp.plan.info["n_ciphertexts"] // 4),
    "d": lambda sp: dict(retain_stream=False, drain_segment_records=sp.plan.info["n_ciphertexts"] // 4),
}
SEED0 = 900  # instance i of every batch has seed SEED0 + i: the reference of a seed is computed once per test session

_plan = {}


def small_plan():
    import garbled_snark_verifier_amd as gsv
    if "sp" not in _plan:
        _plan["sp"] = P.build_small_plan(gsv)
    return gsv, _plan["sp"]


# ---- CPU half --------------------------------------------------------------------------------------------------------------------------------
def test_plan_counts_and_call_offsets_are_the_flat_lists():
    gsv, sp = small_plan()
    n_ct = int(sp.is_ct.sum())
    assert sp.plan.info["n_gates"] == len(sp.flat) < 50_000 and sp.plan.info["n_ciphertexts"] == n_ct and sp.plan.info["n_calls"] == len(sp.calls)
    assert sp.plan.info["n_inputs"] == len(sp.inputs) and sp.plan.info["n_outputs"] == len(sp.outputs)
    info = sp.plan.call_info()
    for k, c in enumerate(sp.calls):
        want = [c.g0, c.g1 - c.g0, sp.ct_before[c.g0], sp.ct_before[c.g1] - sp.ct_before[c.g0]]
        assert [int(v) for v in info[k][:4]] == [int(v) for v in want], "call %d (%s): [gate offset, gates, ciphertext offset, ciphertexts]" % (k, c.name)
        if c.unit:
            assert int(info[k][4]) == c.unit.prog.info["n_steps"] == len(c.unit.shapes)


def test_record_forms_are_as_intended():
    gsv, sp = small_plan()
    forms = sp.plan.call_record_forms()
    for k, c in enumerate(sp.calls):
        if c.unit:
            assert forms[k] == c.unit.terms == c.unit.prog.info["and_terms"], "call %d (%s)" % (k, c.name)
        else:
            assert forms[k] in (2, 4)
    assert [c.name for c in sp.calls] == ["two", "four", "glue", "two", "four", "long", "glue", "two", "free", "four", "long", "glue"]
    assert [f for f, c in zip(forms, sp.calls) if c.unit] == [2, 4, 2, 4, 2, 2, 2, 4, 2]


def test_flat_reference_round_trip_with_a_carry_inside_the_plan():
    gsv, sp = small_plan()
    base = S.gate_id_bases(len(sp.flat))[0]
    assert base < 2**32 < base + len(sp.flat)
    carry_gate = 2**32 - base
    assert 0 < sp.call_of_gate(carry_gate) < len(sp.calls) - 1  # not in the first call: gid_base + gid_off carries, not the record's own id
    for hasher in ("aes", "blake3"):
        g, e = P.reference(gsv, sp, SEED0, base, hasher)
        d = P.labels(gsv, sp, SEED0)[0]
        assert g.n_ciphertexts == e.n_consumed == sp.plan.info["n_ciphertexts"] and g.n_dead == sum(1 for q in sp.flat if q[3] is None)
        assert (e.output_active == np.where(e.output_bits[:, None] == 1, g.output_label0 ^ d[None, :], g.output_label0)).all()
        assert g.ct_hash == e.ct_hash
    assert (P.reference(gsv, sp, SEED0, base, "aes")[0].ciphertexts != P.reference(gsv, sp, SEED0, 0, "aes")[0].ciphertexts).any()


def test_plan_has_every_property_the_gpu_half_needs():
    gsv, sp = small_plan()
    forms = sp.plan.call_record_forms()
    calls, dep, prod = sp.calls, sp.depends(), sp.producers()
    units = [k for k, c in enumerate(calls) if c.unit]
    glue = [k for k, c in enumerate(calls) if not c.unit]
    # both record forms (the session kinds a, b and d run the whole plan as one window: asserted on the device)
    assert {2, 4} <= set(forms[k] for k in units)
    # one unit called three or more times with different inputs
    for name in ("two", "four"):
        ins = [tuple(calls[k].in_wires) for k in units if calls[k].name == name]
        assert len(ins) >= 3 and len(set(ins)) == len(ins)
    # two call chains of two calls each that do not depend on each other
    chains = [(i, j) for i in units for j in units if i in dep[j]]
    assert any({a, b}.isdisjoint({c, d}) and all(x not in dep[y] and y not in dep[x] for x in (a, b) for y in (c, d)) for a, b in chains for c, d in chains)
    # a call that reads an earlier call's output; one that reads a glue wire; one with constant inputs
    assert any(prod.get(w) in units for k in units for w in calls[k].in_wires)
    assert any(prod.get(w) in glue for k in units for w in calls[k].in_wires)
    assert any(0 in calls[k].in_wires and 1 in calls[k].in_wires for k in units)
    # a call with outputs that nobody reads, beside outputs that are read
    read = set(sp.outputs)
    for c in calls:
        read |= set(c.in_wires)
    assert any(0 < len([w for w in calls[k].out_wires if w not in read]) < len(calls[k].out_wires) for k in units)
    # plan outputs: an input wire, a constant
    assert any(w in sp.inputs for w in sp.outputs) and any(w in (0, 1) for w in sp.outputs)
    # hand-over lists longer than the workgroup: more than one trip of the pre and post copy loops at EVERY layout, and the wires past the
    # first trip matter — inputs past BT are read by the unit's gates, outputs past BT by later calls and as plan outputs
    longs = [k for k in units if calls[k].unit.n_inputs > BT and calls[k].unit.n_outputs > BT]
    assert longs and len(longs) >= 2
    for k in longs:
        u = calls[k].unit
        used = set()
        for t, a, b, c in u.gates:
            used |= {a, b}
        assert all(2 + i in used for i in range(BT, u.n_inputs))
        tail = calls[k].out_wires[BT:]
        assert any(w in sp.outputs for w in tail) and (k == longs[-1] or any(w in calls[j].in_wires for j in units for w in tail))
    # ... and a pre-copy of more than BT wires that ANOTHER CALL wrote (not plan inputs staged by the host)
    assert any(len([w for w in calls[k].in_wires if prod.get(w) in units]) > BT for k in longs)
    # a unit with dead gates, a glue run with one, a unit that is all free gates (an empty ciphertext block in the middle of the stream)
    assert any(calls[k].unit.n_dead for k in units) and any(q[3] is None for k in glue for q in sp.flat[calls[k].g0:calls[k].g1])
    free = [k for k in units if calls[k].unit.n_ct == 0]
    assert free and all(calls[k].unit.prog.info["n_ciphertexts"] == 0 and 0 < sp.ct_before[calls[k].g0] < sp.ct_before[-1] for k in free)
    # the sizes the session kinds c and d derive: at least three windows / segments can exist (no call is larger than the unit of size)
    assert max(int(r[3]) for r in sp.plan.call_info()) <= sp.plan.info["n_ciphertexts"] // 4


# ---- GPU half --------------------------------------------------------------------------------------------------------------------------------
_hip = []


def _hip_runtime():
    """The HIP runtime the engine library itself is linked to, looked up through the engine library's own handle (a symbol lookup on a
    library's handle searches the libraries it depends on).  Which file that is depends on the process: torch ships a runtime of its own,
    and when torch was imported first the engine resolves to that one, otherwise to the system's — a block from another runtime's
    allocator would sit nowhere near the session's, and a second runtime finds no device once the first has the GPU open."""
    if not _hip:
        import garbled_snark_verifier_amd as gsv
        L = C.CDLL(gsv.lib()._name)  # the same loaded library, a handle of our own to put argtypes on
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipFree.argtypes = [C.c_void_p]
        _hip.append(L)
    return _hip[0]


class _Tripwire:
    """256 KiB of device memory filled with a pattern, allocated right after a session, checked after its run.  A TRIPWIRE, not a proof:
    it notices a write past one of the session's allocations (the completion flag rows are among the last) only if the allocator happens
    to place this block directly behind it."""
    BYTES = 256 * 1024

    def __init__(self):
        L = _hip_runtime()
        self.p = C.c_void_p()
        assert L.hipMalloc(C.byref(self.p), self.BYTES) == 0 and L.hipMemset(self.p, 0xA5, self.BYTES) == 0 and L.hipDeviceSynchronize() == 0

    def check(self, what):
        L = _hip_runtime()
        host = np.zeros(self.BYTES, np.uint8)
        assert L.hipDeviceSynchronize() == 0 and L.hipMemcpy(host.ctypes.data, self.p, self.BYTES, 2) == 0  # 2 = hipMemcpyDeviceToHost
        assert L.hipFree(self.p) == 0
        assert (host == 0xA5).all(), what + ": device memory next to the session's allocations was overwritten"


def _compare(gsv, sp, what, seeds, base, hasher, cts, macs, out0, act_out, bit_out):
    for i, seed in enumerate(seeds):
        g, e = P.reference(gsv, sp, seed, base, hasher)
        d = P.labels(gsv, sp, seed)[0]
        w = "%s, instance %d of %d (seed %d)" % (what, i, len(seeds), seed)
        assert cts[i].shape == g.ciphertexts.shape, w
        bad = np.nonzero((cts[i] != g.ciphertexts).any(axis=1))[0]
        assert bad.size == 0, "%s: %d ciphertexts differ, the first at stream index %d: %s" % (w, bad.size, bad[0], sp.where_ct(int(bad[0])))
        assert macs[i] == g.ct_hash, w + ": CBC-MAC"
        bad = np.nonzero((out0[i] != g.output_label0).any(axis=1))[0]
        assert bad.size == 0, "%s: %d output label0s differ, the first: plan output %d = %s" % (w, bad.size, bad[0], sp.where_wire(sp.outputs[bad[0]]))
        bad = np.nonzero(bit_out[i] != e.output_bits)[0]
        assert bad.size == 0, "%s: %d plaintext bits differ, the first: plan output %d = %s" % (w, bad.size, bad[0], sp.where_wire(sp.outputs[bad[0]]))
        bad = np.nonzero((act_out[i] != e.output_active).any(axis=1))[0]
        assert bad.size == 0, "%s: %d active labels differ, the first: plan output %d = %s" % (w, bad.size, bad[0], sp.where_wire(sp.outputs[bad[0]]))
        assert (act_out[i] == np.where(bit_out[i][:, None] == 1, out0[i] ^ d[None, :], out0[i])).all(), w + ": active label != select(label0, bit)"


def _run_plan(engine, monkeypatch, tmp_path, ni, hasher, kind, base=0):
    gsv, sp = small_plan()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    monkeypatch.delenv("GSV_AND_TERMS", raising=False)
    seeds = [SEED0 + i for i in range(2 * ni + 1)]
    B = len(seeds)
    labs = [P.labels(gsv, sp, s) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([x[1] for x in labs]); inputs = np.stack([x[2] for x in labs]); bits = np.stack([x[3] for x in labs])
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    opts = KINDS[kind](sp)
    what = "%s, %d per workgroup requested, session kind %s %r, gate_id_base %d" % (hasher, ni, kind, opts, base)

    def session():
        s = gsv.Session(engine, sp.plan, B, **opts)
        wire = _Tripwire()
        assert s.instances_per_workgroup == ni, "the plan's images must serve this layout"
        s.set_hasher(hasher)
        assert s.instances_per_workgroup == (1 if hasher == "blake3" else ni)  # BLAKE3 launches one instance per workgroup
        info = s.schedule_info()
        assert info["n_calls"] == len(sp.calls)
        if kind == "a":
            assert info["max_width"] == 1 and info["n_windows"] == 1
        elif kind == "b":
            assert info["max_width"] >= 2 and info["n_windows"] == 1
        elif kind == "c":
            assert info["n_windows"] >= 3
        else:
            assert info["max_width"] >= 2 and info["n_windows"] == 1 and info["n_segments"] >= 3
        return s, wire

    sess, wire = session()
    sess.set_garble_inputs(delta, consts, inputs)
    if kind in "ab":
        sess.garble(base)
        sess.sync()
        cts = [sess.read_ciphertexts(i) for i in range(B)]
        macs = [sess.ciphertext_hash(i) for i in range(B)]
    else:
        macs = sess.garble_streaming(base, directory=str(tmp_path))
        cts = [gsv.read_gc_file(os.path.join(str(tmp_path), gsv.gc_file_name(i)))[0] for i in range(B)]
    out0 = sess.read_outputs()
    assert sess.fallback_count() == 0
    sess.close()
    wire.check(what + " (garbling)")
    ev, wire = session()
    ev.set_evaluate_inputs(consts_active, active, bits)
    if kind in "ab":
        for i in range(B):
            ev.upload_ciphertexts(i, cts[i])
        ev.evaluate(base)
        ev.sync()
    else:
        assert ev.evaluate_streaming(str(tmp_path), 0, base) == macs, what + ": the evaluator's CBC-MACs of the files it read"
    act_out, bit_out = ev.read_outputs(with_bits=True)
    assert ev.fallback_count() == 0
    ev.close()
    wire.check(what + " (evaluating)")
    _compare(gsv, sp, what, seeds, base, hasher, cts, macs, out0, act_out, bit_out)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("ni", LAYOUTS)
@pytest.mark.parametrize("hasher", ["aes", "blake3"])
def test_small_plan_on_the_device(engine, monkeypatch, tmp_path, hasher, ni, kind):
    """Every session kind at every layout with both hashers, a ragged batch of 2 ni + 1 instances.  With BLAKE3 at 2 and 4 requested the
    launches have one workgroup per instance while the session was laid out for fewer: the completion flag rows and the drain's count of
    finished workgroups must follow the launch (kind d waits on those counts).  Every run carries the _Tripwire block."""
    _run_plan(engine, monkeypatch, tmp_path, ni, hasher, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("hasher,which", [("aes", 0), ("blake3", 2)])
def test_small_plan_with_gate_id_bases(engine, monkeypatch, tmp_path, hasher, which):
    """gid_base + gid_off in 64 bits: the carry out of the low word inside the plan (not in its first call), and a base far past 2^48."""
    gsv, sp = small_plan()
    base = S.gate_id_bases(len(sp.flat))[which]
    assert base < 2**32 < base + len(sp.flat) if which == 0 else base > 2**48
    _run_plan(engine, monkeypatch, tmp_path, 4, hasher, "b", base=base)


# ---- program sessions: the top of the slot encoding ------------------------------------------------------------------------------------
# Slots are 21-bit fields at bit offsets 0, 21 and 42 of a record's words (program.hpp, XorRec / pack_and / pack_and4); bit 20 marks the
# LDS window, so an HBM slot has 20 bits and the wire file ends at 2^20 - 1.  A program with 2^20 - 64 inputs puts its last inputs, and
# everything it computes, just below that end: the operands of every gate here are among the last 400 inputs (slots above 2^20 - 470,
# bits 19 .. 5 all set), each input used once, and fusion folds the free gates in front of an AND into its record, so that EVERY operand field
# of every record — a1 a2 b1 b2 p of the two-wire form, a1 .. a4 b1 .. b4 p of the four-wire form, x1 .. x4 of a free record — and every
# output field holds such a slot.
TOP_INPUTS = 2**20 - 64
TOP_OPERANDS = 400
TOP_ANDS, TOP_FREE = 36, 4


def build_top(terms, n_and=TOP_ANDS):
    """n_and gates AND_t(a1 ^ .. , b1 ^ ..) ^ p and TOP_FREE gates x1 ^ x2 ^ x3 ^ x4 (the second of them an Xnor) over the last inputs."""
    it = iter(range(2 + TOP_INPUTS - 1, 1, -1))
    gates, outputs, nxt = [], [], [2 + TOP_INPUTS]

    def emit(t, a, b):
        gates.append((t, a, b, nxt[0]))
        nxt[0] += 1
        return nxt[0] - 1

    def side():
        if terms == 4:
            return emit(G.XOR, emit(G.XOR, next(it), next(it)), emit(G.XOR, next(it), next(it)))
        return emit(G.XOR, next(it), next(it))

    for k in range(n_and):
        a = side()
        w = emit(k % 8, a, side())
        outputs.append(emit(G.XOR, w, next(it)))
    for k in range(TOP_FREE):
        outputs.append(emit(G.XNOR if k & 1 else G.XOR, emit(G.XOR, next(it), next(it)), emit(G.XOR, next(it), next(it))))
    used = sorted(set(w for g in gates for w in g[1:3] if w < 2 + TOP_INPUTS))
    return gates, outputs, used


_top = {}


def top_program(terms):
    """(gates, outputs, the input wires the gates read, Program — ONE image for a quarter of the LDS window: it serves layouts 1 and 4)."""
    import garbled_snark_verifier_amd as gsv
    if terms not in _top:
        gates, outputs, used = build_top(terms)
        with S.and_terms_env(terms):
            prog = gsv.Program.from_gates(TOP_INPUTS, gates, outputs, window_div=4)
        _top[terms] = (gates, outputs, used, prog)
    return _top[terms]


@pytest.mark.parametrize("terms", [2, 4])
def test_top_slots_fill_every_operand_field(terms):
    gates, outputs, used, prog = top_program(terms)
    info = prog.info
    per_and = 5 if terms == 2 else 9
    assert info["and_terms"] == terms and info["n_inputs"] == TOP_INPUTS and info["n_ciphertexts"] == TOP_ANDS and info["n_fused_free"] == TOP_FREE
    assert len(used) == TOP_ANDS * per_and + TOP_FREE * 4 <= TOP_OPERANDS and min(used) >= 2 + TOP_INPUTS - TOP_OPERANDS  # every operand a different one of the last inputs
    assert 3 + (min(used) - 2) >= 2**20 - 470 >= 2**19  # (input i sits in slot 3 + i)
    # one step; every operand field of every record names an HBM slot (an absent operand, or one in the LDS window, is not counted), and
    # every output is written to HBM — behind the inputs, so above them
    assert [[int(v) for v in row] for row in prog.step_stats()] == [[TOP_ANDS, TOP_FREE, 0, TOP_ANDS * per_and + TOP_FREE * 4, 0, TOP_ANDS + TOP_FREE]]
    assert info["reads_lds"] == info["writes_lds"] == 0 and 3 + TOP_INPUTS + len(outputs) <= info["n_slots"] <= 2**20 - 1


def test_one_slot_too_many_fails_cleanly():
    """60 + 4 outputs behind 2^20 - 64 inputs and the three constant slots: the wire file would need 2^20 + 3 slots."""
    import garbled_snark_verifier_amd as gsv
    gates, outputs, _ = build_top(2, n_and=60)
    assert 3 + TOP_INPUTS + len(outputs) > 2**20 - 1
    with pytest.raises(gsv.GsvError, match=re.escape("more than 2^20 HBM wire slots")):
        gsv.Program.from_gates(TOP_INPUTS, gates, outputs, window_div=4)


_top_labels = {}


def _top_instance(gsv, seed):
    if seed not in _top_labels:
        d, f, t, inp = gsv.labels_from_seed(seed, TOP_INPUTS)
        _top_labels[seed] = (d, np.stack([f, t]), inp, np.random.default_rng(seed).integers(0, 2, TOP_INPUTS).astype(np.uint8))
    return _top_labels[seed]


@pytest.mark.gpu
@pytest.mark.parametrize("hasher,ni", [("aes", 1), ("aes", 4), ("blake3", 1)])
@pytest.mark.parametrize("terms", [2, 4])
def test_top_slots_on_the_device(engine, monkeypatch, terms, hasher, ni):
    """Three instances at one per workgroup, five at four (a session never puts more instances into a workgroup than it holds: a full
    workgroup and one with three idle groups); wire files of 16 MB each; garble and evaluate."""
    import garbled_snark_verifier_amd as gsv
    gates, outputs, used, prog = top_program(terms)
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    seeds = [61, 62, 63, 64, 65][:3 if ni == 1 else 5]
    labs = [_top_instance(gsv, s) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([x[1] for x in labs]); inputs = np.stack([x[2] for x in labs]); bits = np.stack([x[3] for x in labs])
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    sess = gsv.Session(engine, prog, len(seeds))
    assert sess.instances_per_workgroup == ni
    sess.set_hasher(hasher)
    sess.set_garble_inputs(delta, consts, inputs)
    sess.garble(0)
    sess.sync()
    out0 = sess.read_outputs()
    cts = [sess.read_ciphertexts(i) for i in range(len(seeds))]
    macs = [sess.ciphertext_hash(i) for i in range(len(seeds))]
    sess.close()
    ev = gsv.Session(engine, prog, len(seeds))
    ev.set_hasher(hasher)
    ev.set_evaluate_inputs(consts_active, active, bits)
    for i in range(len(seeds)):
        ev.upload_ciphertexts(i, cts[i])
    ev.evaluate(0)
    ev.sync()
    act_out, bit_out = ev.read_outputs(with_bits=True)
    ev.close()
    idx = np.array(used) - 2
    o.set_hasher(hasher)
    try:
        for i in range(len(seeds)):
            what = "instance %d, %d per workgroup, %d-wire records, %s" % (i, ni, terms, hasher)
            g = G.garble(gates, delta[i], consts[i], inputs[i][idx], outputs, input_wires=used)
            e = G.evaluate(gates, consts_active[i], active[i][idx], bits[i][idx], g.ciphertexts, outputs, input_wires=used)
            bad = np.nonzero((cts[i] != g.ciphertexts).any(axis=1))[0]
            assert bad.size == 0, "%s: %d ciphertexts differ, the first is gate %d's (AND gate k reads the %d inputs below wire %d)" % (what, bad.size, bad[0], 5 if terms == 2 else 9, 2 + TOP_INPUTS)
            assert macs[i] == g.ct_hash, what
            bad = np.nonzero((out0[i] != g.output_label0).any(axis=1))[0]
            assert bad.size == 0, "%s: %d output label0s differ, the first: output %d" % (what, bad.size, bad[0])
            assert (bit_out[i] == e.output_bits).all(), what + ": plaintext bits differ"
            bad = np.nonzero((act_out[i] != e.output_active).any(axis=1))[0]
            assert bad.size == 0, "%s: %d active labels differ, the first: output %d" % (what, bad.size, bad[0])
            assert (act_out[i] == np.where(bit_out[i][:, None] == 1, out0[i] ^ delta[i][None, :], out0[i])).all(), what
    finally:
        o.set_hasher("aes")


# ---- program sessions: feedback whose sources are its destinations -----------------------------------------------------------------------
# The replay epilogue copies W[fb_dst[i]] <- W[fb_src[i]] through staging slots, in trips of the instance's thread group, "because sources
# may alias destinations" (kernels.hip) — and every other test feeds output i to input i, with disjoint slots.  Here the outputs ARE the
# input wires (output j = input j) followed by four computed wires, and the feedback list permutes them: inputs 0 and 1 swap, inputs
# 2 .. N - 5 rotate by one, the computed outputs go to the last four inputs — more pairs than the workgroup has threads, so that a copy
# without the stage reads, in its second trip, what its first trip has already overwritten.
FB_INPUTS = BT + 40
FB_COMPUTED = 4
FB_REPLAYS = 3
_fb = {}


def feedback_program():
    import garbled_snark_verifier_amd as gsv
    if "p" not in _fb:
        N = FB_INPUTS
        gates, outs, _ = S.build_layered([(30, 20), (12, 9), (25, 6)], n_inputs=N)  # (reads the first inputs only)
        nxt = max(g[3] for g in gates if g[3] is not None) + 1
        computed = []
        for k in range(FB_COMPUTED):  # ... and gates over inputs from the far end of the rotation, past the first trip of the copy loops
            gates.append((G.XOR, 2 + BT + k, 2 + N - 5 - k, nxt))
            gates.append((k, nxt, outs[k], nxt + 1))
            computed.append(nxt + 1)
            nxt += 2
        pairs = [(0, 1), (1, 0)] + [(j, j + 1) for j in range(2, N - 5)] + [(N - 5, 2)] + [(N + k, N - 4 + k) for k in range(FB_COMPUTED)]
        prog = gsv.Program.from_gates(N, gates, list(range(2, 2 + N)) + computed, feedback=pairs)
        _fb["p"] = (gates, computed, pairs, prog)
    return _fb["p"]


def test_feedback_list_is_a_permutation_of_the_inputs():
    gates, computed, pairs, prog = feedback_program()
    N = FB_INPUTS
    assert prog.info["n_inputs"] == N and prog.info["n_outputs"] == N + FB_COMPUTED and len(pairs) == N > BT
    src, dst = [a for a, _ in pairs], [b for _, b in pairs]
    assert sorted(dst) == list(range(N)) and sorted(src) == list(range(N - 4)) + list(range(N, N + 4))
    assert (0, 1) in pairs and (1, 0) in pairs and all(a != b for a, b in pairs)                       # a swap; no pair copies a slot onto itself
    assert sum(1 for a, b in pairs if a < N and b == a + 1) >= BT and set(src[:N - 4]) <= set(dst)      # a rotation longer than one trip; sources are destinations
    used = set(w for g in gates for w in g[1:3])
    assert {2, 3, 2 + BT, 2 + N - 5} <= used  # the gates read swapped, rotated and overwritten inputs: the permutation changes every replay's stream


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 4])
def test_feedback_onto_its_own_sources_on_the_device(engine, monkeypatch, ni):
    """replays = 3 on the device == the reference run three times with the inputs re-wired by hand (gate ids continue across replays, a
    non-zero base); the outputs read afterwards are the input slots AFTER the last epilogue and the last replay's computed wires.  The
    plaintext bits go through the same staging."""
    import garbled_snark_verifier_amd as gsv
    gates, computed, pairs, prog = feedback_program()
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    N, base = FB_INPUTS, 2**32 - len(gates) - len(gates) // 2
    seeds = [80 + k for k in range(2 * ni + 1)]
    B = len(seeds)
    labs = [gsv.labels_from_seed(s, N) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([np.stack([x[1], x[2]]) for x in labs]); inputs = np.stack([x[3] for x in labs])
    bits = np.random.default_rng(8).integers(0, 2, (B, N)).astype(np.uint8)
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    sess = gsv.Session(engine, prog, B, FB_REPLAYS)
    assert sess.instances_per_workgroup == ni
    sess.set_garble_inputs(delta, consts, inputs)
    sess.garble(base)
    sess.sync()
    out0 = sess.read_outputs()
    cts = [sess.read_ciphertexts(i) for i in range(B)]
    macs = [sess.ciphertext_hash(i) for i in range(B)]
    sess.close()
    ev = gsv.Session(engine, prog, B, FB_REPLAYS)
    ev.set_evaluate_inputs(consts_active, active, bits)
    for i in range(B):
        ev.upload_ciphertexts(i, cts[i])
    ev.evaluate(base)
    ev.sync()
    act_out, bit_out = ev.read_outputs(with_bits=True)
    ev.close()
    n_ct = prog.info["n_ciphertexts"]
    for i in range(B):
        what = "instance %d of %d, %d per workgroup" % (i, B, ni)
        lab0, act, bit = inputs[i].copy(), active[i].copy(), bits[i].copy()
        stream = []
        for r in range(FB_REPLAYS):
            g = G.garble(gates, delta[i], consts[i], lab0, computed, gate_id_base=base + r * len(gates))
            e = G.evaluate(gates, consts_active[i], act, bit, g.ciphertexts, computed, gate_id_base=base + r * len(gates))
            stream.append(g.ciphertexts)
            out_l, out_a, out_b = np.concatenate([lab0, g.output_label0]), np.concatenate([act, e.output_active]), np.concatenate([bit, e.output_bits])
            lab0, act, bit = lab0.copy(), act.copy(), bit.copy()
            for a, b in pairs:  # the epilogue, on copies: every source is read before any destination is written
                lab0[b], act[b], bit[b] = out_l[a], out_a[a], out_b[a]
            bad = np.nonzero((cts[i][r * n_ct:(r + 1) * n_ct] != g.ciphertexts).any(axis=1))[0]
            assert bad.size == 0, "%s: replay %d: %d ciphertexts differ, the first at index %d of the replay (replay 0 is plain; later ones read what the feedback epilogue wrote)" % (what, r, bad.size, bad[0])
        assert macs[i] == o.cbcmac(np.concatenate(stream)), what
        want_l, want_a, want_b = np.concatenate([lab0, g.output_label0]), np.concatenate([act, e.output_active]), np.concatenate([bit, e.output_bits])
        bad = np.nonzero((out0[i] != want_l).any(axis=1))[0]
        assert bad.size == 0, "%s: %d output label0s differ after the last epilogue, the first: output %d (outputs below %d are the input slots)" % (what, bad.size, bad[0], N)
        assert (bit_out[i] == want_b).all(), what + ": plaintext bits differ after the last epilogue"
        bad = np.nonzero((act_out[i] != want_a).any(axis=1))[0]
        assert bad.size == 0, "%s: %d active labels differ after the last epilogue, the first: output %d" % (what, bad.size, bad[0])
        assert (act_out[i] == np.where(bit_out[i][:, None] == 1, out0[i] ^ delta[i][None, :], out0[i])).all(), what
