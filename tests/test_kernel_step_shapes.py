"""The kernel's own control flow — which lanes take which gate of a step — swept at its thresholds, against a reference that knows
nothing of steps.

run_program_kernel (csrc/engine/kernels.hip) picks a lane-to-gate mapping per step from the step's AND-family and free-gate counts:
narrow steps (several lanes per AND gate, the free gates behind them from the next wave boundary), wide steps with zero, one or
several whole one-gate-per-lane passes, a remainder in a multi-lane form or as a partly filled pass, free-gate batches over one or
several widths of the instance's thread group.  The oracle, the host interpreter (tests/hostsim) and the Python restatements share
none of that; real circuits hit the threshold-equality cases only by accident.  Here synthetic LAYERED programs are built so that the
compiled step k holds exactly (a_k, x_k) gates, with the (a, x) table DERIVED from the kernel's own quantities (`Lanes` / `narrow_lpg` /
`rem_lpg` / `shape_pairs` below — one restatement, cited to the kernel's lambdas, no literal thresholds):

  * CPU half (default non-GPU set): for each of the twelve (instances per workgroup, garble / evaluate, record form) combinations the
    table is derived, the program that carries it is compiled, and Program.step_stats() must give exactly the intended sequence and
    info["and_terms"] the intended form; every lane-mapping class and every equality edge must be in the table.  A compiler change
    that voids the coverage fails here, not silently.
  * GPU half: the programs garbled and evaluated for a ragged batch with distinct seeds and compared per instance with
    tests/gate_list_ref.py (pinned to the oracle in tests/test_gate_list_ref.py): whole ciphertext stream, CBC-MAC, output label0s,
    active labels, plaintext bits — with the AES hasher at 1, 2 and 4 instances per workgroup, with BLAKE3 at one, and once more with
    gate-id bases whose 64-bit tweak product carries out of the low word in the middle of the program (tweak_word).

Not covered on purpose: in rem_lpg the third alternative of the DUAL branch, `rem <= 2*(BT/LPG)`, sits behind the wider
`rem <= 2*(BT/LPG2)` and cannot be taken (LPG2 < LPG); no shape is invented for it.
"""
import contextlib
import os
import random
import re

import numpy as np
import pytest

import gate_list_ref as G
import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_THREADS = int(re.search(r"#define\s+GSV_BLOCK_THREADS\s+(\d+)", open(os.path.join(ROOT, "garbled_snark_verifier_amd", "csrc", "engine", "kernel_api.h")).read()).group(1))
XOR_BATCH = 2  # kernels.hip run_step: `constexpr int XB = 2` — a free-gate batch is XB widths of the thread group
N_INPUTS = 48
COMBINATIONS = [(ni, evaluate, terms) for terms in (2, 4) for ni in (1, 2, 4) for evaluate in (False, True)]


# ---- the kernel's step-shape quantities, restated ONCE (kernels.hip, run_program_kernel) ------------------------------------------------
class Lanes:
    """BT, LPG, LPG2 of one kernel instantiation as run on one program: `BT = GSV_BLOCK_THREADS / NI`; `LPG = EVAL ? 4 : 8`;
    `DUAL = FW && !EVAL && HASH == 0`, FW being the record form's instantiation (four-wire program) and dual_prog = four_wire;
    `LPG2 = DUAL ? 4 : LPG`.  HASH = 1 (BLAKE3) has no multi-lane form at all."""

    def __init__(self, ni, evaluate, terms, blake3=False):
        self.ni, self.evaluate, self.terms, self.blake3 = ni, evaluate, terms, blake3
        self.BT = BLOCK_THREADS // ni
        self.LPG = 4 if evaluate else 8
        self.dual = terms == 4 and not evaluate and not blake3
        self.LPG2 = 4 if self.dual else self.LPG


def xor_lane0(na):
    """`xor_lane0`: the free gates of a narrow step start at the next wave boundary behind the AND lanes."""
    return (na + 63) & ~63


def narrow_lpg(L, a, x):
    """`narrow_lpg`: lanes per AND gate of a narrow step (its AND lanes + free gates fit ONE pass), 0 = not narrow."""
    if L.blake3 or a == 0:
        return 0
    if xor_lane0(a * L.LPG) + x <= L.BT:
        return L.LPG
    if L.dual and xor_lane0(a * L.LPG2) + x <= L.BT:
        return L.LPG2
    return 0


def rem_lpg(L, a):
    """`rem_lpg`: lanes per gate of a wide step's AND remainder, 0 = one partly filled one-gate-per-lane pass."""
    if L.blake3:
        return 0
    rem = a % L.BT
    if L.dual:
        return L.LPG if rem <= L.BT // L.LPG else L.LPG2 if rem <= 2 * (L.BT // L.LPG2) else 0  # (the kernel's third alternative is unreachable)
    return L.LPG if rem <= 2 * (L.BT // L.LPG) else 0


def classify(L, a, x):
    """The lane mapping `run_step` and the record prefetch `rec_ptr` use for a step of a AND-family and x free gates:
    ("narrow", lanes per gate) or ("wide", one-gate-per-lane passes (2 = two or more), remainder form, free-gate widths (3 = more than
    one batch)), the remainder form being None, ("multi", lanes per gate, passes) or "partial"."""
    nl = narrow_lpg(L, a, x)
    if nl:
        return ("narrow", nl)
    rem, rl = a % L.BT, rem_lpg(L, a)
    whole = a // L.BT
    if rem == 0:
        form = None
    elif rl:
        form = ("multi", rl, -(-rem // (L.BT // rl)))
    else:
        form = "partial"
    return ("wide", min(whole, 2), form, min(-(-x // L.BT), XOR_BATCH + 1))


def and_values(L):
    BT, per, per2 = L.BT, L.BT // L.LPG, L.BT // L.LPG2
    v = [0, 1, per - 1, per, per + 1, 2 * per, 2 * per + 1]
    if L.LPG2 != L.LPG:
        v += [per2, 2 * per2, 2 * per2 + 1]
    v += [BT - 1, BT, BT + 1, BT + per, 2 * BT - 1, 2 * BT, 2 * BT + 1, 3 * BT - 1]
    return sorted(set(v))


def narrow_edges(L, a):
    """For a AND gates: the largest free-gate count for which the step is still narrow at LPG (and at LPG2), and that count plus one."""
    out = []
    if a:
        for lpg in sorted({L.LPG, L.LPG2}):
            room = L.BT - xor_lane0(a * lpg)
            if room >= 0:
                out += [room, room + 1]
    return out


def shape_pairs(L):
    """A sparse cover of and_values x free-gate counts: every AND count with its narrow edges and with two of the generic free-gate
    counts (0, 1, BT, BT + 1, XB * BT + 1), rotating, so that every generic count meets small, middle and large AND counts."""
    generic = [0, 1, L.BT, L.BT + 1, XOR_BATCH * L.BT + 1]
    pairs = []
    for i, a in enumerate(and_values(L)):
        for x in narrow_edges(L, a) + [generic[i % len(generic)], generic[(i + 2) % len(generic)]]:
            if (a or x) and (a, x) not in pairs:
                pairs.append((a, x))
    return pairs


def required_classes(L):
    """Every lane-mapping class the instantiation has: (narrow classes, whole one-gate-per-lane passes, remainder forms, free-gate widths)."""
    narrow = [("narrow", L.LPG)] + ([("narrow", L.LPG2)] if L.dual else [])
    forms = {None, "partial", ("multi", L.LPG, 1)} | ({("multi", L.LPG2, 1), ("multi", L.LPG2, 2)} if L.dual else {("multi", L.LPG, 2)})
    return narrow, {0, 1, 2}, forms, {0, 1, 2, XOR_BATCH + 1}


def program_shapes(ni, terms):
    """One program per (instances per workgroup, record form): the garbling table and the evaluating table in one step sequence (the
    evaluator needs the garbler's ciphertexts of the same program), shuffled so that the two-steps-ahead record prefetch crosses from
    every form into every other."""
    pairs = []
    for evaluate in (False, True):
        for p in shape_pairs(Lanes(ni, evaluate, terms)):
            if p not in pairs:
                pairs.append(p)
    random.Random(1000 * ni + terms).shuffle(pairs)
    return pairs


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
def build_layered(shapes, n_inputs=N_INPUTS):
    """A layered circuit whose step k (ASAP level k + 1 after fusion) holds exactly shapes[k] = (AND-family, free) gates.
    Every AND-family gate takes one output of level k - 1 and one of level k - 1, of an earlier level or a constant; every free gate
    takes level k - 1 wires and is a circuit output (pinned: fusion keeps it as a record of its own).  An AND output is pinned too
    when nothing reads it (its label is then compared) or when its only reader is a Xor / Xnor (fuse_trace would fold that reader into
    the AND's record).  Gate types rotate through all eight AND-family and all three free types; a dead gate of a rotating type follows
    every 89th gate (it consumes a gate id); AND and free gates of a step alternate in the list, so stream order is not record order.
    Returns (gates, outputs, step_of_gate)."""
    gates, outputs, step_of, all_and_outs = [], [], [], []
    nxt = 2 + n_inputs
    prev, older = list(range(2, 2 + n_inputs)), []
    readers = {}
    n_and = n_free = n_dead = 0

    def emit(t, a, b, live, k):
        nonlocal nxt, n_dead
        c = None
        if live:
            c, nxt = nxt, nxt + 1
            readers.setdefault(a, []).append(t)
            if t != G.NOT:
                readers.setdefault(b, []).append(t)
        gates.append((t, a, b, c))
        step_of.append(k)
        if live and len(gates) % 89 == 0:
            gates.append((n_dead % 11, a, b, None))
            step_of.append(k)
            n_dead += 1
        return c

    for k, (na, nx) in enumerate(shapes):
        ands, frees = [], []
        for j in range(na):
            p = prev[j % len(prev)]
            sel = (j + k) % 6
            if sel == 0:
                q = j // 6 & 1  # a constant operand
            elif sel in (1, 2) and older:
                q = older[(j * 13 + k) % len(older)]
            else:
                q = prev[(j * 5 + 3) % len(prev)]
            ands.append((n_and % 8,) + ((p, q) if j & 1 else (q, p)))
            n_and += 1
        for j in range(nx):
            t = 8 + n_free % 3
            n_free += 1
            p = prev[(j * 3 + 1) % len(prev)]
            q = prev[(j * 7 + 2) % len(prev)]
            if q == p:
                q = prev[(j * 7 + 3) % len(prev)] if len(prev) > 1 else (older or [0])[-1]  # (a level of one wire: pair it with an earlier one)
            frees.append((t, p, p if t == G.NOT else q))
        level, and_outs = [], []
        for j in range(max(na, nx)):
            if j < na:
                c = emit(*ands[j], True, k)
                level.append(c)
                and_outs.append(c)
            if j < nx:
                c = emit(*frees[j], True, k)
                level.append(c)
                outputs.append(c)
        all_and_outs += and_outs
        older = (older + prev)[-4096:]
        prev = level
    for i, c in enumerate(all_and_outs):  # (pinning is decided once every reader is known)
        r = readers.get(c, [])
        if not r or (len(r) == 1 and r[0] in (G.XOR, G.XNOR)) or i % 5 == 0:
            outputs.append(c)
    return gates, outputs, step_of


@contextlib.contextmanager
def and_terms_env(terms):
    """GSV_AND_TERMS=terms while a program is compiled (a compile knob: read by the entry point that compiles, kept with the program)."""
    with pytest.MonkeyPatch.context() as mp:  # saves and restores this one variable
        mp.setenv("GSV_AND_TERMS", str(terms))
        yield


_built = {}


def layered_program(gsv, ni, terms):
    """(gates, outputs, step_of_gate, shapes, Program compiled in the `terms` record form) — built once per process."""
    key = (ni, terms)
    if key not in _built:
        shapes = program_shapes(ni, terms)
        gates, outputs, step_of = build_layered(shapes)
        with and_terms_env(terms):
            prog = gsv.Program.from_gates(N_INPUTS, gates, outputs)
        _built[key] = (gates, outputs, step_of, shapes, prog)
    return _built[key]


# ---- CPU half --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni,evaluate,terms", COMBINATIONS)
def test_shape_table_is_what_the_compiler_emits(ni, evaluate, terms):
    import garbled_snark_verifier_amd as gsv
    L = Lanes(ni, evaluate, terms)
    table = shape_pairs(L)
    gates, outputs, step_of, shapes, prog = layered_program(gsv, ni, terms)
    assert prog.info["and_terms"] == terms
    stats = prog.step_stats()
    assert prog.info["n_steps"] == len(shapes) and [tuple(int(v) for v in row[:2]) for row in stats] == shapes, "the compiled steps are not the intended (and_cnt, xor_cnt) sequence"
    assert prog.info["n_gates"] == len(gates) and prog.info["n_dead"] == sum(1 for g in gates if g[3] is None) > 0
    assert prog.info["n_ciphertexts"] == sum(a for a, _ in shapes) and sorted(set(g[0] for g in gates)) == list(range(11))
    assert set(table) <= set(shapes)
    # every value the sweep is about, from the same quantities
    ands, xors = set(a for a, _ in table), {}
    for a, x in table:
        xors.setdefault(a, set()).add(x)
    BT, per, per2 = L.BT, L.BT // L.LPG, L.BT // L.LPG2
    assert {0, 1, per - 1, per, per + 1, 2 * per, 2 * per + 1, BT - 1, BT, BT + 1, BT + per, 2 * BT, 2 * BT + 1, 3 * BT - 1} <= ands
    assert L.LPG2 == L.LPG or {per2, 2 * per2, 2 * per2 + 1} <= ands
    assert L.dual == (terms == 4 and not evaluate) and (L.LPG2 != L.LPG) == L.dual
    for a in ands:
        assert set(narrow_edges(L, a)) <= xors[a]
    for x in (0, 1, BT, BT + 1, XOR_BATCH * BT + 1):
        assert len([a for a in ands if x in xors[a]]) >= 3
    # the equality edges: the last narrow count is narrow, one more is not (or is narrow only at the other lane count)
    n_edges = 0
    for a in ands:
        for lpg in sorted({L.LPG, L.LPG2}):
            room = BT - xor_lane0(a * lpg)
            if a and room >= 0:
                assert xor_lane0(a * lpg) + room == BT and narrow_lpg(L, a, room) in (L.LPG, L.LPG2) and narrow_lpg(L, a, room + 1) != lpg
                if lpg == L.LPG2:
                    assert narrow_lpg(L, a, room + 1) == 0
                n_edges += 1
    assert n_edges >= 3  # 1, BT/LPG - 1 and BT/LPG AND gates always leave room for a narrow step
    assert rem_lpg(L, per) == L.LPG and rem_lpg(L, 2 * per2) == L.LPG2 and rem_lpg(L, 2 * per2 + 1) == 0 and rem_lpg(L, BT + per) == L.LPG and rem_lpg(L, 3 * BT - 1) == 0
    # every class of the instantiation
    classes = set(classify(L, a, x) for a, x in table)
    narrow, whole, forms, free = required_classes(L)
    wide = [c for c in classes if c[0] == "wide"]
    assert set(narrow) <= classes and whole <= set(c[1] for c in wide) and forms <= set(c[2] for c in wide) and free <= set(c[3] for c in wide)
    # a partly filled pass alone, behind one and behind two whole passes; a multi-lane remainder prefetched (no whole pass) and loaded in the step
    assert {(w, f) for w in (0, 1, 2) for f in ("partial", ("multi", L.LPG, 1))} <= set((c[1], c[2]) for c in wide)


def test_blake3_kernel_has_one_gate_per_lane_only():
    L = Lanes(1, False, 2, blake3=True)
    assert all(classify(L, a, x)[0] == "wide" and classify(L, a, x)[2] in (None, "partial") for a, x in program_shapes(1, 2))
    assert {0, 1, 2} <= set(classify(L, a, x)[1] for a, x in program_shapes(1, 2))


def test_layered_reference_runs_garble_to_evaluate_on_the_cpu():
    """The builder's gate lists are well formed for the reference (every wire written once, before it is read) and the reference's
    evaluator recovers select(label0, bit) from its garbler's stream on them — with a gate-id base whose carry lands inside."""
    gates, outputs, _ = build_layered([(3, 2), (0, 1), (5, 0), (1, 4), (2, 2)], n_inputs=4)
    labs = o.chacha_labels(3, 3 + 4)
    delta, consts, inputs = labs[0], labs[1:3], labs[3:]
    base = 2**32 - len(gates) // 2
    g = G.garble(gates, delta, consts, inputs, outputs, gate_id_base=base)
    for bits in ([0, 0, 0, 0], [1, 0, 1, 1], [1, 1, 1, 1]):
        bits = np.array(bits, np.uint8)
        act = np.where(bits[:, None] == 1, inputs ^ delta[None, :], inputs)
        e = G.evaluate(gates, (consts[0], consts[1] ^ delta), act, bits, g.ciphertexts, outputs, gate_id_base=base)
        assert (e.output_active == np.where(e.output_bits[:, None] == 1, g.output_label0 ^ delta[None, :], g.output_label0)).all()
        assert e.n_consumed == g.n_ciphertexts == 11


# ---- GPU half --------------------------------------------------------------------------------------------------------------------------------
def _where(step_of, gates, shapes, ct_index):
    """Gate, step and step shape of ciphertext `ct_index` of the stream (for a failure's message)."""
    k = -1
    for i, g in enumerate(gates):
        if g[3] is not None and g[0] < 8:
            k += 1
            if k == ct_index:
                return "gate %d, step %d with (and_cnt, xor_cnt) = %s" % (i, step_of[i], shapes[step_of[i]])
    return "?"


def _run_and_compare(gsv, engine, ni, terms, seeds, base=0, hasher="aes"):
    gates, outputs, step_of, shapes, prog = layered_program(gsv, ni, terms)
    B = len(seeds)
    labs = [gsv.labels_from_seed(s, N_INPUTS) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([np.stack([x[1], x[2]]) for x in labs]); inputs = np.stack([x[3] for x in labs])
    bits = np.random.default_rng(seeds[0]).integers(0, 2, (B, N_INPUTS)).astype(np.uint8)
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    sess = gsv.Session(engine, prog, B)
    assert sess.instances_per_workgroup == ni
    sess.set_hasher(hasher)
    sess.set_garble_inputs(delta, consts, inputs)
    sess.garble(base)
    sess.sync()
    out0 = sess.read_outputs()
    cts = [sess.read_ciphertexts(i) for i in range(B)]
    macs = [sess.ciphertext_hash(i) for i in range(B)]
    sess.close()
    ev = gsv.Session(engine, prog, B)
    assert ev.instances_per_workgroup == ni
    ev.set_hasher(hasher)
    ev.set_evaluate_inputs(consts_active, active, bits)
    for i in range(B):
        ev.upload_ciphertexts(i, cts[i])
    ev.evaluate(base)
    ev.sync()
    act_out, bit_out = ev.read_outputs(with_bits=True)
    ev.close()
    o.set_hasher(hasher)
    try:
        for i in range(B):
            g = G.garble(gates, delta[i], consts[i], inputs[i], outputs, gate_id_base=base)
            what = "instance %d of %d (seed %d), %d per workgroup, %d-wire records, gate_id_base %d, %s" % (i, B, seeds[i], ni, terms, base, hasher)
            assert cts[i].shape == g.ciphertexts.shape
            bad = np.nonzero((cts[i] != g.ciphertexts).any(axis=1))[0]
            assert bad.size == 0, "%s: %d ciphertexts differ, the first at stream index %d: %s" % (what, bad.size, bad[0], _where(step_of, gates, shapes, int(bad[0])))
            assert macs[i] == g.ct_hash, what
            bad = np.nonzero((out0[i] != g.output_label0).any(axis=1))[0]
            assert bad.size == 0, "%s: %d output label0s differ, the first: output %d (wire %d)" % (what, bad.size, bad[0], outputs[bad[0]])
            e = G.evaluate(gates, consts_active[i], active[i], bits[i], g.ciphertexts, outputs, gate_id_base=base)
            assert (bit_out[i] == e.output_bits).all(), what + ": plaintext bits differ"
            bad = np.nonzero((act_out[i] != e.output_active).any(axis=1))[0]
            assert bad.size == 0, "%s: %d active labels differ, the first: output %d (wire %d)" % (what, bad.size, bad[0], outputs[bad[0]])
            assert (act_out[i] == np.where(bit_out[i][:, None] == 1, out0[i] ^ delta[i][None, :], out0[i])).all(), what + ": active label != select(label0, bit)"
    finally:
        o.set_hasher("aes")


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 2, 4])
@pytest.mark.parametrize("terms", [2, 4])
def test_step_shapes_on_the_device(engine, monkeypatch, terms, ni):
    """A ragged batch (2 NI + 1 instances with distinct seeds: the last workgroup has idle groups) through every step shape."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_AND_TERMS", str(terms))
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    _run_and_compare(gsv, engine, ni, terms, [500 + 10 * ni + k for k in range(2 * ni + 1)])


@pytest.mark.gpu
def test_step_shapes_with_the_blake3_hasher(engine, monkeypatch):
    """HASH = 1: one gate per lane in every step, whole passes and a partly filled one, over the same step sequence."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_AND_TERMS", "2")
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", "1")
    _run_and_compare(gsv, engine, 1, 2, [31, 32, 33], hasher="blake3")


def gate_id_bases(n_gates):
    """The carry out of the tweak's low word in the middle of the program; past 2^32; far past 2^48 (and below 2^63)."""
    return [2**32 - n_gates // 2, 2**32 + 12345, 2**55 + 0x1234_5678_9ABC]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("ni", [1, 4])
@pytest.mark.parametrize("terms", [2, 4])
def test_step_shapes_with_gate_id_bases(engine, monkeypatch, terms, ni, which):
    """tweak_word forms gate_id * 0xDEADBEEFCAFEBABE in 64 bits from gate_id = base + index: every session entry point takes the base,
    and only a non-zero one moves the ids of a small program past 2^32.  Same programs, same comparisons, same ragged batch."""
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_AND_TERMS", str(terms))
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    n_gates = len(layered_program(gsv, ni, terms)[0])
    base = gate_id_bases(n_gates)[which]
    assert base < 2**32 < base + n_gates if which == 0 else 2**32 < base < 2**63 and (which == 1 or base > 2**48)
    _run_and_compare(gsv, engine, ni, terms, [700 + 10 * which + k for k in range(2 * ni + 1)], base=base)


@pytest.mark.gpu
def test_chained_replay_with_a_gate_id_base(engine):
    """replays = 2 with a non-zero base, the carry inside the second replay: the device's chain (gate ids continue across replays,
    outputs fed back) == two single runs of the host interpreter glued by hand, the second with gid_base = base + n_gates — the device
    form of test_engine_host.py::test_compiled_chain_replay_matches_streamed_chain (the interpreter is held to the oracle at base 0
    there and to gate_list_ref with bases in test_gate_list_ref.py)."""
    import garbled_snark_verifier_amd as gsv
    import hostsim_lib as h
    prog = gsv.Program.from_circuit("fq2_mul", chain_feedback=True)
    sp1 = h.SimProgram("fq2_mul")
    n_in, n_out, n_gates = prog.info["n_inputs"], prog.info["n_outputs"], prog.info["n_gates"]
    base = 2**32 - n_gates - n_gates // 2
    seeds = [41, 42, 43]
    labs = [h.labels_from_seed(s, 3 + n_in) for s in seeds]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([x[1:3] for x in labs]); inputs = np.stack([x[3:] for x in labs])
    sess = gsv.Session(engine, prog, len(seeds), 2)
    sess.set_garble_inputs(delta, consts, inputs)
    sess.garble(base)
    sess.sync()
    out = sess.read_outputs()
    bits = np.random.default_rng(4).integers(0, 2, (len(seeds), n_in)).astype(np.uint8)
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    ev = gsv.Session(engine, prog, len(seeds), 2)
    ev.set_evaluate_inputs(consts_active, active, bits)
    for i in range(len(seeds)):
        ev.upload_ciphertexts(i, sess.read_ciphertexts(i))
    ev.evaluate(base)
    ev.sync()
    act_out, bit_out = ev.read_outputs(with_bits=True)
    for i in range(len(seeds)):
        out_a, cts_a = sp1.garble(delta[i], consts[i], inputs[i], gid_base=base)
        inputs_b = inputs[i].copy()
        inputs_b[:n_out] = out_a
        out_b, cts_b = sp1.garble(delta[i], consts[i], inputs_b, gid_base=base + n_gates)
        glued = np.concatenate([cts_a, cts_b])
        assert (sess.read_ciphertexts(i) == glued).all() and sess.ciphertext_hash(i) == h.cbcmac(glued)
        assert (out[i] == out_b).all()
        oa, ob = sp1.evaluate(consts_active[i], active[i], bits[i], cts_a, gid_base=base)
        act_b, bits_b = active[i].copy(), bits[i].copy()
        act_b[:n_out], bits_b[:n_out] = oa, ob
        oa, ob = sp1.evaluate(consts_active[i], act_b, bits_b, cts_b, gid_base=base + n_gates)
        assert (bit_out[i] == ob).all() and (act_out[i] == oa).all()
        assert (act_out[i] == np.where(ob[:, None] == 1, out[i] ^ delta[i][None, :], out[i])).all()
    sess.close(); ev.close()
