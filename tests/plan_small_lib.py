"""Synthetic plans for tests/test_plan_small.py (TEST INFRASTRUCTURE, CPU only): a plan recorded through gsv.PlanRecorder from unit
programs (Program.from_gates of tests/test_kernel_step_shapes.build_layered circuits) and glue gates, and the SAME circuit as one flat
gate list for tests/gate_list_ref.py — every call replaced by its unit's gates with the wires renamed, in stream order, dead gates
included.  The flattening is written once, here (SmallPlan.call); the reference knows nothing of calls, windows, hand-over copies,
completion flags or drain segments.

Wire ids of the flat list: 0 / 1 the constants, the plan recorder's own ids for every wire the plan level sees (inputs, glue wires,
call outputs), ids from 2^40 on for the wires inside a call.
"""
import numpy as np

import gate_list_ref as G
import oracle_lib as o
import test_kernel_step_shapes as S

BT = S.BLOCK_THREADS
PRIVATE0 = 1 << 40


class Unit:
    """A unit program: its gate list (Program.from_gates numbering), its output wires and the Program compiled for a plan recorder."""

    def __init__(self, gsv, rec, name, terms, n_inputs, shapes):
        self.name, self.terms, self.n_inputs, self.shapes = name, terms, n_inputs, shapes
        self.gates, self.outputs, _ = S.build_layered(shapes, n_inputs=n_inputs)
        with S.and_terms_env(terms):
            self.prog = gsv.Program.from_gates(n_inputs, self.gates, self.outputs, for_plan=rec)
        self.n_outputs = len(self.outputs)
        self.n_ct = sum(1 for g in self.gates if g[3] is not None and g[0] < 8)
        self.n_dead = sum(1 for g in self.gates if g[3] is None)


class Call:
    """One call of the finished plan, in stream order: a unit call or a run of glue gates.  flat[g0:g1] are its gates."""

    def __init__(self, unit, in_wires, out_wires, g0, g1):
        self.unit, self.in_wires, self.out_wires, self.g0, self.g1 = unit, list(in_wires), list(out_wires), g0, g1
        self.name = unit.name if unit else "glue"


class SmallPlan:
    def __init__(self, gsv, window_div=4):
        self.gsv = gsv
        self.rec = gsv.PlanRecorder(window_div=window_div)
        self.inputs, self.flat, self.calls, self._pending = [], [], [], []
        self._private = PRIVATE0
        self.plan = self.outputs = None

    def input_wire(self):
        w = self.rec.input_wire()
        self.inputs.append(w)
        return w

    def glue(self, t, a, b, live=True):
        """One glue gate between calls; returns its output wire (None for a dead gate)."""
        c = self.rec.allocate_wire(1) if live else None
        self._pending.append((t, a, b, c))
        return c

    def _close_glue(self):
        if self._pending:
            self.rec.push_gates(self._pending)
            g0 = len(self.flat)
            self.flat += self._pending
            reads = []
            defs = [g[3] for g in self._pending if g[3] is not None]
            for t, a, b, _ in self._pending:
                for w in (a, b):
                    if w not in defs and w not in reads:
                        reads.append(w)
            self.calls.append(Call(None, reads, defs, g0, len(self.flat)))
            self._pending = []

    def call(self, unit, in_wires):
        """THE flattening: the unit's gates with constants kept, input i -> in_wires[i], output j -> the fresh plan wire the recorder
        returned for it, every other wire -> an id of its own."""
        assert len(in_wires) == unit.n_inputs
        self._close_glue()
        out = self.rec.call(unit.prog, in_wires)
        m = {0: 0, 1: 1}
        for i, w in enumerate(in_wires):
            m[2 + i] = w
        for j, w in enumerate(unit.outputs):
            assert w not in m, "a unit output must be a wire the unit produces"
            m[w] = out[j]
        g0 = len(self.flat)
        for t, a, b, c in unit.gates:
            if c is not None and c not in m:
                m[c] = self._private
                self._private += 1
            self.flat.append((t, m[a], m[b], None if c is None else m[c]))
        self.calls.append(Call(unit, in_wires, out, g0, len(self.flat)))
        return out

    def finish(self, outputs):
        self._close_glue()
        self.outputs = list(outputs)
        self.plan = self.rec.finish(self.outputs)
        self.is_ct = np.array([g[3] is not None and g[0] < 8 for g in self.flat])
        self.ct_before = np.concatenate([[0], np.cumsum(self.is_ct)])  # ciphertexts of flat[:i]
        return self.plan

    # ---- where a difference sits (for a failure's message)
    def call_of_gate(self, i):
        for k, c in enumerate(self.calls):
            if c.g0 <= i < c.g1:
                return k
        return None

    def where_ct(self, ct_index):
        i = int(np.searchsorted(self.ct_before, ct_index, side="right")) - 1
        k = self.call_of_gate(i)
        c = self.calls[k]
        return "flat gate %d = gate %d of call %d (%s, gates [%d, %d), ciphertexts from %d)" % (i, i - c.g0, k, c.name, c.g0, c.g1, self.ct_before[c.g0])

    def where_wire(self, w):
        if w in (0, 1):
            return "constant %d" % w
        if w in self.inputs:
            return "plan input %d" % self.inputs.index(w)
        for k, c in enumerate(self.calls):
            if w in c.out_wires:
                i = [j for j in range(c.g0, c.g1) if self.flat[j][3] == w][0]
                return "output %d of call %d (%s), written by flat gate %d" % (c.out_wires.index(w), k, c.name, i)
        return "wire %d" % w

    # ---- dependencies between the calls, from the flat wires alone
    def producers(self):
        p = {}
        for k, c in enumerate(self.calls):
            for w in c.out_wires:
                p[w] = k
        return p

    def depends(self):
        """depends[k] = set of calls k reads from, transitively."""
        p = self.producers()
        dep = []
        for k, c in enumerate(self.calls):
            d = set()
            for w in c.in_wires:
                if w in p:
                    d |= {p[w]} | dep[p[w]]
            dep.append(d)
        return dep


def build_small_plan(gsv):
    """The plan of tests/test_plan_small.py (see its docstring for what it must contain): ten unit calls of four units and three glue runs."""
    sp = SmallPlan(gsv, window_div=4)
    u = sp.units = {
        "two": Unit(gsv, sp.rec, "two", 2, 16, [(20, 12), (9, 30), (33, 5), (12, 8), (40, 20)]),
        "four": Unit(gsv, sp.rec, "four", 4, 12, [(10, 6), (17, 9), (5, 14), (24, 3), (8, 8), (30, 10)]),
        "long": Unit(gsv, sp.rec, "long", 2, BT + 6, [(50, BT + 76), (21, 40)]),  # inputs and outputs: more than one trip of the hand-over loops at every layout
        "free": Unit(gsv, sp.rec, "free", 2, 8, [(0, 6), (0, 5), (0, 3)]),       # no ciphertexts
    }
    X = [sp.input_wire() for _ in range(BT + 40)]
    c0 = sp.call(u["two"], X[0:16])                     # chain 1
    c1 = sp.call(u["four"], X[16:28])                   # chain 2: shares nothing with chain 1
    g = [sp.glue(0, c0[0], X[30]), sp.glue(G.XOR, c0[1], c0[2]), sp.glue(G.NOT, X[31], X[31]), sp.glue(7, c0[3], 1)]
    sp.glue(3, c0[0], X[32], live=False)
    for t, i, j in ((G.XNOR, 0, 1), (2, 2, 3), (5, 4, 0), (G.XOR, 5, 33), (6, 6, 7), (1, 34, 35)):  # operands: g[i] below 30, else X[i]; one constant
        g.append(sp.glue(t, g[i] if i < 30 else X[i], 0 if t == 5 else g[j] if j < 30 else X[j]))
    c2 = sp.call(u["two"], g[0:10] + [0, 1] + c0[4:8])  # glue wires, both constants, an earlier call's outputs
    c3 = sp.call(u["four"], c1[0:12])                   # an earlier call's outputs only (chain 2 goes on)
    c4 = sp.call(u["long"], X[40:40 + BT - 2] + c2[0:4] + c3[0:4])
    h = [sp.glue(4, c4[-1], c4[-2]), sp.glue(G.XOR, c4[BT], c3[5]), sp.glue(G.XNOR, c4[BT + 1], c4[0])]
    h.append(sp.glue(0, h[0], h[1]))
    h.append(sp.glue(G.NOT, h[2], h[2]))
    c5 = sp.call(u["two"], c4[-8:] + h[0:4] + c4[BT:BT + 4])  # outputs of the long unit past the first trip of the post-copy loop
    c6 = sp.call(u["free"], c5[0:4] + c3[4:8])
    c7 = sp.call(u["four"], c6[0:6] + c4[BT - 6:BT])
    c8 = sp.call(u["long"], c4[0:BT + 6])               # a pre-copy of more than BT wires that another call wrote
    t = [sp.glue(G.XOR, c8[-1], c7[0]), sp.glue(1, c8[BT + 2], c5[7])]
    outs = [X[5], 1] + c8[-20:] + c8[:5] + c7 + c5[4:] + [h[4]] + c2[8:12] + [c4[BT + 10]] + t + c6[6:]
    sp.finish(outs)
    return sp


_refs = {}


def labels(gsv, sp, seed):
    """(delta, consts [2,16], input label0s, input bits) of one instance: labels as GarbleMode draws them from `seed`, bits from it too."""
    d, f, t, inp = gsv.labels_from_seed(seed, len(sp.inputs))
    bits = np.random.default_rng(seed).integers(0, 2, len(sp.inputs)).astype(np.uint8)
    return d, np.stack([f, t]), inp, bits


def reference(gsv, sp, seed, base=0, hasher="aes"):
    """gate_list_ref on the flat list, once per (seed, base, hasher) of a test session: (GarbleRef, EvalRef)."""
    key = (id(sp), seed, base, hasher)
    if key not in _refs:
        d, consts, inp, bits = labels(gsv, sp, seed)
        o.set_hasher(hasher)
        try:
            g = G.garble(sp.flat, d, consts, inp, sp.outputs, gate_id_base=base, input_wires=sp.inputs)
            act = np.where(bits[:, None] == 1, inp ^ d[None, :], inp)
            e = G.evaluate(sp.flat, (consts[0], consts[1] ^ d), act, bits, g.ciphertexts, sp.outputs, gate_id_base=base, input_wires=sp.inputs)
        finally:
            o.set_hasher("aes")
        _refs[key] = (g, e)
    return _refs[key]
