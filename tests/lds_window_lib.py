"""Builder of the synthetic programs of tests/test_lds_window_edges.py (TEST INFRASTRUCTURE, CPU only): gate lists whose compiled image
fills one instance's share of the LDS label window exactly, with the step that takes the last entries and the step that reads them
of a chosen lane-mapping class.  The shapes come from the kernel's quantities as restated once in tests/test_kernel_step_shapes.py
(`Lanes`, `classify`, `narrow_edges`); nothing here knows a threshold of its own.

How a gate list steers the compiler (program.hpp, compile_program 4. and fuse_trace) — every rule below is checked on the compiled
image by the CPU half of the test, none is trusted:
  * a wire gets a window entry only if it is not pinned (no input, no output); the window is handed out next-fit, and before
    anything is released that is: entries 1, 2, 3 ... in record order;
  * a wire keeps its entry until the step of its last reader: the FILL wires are read by the last step and hold entries
    1 .. share - 1 - T through the whole program, so that the TOP step's T outputs take exactly the remaining ones;
  * an unpinned free gate is folded into its readers unless it has three or more of them, and the Xor that is the single reader of an
    unpinned AND output is folded into that AND (which moves it a level later): top wires are read three times or more where they
    are free gates and twice or more otherwise, fill wires twice or more — build() counts and refuses a list that breaks this;
  * a Xor tree with one reader IS folded into that reader: that is how the reader step's records get a top wire into every operand
    field (a1 a2 b1 b2 p / a1 .. a4 b1 .. b4 p / x1 .. x4) while the gate list stays one of two-input gates.
"""
import os
import re

import gate_list_ref as G
import test_kernel_step_shapes as S

_LIMITS = open(os.path.join(S.ROOT, "garbled_snark_verifier_amd", "csrc", "engine", "limits.h")).read()
WINDOW = int(re.search(r"#define\s+GSV_LDS_SLOTS\s+(\d+)u", _LIMITS).group(1))  # entries of the whole LDS label window
DIVS = (1, 2, 4)      # instances per workgroup = window_div of the image: shares of WINDOW / d entries
WAVE = 64             # kernels.hip `xor_lane0`: the free lanes of a narrow step start at the next multiple of the wave size
N_INPUTS = 64
SURPLUS = 5           # outputs of an overfull top step beyond the free entries
DEAD_EVERY = 97       # a dead gate (it consumes a gate id) behind every 97th live one


def room(L, a):
    """The most free gates with which a step of `a` AND gates is still narrow at L.LPG lanes per gate (kernels.hip `narrow_lpg`)."""
    return L.BT - S.xor_lane0(a * L.LPG)


def variants(d, terms):
    """name -> ((AND, free) of the top step, (AND, free) of the reader step) for shares of WINDOW / d and the `terms`-wire record form.
    The classes these shapes have in the garbling and in the evaluating instantiation are spelled out in expected_classes()."""
    Lg = S.Lanes(d, False, terms)
    BT, per_g, per_e = Lg.BT, Lg.BT // Lg.LPG, Lg.BT // S.Lanes(d, True, terms).LPG
    half = per_g // 2
    a_multi, a_quarter = per_g - WAVE // Lg.LPG, per_e - WAVE // S.Lanes(d, True, terms).LPG
    return {
        # a whole one-gate-per-lane pass writes the last entries (16-byte st) and one reads them (16-byte ld)
        "pass": ((BT, 0), (BT, per_g)),
        # a narrow step: multi-lane AND gates in front, the free lanes behind them write / read the last entries (16 bytes)
        "narrow_free": ((half, BT // 4), (half, room(Lg, half))),
        # a free-gate phase of more than one batch (XOR_BATCH widths of the thread group); its readers: a third width again
        "wide_free": ((0, S.XOR_BATCH * BT + 1), (per_g, S.XOR_BATCH * BT + 1)),
        # one full multi-lane pass at LPG writes (4-byte st_word); read by multi-lane gates with free lanes behind them
        "multi": ((per_g, 0), (a_multi, room(Lg, a_multi))),
        # as many AND gates as fit at four lanes each: the four-lane x2 form when a four-wire program is garbled, two eight-lane passes of
        # a wide step's remainder when a two-wire program is, one narrow pass when either is evaluated
        "quarter": ((per_e, 0), (a_quarter, WAVE)),
    }


def expected_classes(d, terms, name):
    """{evaluate: (class of the top step, class of the reader step)} as S.classify must give them (asserted by the CPU half)."""
    out = {}
    for evaluate in (False, True):
        L = S.Lanes(d, evaluate, terms)
        multi1 = ("multi", L.LPG, 1)
        if name == "pass":
            c = (("wide", 1, None, 0), ("wide", 1, None, 1))
        elif name == "narrow_free" or name == "multi":
            c = (("narrow", L.LPG), ("narrow", L.LPG))
        elif name == "wide_free":
            c = (("wide", 0, None, S.XOR_BATCH + 1), ("wide", 0, multi1, S.XOR_BATCH + 1))
        elif evaluate or L.dual:
            c = (("narrow", L.LPG2), ("narrow", L.LPG2))
        else:
            c = (("wide", 0, ("multi", L.LPG, 2), 0), ("wide", 0, ("multi", L.LPG, 2), 1))
        out[evaluate] = c
    return out


def access_paths(L, cls, shape):
    """The access paths through which the records of a step of class `cls` reach the label window: (of its AND records, of its free
    records), None where the step has none.  AND records: "lane16" = one gate per lane, 16-byte ld / st; ("word", lanes per gate,
    "x2" or "x1") = a multi-lane form, 4-byte ld_word / st_word.  Free records: ("free16", "narrow" | "wide" | "batches") = 16-byte
    ld / st from a narrow step's free lanes, from one batch of a wide step, from more than one batch."""
    a, x = shape
    if cls[0] == "narrow":
        return (("word", cls[1], "x2" if L.dual and cls[1] == L.LPG2 else "x1"), ("free16", "narrow") if x else None)
    _, whole, form, widths = cls
    kinds = set()
    if whole:
        kinds.add("lane16")
    if form == "partial":
        kinds.add("lane16")
    elif form:
        kinds.add(("word", form[1], "x2" if L.dual and form[1] == L.LPG2 else "x1"))
    assert len(kinds) <= 1, "a step of one class was asked for: %r" % (cls,)
    return (kinds.pop() if kinds else None, ("free16", "batches" if widths > S.XOR_BATCH else "wide") if x else None)


class Edge:
    """One program: .gates .outputs .step_of (gate index -> step) .step_of_wire .shapes (the four intended steps) .tops (top-step wires,
    AND gates first) .top_read_by (wire -> kinds of reader records, "and" / "free") .reader_operands (operand fields of the reader step
    that name a wire) .fill .surplus."""


def build(share, terms, top, reader, surplus=0, n_inputs=N_INPUTS):
    """The gate list for a window share of `share` entries: fill (step 0), top (step 1, top[0] AND-family + top[1] free gates, `surplus` of
    them more than there are free entries), reader (step 2), last (step 3)."""
    T = top[0] + top[1] - surplus          # entries the top step takes
    F = share - 1 - T                      # entries 1 .. F: the fill wires
    assert T >= 9 and F >= 2 and surplus >= 0
    e = Edge()
    gates, step_of, outputs, step_of_wire = [], [], [], {}
    reads = {}
    nxt = [2 + n_inputs]
    n_live = [0]

    def emit(t, a, b, k):
        c = nxt[0]
        nxt[0] += 1
        gates.append((t, a, b, c))
        step_of.append(k)
        step_of_wire[c] = k
        reads[a] = reads.get(a, 0) + 1
        if t != G.NOT:
            reads[b] = reads.get(b, 0) + 1
        n_live[0] += 1
        if n_live[0] % DEAD_EVERY == 0:
            gates.append(((n_live[0] // DEAD_EVERY) % 11, a, b, None))
            step_of.append(k)
        return c

    ins = list(range(2, 2 + n_inputs))
    # step 0: the fill wires, AND-family gates of every type over the inputs
    fill = [emit(j % 8, ins[j % n_inputs], ins[(5 * j + 3) % n_inputs], 0) for j in range(F)]
    # step 1: the top wires, over fill wires
    tops = [emit(j % 8, fill[(3 * j) % F], fill[(3 * j + 1) % F], 1) for j in range(top[0])]
    for j in range(top[1]):
        t = 8 + j % 3
        p, q = fill[(3 * j + 2) % F], fill[(3 * j + 7) % F]
        tops.append(emit(t, p, p if t == G.NOT else q, 1))
    free_tops = set(tops[top[0]:])

    # step 2: the reader records.  Each kind walks the top wires round-robin from the first one, so that a kind with at least as many
    # operand fields as there are top wires reads every one of them.
    read_by = {w: set() for w in tops}
    n_operands = [0]

    def taker(kind):
        pos = [0]

        def take(n):
            ws = [tops[(pos[0] + i) % len(tops)] for i in range(n)]
            pos[0] += n
            n_operands[0] += n
            for w in ws:
                read_by[w].add(kind)
            return ws
        return take

    def xor_tree(ws, k, parity=0):
        """ws[0] ^ ws[1] ^ ... as a tree of two-input gates with one reader each (folded into that reader), an Xnor in it if parity."""
        if len(ws) == 1:
            return ws[0]
        if len(ws) == 2:
            return emit(G.XNOR if parity else G.XOR, ws[0], ws[1], k)
        h = len(ws) // 2
        return emit(G.XOR, xor_tree(ws[:h], k, parity), xor_tree(ws[h:], k), k)

    take = taker("and")
    routs = []
    for i in range(reader[0]):
        form = i % 4
        if form == 0:    # every operand field: a1 a2 b1 b2 p, or a1 .. a4 b1 .. b4 p
            w = emit(i // 4 % 8, xor_tree(take(terms), 2, i & 4), xor_tree(take(terms), 2), 2)
            routs.append(emit(G.XNOR if i & 8 else G.XOR, w, take(1)[0], 2))
        elif form == 1:  # ABSENT operands: single wires on both sides and no p
            a, b = take(2)
            routs.append(emit((i // 4 + 3) % 8, a, b, 2))
        elif form == 2:  # one folded side, p
            w = emit((i // 4 + 5) % 8, take(1)[0], xor_tree(take(2), 2), 2)
            routs.append(emit(G.XOR, w, take(1)[0], 2))
        else:            # single wires and p
            a, b = take(2)
            routs.append(emit(G.XOR, emit((i // 4 + 6) % 8, a, b, 2), take(1)[0], 2))
    take = taker("free")
    for i in range(reader[1]):
        form = i % 8
        if form == 1:    # ABSENT operands: a two-operand free gate
            a, b = take(2)
            routs.append(emit(G.XNOR if i & 8 else G.XOR, a, b, 2))
        elif form == 5:  # ... and a one-operand one
            routs.append(emit(G.NOT, take(1)[0], 0, 2))
        else:            # x1 x2 x3 x4
            routs.append(xor_tree(take(4), 2, i & 16))
    outputs += routs
    # step 3: every record reads a reader output (pinned: HBM) — that is what puts it behind the reader step — beside fill wires (window):
    # an AND-family gate per fill wire (an AND reader is never folded into the wire's own record), and for every 8th a free record
    # fill ^ fill ^ reader output
    R = len(routs)
    n_last_free = 0
    for j in range(F):
        p, q = (fill[j], routs[j % R]) if j & 1 else (routs[j % R], fill[j])
        outputs.append(emit(j % 8, p, q, 3))
        if j % 8 == 3:
            u = emit(G.XNOR if j & 8 else G.XOR, fill[j], fill[(j + 1) % F], 3)
            outputs.append(emit(G.XOR, u, routs[(j + R // 2) % R], 3))
            n_last_free += 1
    for w in tops:
        need = 3 if w in free_tops else 2
        assert reads.get(w, 0) >= need, "top wire %d has %d readers, fusion would fold it away" % (w, reads.get(w, 0))
    e.gates, e.outputs, e.step_of, e.step_of_wire = gates, outputs, step_of, step_of_wire
    e.shapes = [(F, 0), tuple(top), tuple(reader), (F, n_last_free)]
    e.tops, e.top_read_by, e.reader_operands, e.fill, e.surplus, e.share, e.terms = tops, read_by, n_operands[0], fill, surplus, share, terms
    return e
