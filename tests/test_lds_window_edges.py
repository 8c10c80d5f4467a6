"""The LDS label window at the edges of each instance's share, against a reference that knows nothing of slots.

run_program_kernel (csrc/engine/kernels.hip) keeps short-lived wires in a window of GSV_LDS_SLOTS entries in LDS (limits.h); with 2 or 4
instances per workgroup every instance has a half or a quarter of it, and nothing but address arithmetic (`win_base`, `bit_base`,
WireFile::win / win_word / win_bit) separates the regions: entry share - 1 of instance g lies 16 bytes below entry 0 of instance g + 1 —
the all-zero label that every ABSENT operand of a fused record names —, the last label entry of the last instance directly below
plaintext bit 0 of instance 0 (the bit absent operands read when evaluating), the last plaintext bit of the last instance directly
below the round keys.  Real circuits fill a share only inside the large units, where the inputs decide which entry is touched and a
failure names nothing.  Here small synthetic programs (tests/lds_window_lib.py; Program.from_gates, ONE image per share: window_div) are
built so that the compiled image has `n_lds_slots == share` exactly, in four steps: FILL wires that hold entries 1 .. share - 1 - T to
the last step; a TOP step whose T outputs take exactly the remaining entries, the last of them entry share - 1; a READER step whose
every operand field (a1 a2 b1 b2 p / a1 .. a4 b1 .. b4 p / x1 .. x4) names a top wire, beside records with ABSENT operands — which read
entry 0, label and bit, after the neighbours' top entries were written —, its outputs pinned and compared; a LAST step that reads the
fill wires together with reader outputs, window and wire-file operands in one record.  One family of programs per (share, record form):
the top and reader steps of its members are of the lane-mapping classes through which entry share - 1 is written and read by every
access path — 16-byte st / ld of a whole one-gate-per-lane AND pass, of a narrow step's free lanes and of a free-gate phase of more than
one batch; 4-byte st_word / ld_word of the multi-lane forms (eight lanes, four lanes, and the four-lane x2 form when a four-wire
program is garbled); 1-byte st_bit / ld_bit of the plaintext bits when evaluating — the shapes taken from the kernel's quantities as
tests/test_kernel_step_shapes.py restates them.  An OVERFULL member per family has a few top outputs more than there are free entries:
the window is still exactly full, the surplus goes to the wire file in the same step (one wave stores to both), the reader reads both.

  * CPU half (default non-GPU set): for every image the record form, the exact (AND, free) step sequence, the class of the top and reader
    steps in the instantiation that will run them, n_lds_slots == share, the top step's window writes (and wire-file writes of the
    surplus), the reader step's window reads == its operand fields with no wire-file read (both kinds when overfull), and that every
    top wire is read by a record of the kind the member is about; per family, that the classes cover every access path; one entry too
    many still compiles, spills and keeps n_lds_slots == share.  A compiler change that voids the coverage fails here.  With it: the
    host interpreter (tests/hostsim) now sizes its window image by the share the image was compiled for and refuses, naming the slot, a
    record that names an entry at or above it (or any window entry in a program compiled without a window); every image here is
    interpreted under it against the reference (SimProgram.from_gates), and the random circuits and fq_mul are held to the oracle under
    it with the window capped to a half, a quarter and nothing.
  * GPU half: every image at `GSV_INSTANCES_PER_WG` = its window_div — every instance's share exactly full — for a ragged batch of
    2 d + 1 distinct seeds (full workgroups and one with idle groups) and, at four per workgroup, for exactly four (all four shares and
    both ends of the bit window in use in one workgroup); garbled, then evaluated from the garbler's stream; per instance the whole
    ciphertext stream, the CBC-MAC, the output label0s, the active labels, the plaintext bits and active == select(label0, bit)
    against tests/gate_list_ref.py, bit for bit.  A failure names the share, the record form, the step and its class and the instance's
    position in its workgroup: the instance that fails is the NEIGHBOUR of the one that overran.  One member per share also runs
    with BLAKE3 (one instance per workgroup, one gate per lane); one two-wire and one four-wire member compiled with GSV_LDS_SLOTS=0 —
    every wire and the absent operands' zero slot in the wire file — run at 1 and 4 per workgroup with replays = 2 and chained
    feedback: the zero label and the zero bit must survive the feedback epilogue.

Not covered on purpose: plan (window) launches of these images — the window addressing is the same code, and tests/test_plan_small.py
runs quarter-window images through every session kind; the partly filled one-gate-per-lane pass as the writer of the last entry — it
stores through the same 16-byte path as a whole pass, and tests/test_kernel_step_shapes.py sweeps it.
"""
import contextlib

import numpy as np
import pytest

import gate_list_ref as G
import lds_window_lib as W
import oracle_lib as o
import test_kernel_step_shapes as S

NAMES = ["pass", "narrow_free", "wide_free", "multi", "quarter"]
OVERFULL = {2: "narrow_free", 4: "multi"}  # the family member that also exists with SURPLUS more top outputs, per record form
FAMILY = [(d, terms, name, 0) for terms in (2, 4) for d in W.DIVS for name in NAMES] + [(d, terms, OVERFULL[terms], W.SURPLUS) for terms in (2, 4) for d in W.DIVS]
BLAKE3_MEMBER = {1: "wide_free", 2: "pass", 4: "narrow_free"}  # share -> the member that also runs with BLAKE3
ALL_HBM = {2: "pass", 4: "quarter"}  # record form -> the full-window member that is also compiled with GSV_LDS_SLOTS=0
SEED0 = 1300  # instance i of every batch has seed SEED0 + i: a program's reference for a seed is computed once per test session

_built = {}


@contextlib.contextmanager
def compile_env(terms, no_window=False):
    """The compile knobs of a family member while it is compiled (read by the entry point that compiles, kept with the program)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GSV_AND_TERMS", str(terms))
        mp.delenv("GSV_LDS_SLOTS_CAP", raising=False)
        if no_window:
            mp.setenv("GSV_LDS_SLOTS", "0")
        else:
            mp.delenv("GSV_LDS_SLOTS", raising=False)
        yield


def member(d, terms, name, surplus=0):
    """(Edge, Program — ONE image for a share of WINDOW / d entries) of a family member, built once per process."""
    import garbled_snark_verifier_amd as gsv
    key = (d, terms, name, surplus)
    if key not in _built:
        top, reader = W.variants(d, terms)[name]
        e = W.build(W.WINDOW // d, terms, top, reader, surplus)
        with compile_env(terms):
            _built[key] = (e, gsv.Program.from_gates(W.N_INPUTS, e.gates, e.outputs, window_div=d if d > 1 else None))
    return _built[key]


def all_hbm_member(terms):
    """(Edge, Program compiled with GSV_LDS_SLOTS=0 and the feedback output i -> input i, feedback pairs) of the full-window member."""
    import garbled_snark_verifier_amd as gsv
    key = ("hbm", terms)
    if key not in _built:
        top, reader = W.variants(1, terms)[ALL_HBM[terms]]
        e = W.build(W.WINDOW, terms, top, reader)
        pairs = [(i, i) for i in range(W.N_INPUTS)]
        with compile_env(terms, no_window=True):
            _built[key] = (e, gsv.Program.from_gates(W.N_INPUTS, e.gates, e.outputs, feedback=pairs), pairs)
    return _built[key]


def _stats(prog):
    return [[int(v) for v in row] for row in prog.step_stats()]


_refs = {}


def _reference(key, e, seed, hasher, replays=1, pairs=None):
    """Per (program, seed, hasher), computed once: delta, consts, inputs, bits and the reference's garbling and evaluation — for
    replays > 1 run after run with the inputs re-wired by hand through `pairs` (gate ids continue across replays)."""
    k = (key, seed, hasher, replays)
    if k not in _refs:
        import garbled_snark_verifier_amd as gsv
        d, f, t, inp = gsv.labels_from_seed(seed, W.N_INPUTS)
        consts = np.stack([f, t])
        bits = np.random.default_rng(seed).integers(0, 2, W.N_INPUTS).astype(np.uint8)
        act = np.where(bits[:, None] == 1, inp ^ d[None, :], inp)
        ca = np.stack([consts[0], consts[1] ^ d])
        o.set_hasher(hasher)
        try:
            lab0, a, b, stream = inp.copy(), act.copy(), bits.copy(), []
            for r in range(replays):
                g = G.garble(e.gates, d, consts, lab0, e.outputs, gate_id_base=r * len(e.gates))
                ev = G.evaluate(e.gates, ca, a, b, g.ciphertexts, e.outputs, gate_id_base=r * len(e.gates))
                stream.append(g.ciphertexts)
                if pairs:  # the feedback epilogue: output src -> input dst (the outputs themselves stay: they are what is read back)
                    lab0, a, b = lab0.copy(), a.copy(), b.copy()
                    for src, dst in pairs:
                        lab0[dst], a[dst], b[dst] = g.output_label0[src], ev.output_active[src], ev.output_bits[src]
        finally:
            o.set_hasher("aes")
        cts = np.concatenate(stream)
        _refs[k] = dict(delta=d, consts=consts, inputs=inp, bits=bits, active=act, consts_active=ca, cts=cts, mac=o.cbcmac(cts),
                        label0=g.output_label0, out_active=ev.output_active, out_bits=ev.output_bits)
    return _refs[k]


# ---- CPU half --------------------------------------------------------------------------------------------------------------------------------
def test_window_constants_are_the_kernels():
    """limits.h as this module reads it: the shares divide the window, and the bit window ends where the round keys begin."""
    assert all(W.WINDOW % d == 0 for d in W.DIVS)
    assert all(W.WINDOW // d - 3 > S.XOR_BATCH * (S.BLOCK_THREADS // d) + 1 for d in W.DIVS)  # more than one free-gate batch fits every share
    assert "GSV_LDS_RK_BASE (GSV_LDS_TABLE_BYTES + GSV_LDS_SLOTS * 16u + GSV_LDS_SLOTS)" in W._LIMITS


@pytest.mark.parametrize("d,terms,name,surplus", FAMILY)
def test_image_fills_its_share_exactly(d, terms, name, surplus):
    e, prog = member(d, terms, name, surplus)
    share, info, stats = W.WINDOW // d, prog.info, _stats(prog)
    top, reader = e.shapes[1], e.shapes[2]
    assert info["and_terms"] == terms
    assert info["n_steps"] == 4 and [tuple(r[:2]) for r in stats] == e.shapes, "the compiled steps are not the intended (and_cnt, xor_cnt) sequence"
    assert info["n_gates"] == len(e.gates) < 17_000 and info["n_dead"] == sum(1 for g in e.gates if g[3] is None) > 0
    want = W.expected_classes(d, terms, name)
    for evaluate in (False, True):
        L = S.Lanes(d, evaluate, terms)
        assert (S.classify(L, *top), S.classify(L, *reader)) == want[evaluate], "evaluate" if evaluate else "garble"
    assert info["n_lds_slots"] == share
    T = top[0] + top[1] - surplus
    assert len(e.fill) == share - 1 - T and len(e.tops) == T + surplus
    # fill: every output into the window; top: exactly the remaining entries, the surplus (only then) into the wire file
    assert stats[0][4:] == [len(e.fill), 0] and stats[1][4:] == [T, surplus] and stats[1][3] == 0
    # reader: every operand field that names a wire names a top wire; all of them in the window unless the top step spilled
    assert stats[2][2] + stats[2][3] == e.reader_operands and stats[2][4:] == [0, reader[0] + reader[1]]
    assert (stats[2][3] == 0) if surplus == 0 else (stats[2][2] > 0 and stats[2][3] >= surplus)
    # last: window operands (the fill wires, each held to this step) and wire-file operands (reader outputs) in every record
    assert stats[3][2] >= len(e.fill) and stats[3][3] >= len(e.fill) and stats[3][4] == 0
    # every top wire is read by a record of the kind the member is about (so the one in entry share - 1 is, whichever it is)
    kind = "free" if name in ("narrow_free", "wide_free") else "and"
    assert all(kind in e.top_read_by[w] for w in e.tops) and all(e.top_read_by[w] for w in e.tops)


@pytest.mark.parametrize("d", W.DIVS)
@pytest.mark.parametrize("terms", [2, 4])
def test_family_covers_every_access_path(d, terms):
    """Across the members of a family, entry share - 1 is written and read once through each path of the table in the module docstring."""
    written, read = {False: set(), True: set()}, {False: set(), True: set()}
    for name in NAMES:
        e, prog = member(d, terms, name)
        for evaluate in (False, True):
            L = S.Lanes(d, evaluate, terms)
            top, reader = e.shapes[1], e.shapes[2]
            wa, wx = W.access_paths(L, S.classify(L, *top), top)
            # records get their entries in record order, AND-family first: the last entry is the last free record's if there is one
            written[evaluate].add(wx if wx else wa)
            ra, rx = W.access_paths(L, S.classify(L, *reader), reader)
            covered = set.intersection(*(e.top_read_by[w] for w in e.tops))  # record kinds that read EVERY top wire
            assert covered
            read[evaluate] |= {p for p, k in ((ra, "and"), (rx, "free")) if k in covered and p}
    for evaluate in (False, True):
        L = S.Lanes(d, evaluate, terms)
        need = {"lane16", ("free16", "narrow"), ("free16", "batches"), ("word", L.LPG, "x1")}
        if L.dual:
            need.add(("word", L.LPG2, "x2"))
        assert need <= written[evaluate], (evaluate, need - written[evaluate])
        assert need <= read[evaluate], (evaluate, need - read[evaluate])
    assert S.Lanes(d, False, 4).dual and not S.Lanes(d, True, 4).dual and not S.Lanes(d, False, 2).dual  # x2: garbling four-wire programs only


@pytest.mark.parametrize("d", W.DIVS)
@pytest.mark.parametrize("terms", [2, 4])
def test_one_entry_too_many_spills_and_keeps_the_share(d, terms):
    """The same top step with ONE output more than there are free entries: it compiles, that one output goes to the wire file, the
    window is exactly full and no entry past the share is handed out."""
    import garbled_snark_verifier_amd as gsv
    top, reader = W.variants(d, terms)[OVERFULL[terms]]
    e = W.build(W.WINDOW // d, terms, top, reader, surplus=1)
    with compile_env(terms):
        prog = gsv.Program.from_gates(W.N_INPUTS, e.gates, e.outputs, window_div=d if d > 1 else None)
    stats = _stats(prog)
    assert [tuple(r[:2]) for r in stats] == e.shapes and prog.info["n_lds_slots"] == W.WINDOW // d
    assert stats[1][4:] == [top[0] + top[1] - 1, 1] and stats[2][3] >= 1 and stats[2][2] + stats[2][3] == e.reader_operands


@pytest.mark.parametrize("terms", [2, 4])
def test_all_hbm_image_has_no_window_access(terms):
    e, prog, pairs = all_hbm_member(terms)
    info, stats = prog.info, _stats(prog)
    assert info["and_terms"] == terms and [tuple(r[:2]) for r in stats] == e.shapes
    assert info["n_lds_slots"] == info["reads_lds"] == info["writes_lds"] == 0 and all(r[2] == r[4] == 0 for r in stats)
    # absent operands name the wire file's zero slot: they count as wire-file reads, so every operand FIELD of the reader step is one
    fields = (5 if terms == 2 else 9) * e.shapes[2][0] + 4 * e.shapes[2][1]
    assert stats[2][3] == fields > e.reader_operands
    assert len(pairs) == W.N_INPUTS and all(e.step_of_wire[e.outputs[a]] == 2 for a, _ in pairs)  # reader outputs are fed back to the inputs


def test_builder_reference_round_trip_on_the_cpu():
    """The builder's gate lists are well formed for the reference and its evaluator recovers select(label0, bit) from its garbler's
    stream on one — at a toy share, both record forms' lists, an overfull one."""
    for terms, surplus in ((2, 0), (4, 3)):
        e = W.build(80, terms, (10, 7), (9, 11), surplus)
        labs = o.chacha_labels(5, 3 + W.N_INPUTS)
        delta, consts, inputs = labs[0], labs[1:3], labs[3:]
        g = G.garble(e.gates, delta, consts, inputs, e.outputs)
        bits = np.random.default_rng(terms).integers(0, 2, W.N_INPUTS).astype(np.uint8)
        act = np.where(bits[:, None] == 1, inputs ^ delta[None, :], inputs)
        ev = G.evaluate(e.gates, (consts[0], consts[1] ^ delta), act, bits, g.ciphertexts, e.outputs)
        assert (ev.output_active == np.where(ev.output_bits[:, None] == 1, g.output_label0 ^ delta[None, :], g.output_label0)).all()
        assert ev.n_consumed == g.n_ciphertexts == sum(a for a, _ in e.shapes) and g.n_dead > 0
        assert 0 < ev.output_bits.sum() < len(e.outputs)


def _interpret_and_compare(sp, prog, key, e, replays=1, pairs=None):
    """The image under tests/hostsim (one instance, its window image as large as the share it was compiled for) == the reference."""
    assert [sp.info[k] for k in ("n_steps", "n_lds_slots", "reads_lds", "reads_hbm", "writes_lds", "writes_hbm", "n_slots")] == \
           [prog.info[k] for k in ("n_steps", "n_lds_slots", "reads_lds", "reads_hbm", "writes_lds", "writes_hbm", "n_slots")], "the interpreter compiled another image"
    r = _reference(key, e, SEED0, "aes", replays, pairs)
    out, cts = sp.garble(r["delta"], r["consts"], r["inputs"], replays=replays)
    assert (cts == r["cts"]).all() and (out == r["label0"]).all()
    oa, ob = sp.evaluate(r["consts_active"], r["active"], r["bits"], cts, replays=replays)
    assert (ob == r["out_bits"]).all() and (oa == r["out_active"]).all()
    assert (oa == np.where(ob[:, None] == 1, out ^ r["delta"][None, :], out)).all() and 0 < int(ob.sum()) < len(ob)


@pytest.mark.parametrize("d,terms,name,surplus", FAMILY)
def test_image_interprets_to_the_reference_inside_its_share(d, terms, name, surplus):
    """Before anything runs on a device: the image is correct and names no window entry at or above its share (the interpreter refuses
    one, by name) — the reference computed here is the GPU half's for the first instance."""
    import hostsim_lib as h
    e, prog = member(d, terms, name, surplus)
    with compile_env(terms):
        sp = h.SimProgram.from_gates(W.N_INPUTS, e.gates, e.outputs, window_div=d if d > 1 else None)
    _interpret_and_compare(sp, prog, (d, terms, name, surplus), e)


@pytest.mark.parametrize("terms", [2, 4])
def test_all_hbm_image_interprets_to_the_reference_with_chained_replays(terms):
    import hostsim_lib as h
    e, prog, pairs = all_hbm_member(terms)
    with compile_env(terms, no_window=True):
        sp = h.SimProgram.from_gates(W.N_INPUTS, e.gates, e.outputs, feedback=pairs)
    _interpret_and_compare(sp, prog, ("hbm", terms), e, replays=2, pairs=pairs)
    one = _reference(("hbm", terms), e, SEED0, "aes")
    two = _reference(("hbm", terms), e, SEED0, "aes", 2, pairs)
    n = len(one["cts"])
    assert (two["cts"][:n] == one["cts"]).all() and (two["label0"] != one["label0"]).any()  # the feedback changes the second replay


@pytest.mark.parametrize("spec,seed", [("random_circuit:0", 0), ("random_circuit:1", 1), ("random_circuit:2", 2), ("random_circuit:3", 3), ("fq_mul", 1)])
@pytest.mark.parametrize("knob,slots", [("GSV_LDS_SLOTS_CAP", W.WINDOW // 4), ("GSV_LDS_SLOTS_CAP", W.WINDOW // 2), ("GSV_LDS_SLOTS", 0)])
def test_capped_images_stay_inside_their_window_under_the_interpreter(monkeypatch, knob, slots, spec, seed):
    """tests/hostsim sizes its window image by the share the image was compiled for and refuses a record that names an entry at or
    above it: a capped image that interprets to the oracle's ciphertexts, labels and bits has stayed inside its share."""
    import test_engine_host as EH
    monkeypatch.setenv(knob, str(slots))
    sp = EH._hostsim_check(spec, seed)
    assert sp.info["n_lds_slots"] <= slots
    if slots == 0:
        assert sp.info["reads_lds"] == sp.info["writes_lds"] == 0
    elif spec == "fq_mul":
        assert sp.info["n_lds_slots"] == slots and sp.info["writes_hbm"] > 0  # the window is contended: the bound is reached


# ---- GPU half --------------------------------------------------------------------------------------------------------------------------------
def _where_ct(e, ni, terms, hasher, index, evaluate=False):
    """Gate, step, shape and class of ciphertext `index` of one replay's stream."""
    k = -1
    for i, g in enumerate(e.gates):
        if g[3] is not None and g[0] < 8:
            k += 1
            if k == index:
                return "gate %d, %s" % (i, _step_name(e, ni, terms, hasher, e.step_of[i], evaluate))
    return "?"


def _step_name(e, ni, terms, hasher, step, evaluate):
    L = S.Lanes(ni, evaluate, terms, blake3=hasher == "blake3")
    return "step %d (%s) with (and_cnt, xor_cnt) = %s, class %r when %s" % (step, ("fill", "top", "reader", "last")[step], e.shapes[step], S.classify(L, *e.shapes[step]),
                                                                           "evaluating" if evaluate else "garbling")


def _run_and_compare(engine, monkeypatch, key, e, prog, what, ni, terms, n_instances, hasher="aes", replays=1, pairs=None):
    import garbled_snark_verifier_amd as gsv
    monkeypatch.setenv("GSV_AND_TERMS", str(terms))
    monkeypatch.setenv("GSV_INSTANCES_PER_WG", str(ni))
    seeds = [SEED0 + i for i in range(n_instances)]
    B = len(seeds)
    refs = [_reference(key, e, s, hasher, replays, pairs) for s in seeds]
    stack = lambda name: np.stack([r[name] for r in refs])
    sess = gsv.Session(engine, prog, B, replays)
    assert sess.instances_per_workgroup == ni
    sess.set_hasher(hasher)
    sess.set_garble_inputs(stack("delta"), stack("consts"), stack("inputs"))
    sess.garble(0)
    sess.sync()
    out0 = sess.read_outputs()
    cts = [sess.read_ciphertexts(i) for i in range(B)]
    macs = [sess.ciphertext_hash(i) for i in range(B)]
    sess.close()
    ev = gsv.Session(engine, prog, B, replays)
    ev.set_hasher(hasher)
    ev.set_evaluate_inputs(stack("consts_active"), stack("active"), stack("bits"))
    for i in range(B):
        ev.upload_ciphertexts(i, cts[i])
    ev.evaluate(0)
    ev.sync()
    act_out, bit_out = ev.read_outputs(with_bits=True)
    ev.close()
    launched = 1 if hasher == "blake3" else ni
    n_ct = len(refs[0]["cts"]) // replays
    for i, r in enumerate(refs):
        w = "%s, %s, instance %d of %d (seed %d) = workgroup %d, position %d of %d" % (what, hasher, i, B, seeds[i], i // launched, i % launched, launched)
        assert cts[i].shape == r["cts"].shape, w
        bad = np.nonzero((cts[i] != r["cts"]).any(axis=1))[0]
        assert bad.size == 0, "%s: %d ciphertexts differ, the first at stream index %d (replay %d): %s" % (
            w, bad.size, bad[0], bad[0] // n_ct, _where_ct(e, launched, terms, hasher, int(bad[0]) % n_ct))
        assert macs[i] == r["mac"], w + ": CBC-MAC"
        for name, got, ref_name, evaluate in (("output label0s", out0[i], "label0", False), ("active labels", act_out[i], "out_active", True)):
            bad = np.nonzero((got != r[ref_name]).any(axis=1))[0]
            assert bad.size == 0, "%s: %d %s differ, the first: output %d (wire %d), written by %s" % (
                w, bad.size, name, bad[0], e.outputs[bad[0]], _step_name(e, launched, terms, hasher, e.step_of_wire[e.outputs[bad[0]]], evaluate))
        bad = np.nonzero(bit_out[i] != r["out_bits"])[0]
        assert bad.size == 0, "%s: %d plaintext bits differ, the first: output %d (wire %d), written by %s" % (
            w, bad.size, bad[0], e.outputs[bad[0]], _step_name(e, launched, terms, hasher, e.step_of_wire[e.outputs[bad[0]]], True))
        assert (act_out[i] == np.where(bit_out[i][:, None] == 1, out0[i] ^ r["delta"][None, :], out0[i])).all(), w + ": active label != select(label0, bit)"


def _what(d, terms, name, surplus):
    return "share %d (1/%d of the window), %d-wire records, member %s%s" % (W.WINDOW // d, d, terms, name, " with %d top outputs too many" % surplus if surplus else "")


@pytest.mark.gpu
@pytest.mark.parametrize("d,terms,name,surplus", FAMILY)
def test_full_shares_on_the_device(engine, monkeypatch, d, terms, name, surplus):
    """A ragged batch of 2 d + 1 instances with distinct seeds at d per workgroup: full workgroups and one with idle groups, every
    instance's share exactly full."""
    e, prog = member(d, terms, name, surplus)
    assert prog.info["n_lds_slots"] == W.WINDOW // d
    _run_and_compare(engine, monkeypatch, (d, terms, name, surplus), e, prog, _what(d, terms, name, surplus), d, terms, 2 * d + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("d,terms,name,surplus", [m for m in FAMILY if m[0] == 4])
def test_four_full_shares_in_one_workgroup(engine, monkeypatch, d, terms, name, surplus):
    """Exactly four instances at four per workgroup: all four shares, and both ends of the bit window, are in use in ONE workgroup."""
    e, prog = member(d, terms, name, surplus)
    assert prog.info["n_lds_slots"] == W.WINDOW // 4
    _run_and_compare(engine, monkeypatch, (d, terms, name, surplus), e, prog, _what(d, terms, name, surplus), 4, terms, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("d", W.DIVS)
def test_full_share_with_the_blake3_hasher(engine, monkeypatch, d):
    """HASH = 1: one instance per workgroup and one gate per lane in every step, the image's share (whole, half, quarter) exactly full."""
    e, prog = member(d, 2, BLAKE3_MEMBER[d])
    L = S.Lanes(1, False, 2, blake3=True)
    assert all(S.classify(L, *s)[0] == "wide" and S.classify(L, *s)[2] in (None, "partial") for s in e.shapes)
    _run_and_compare(engine, monkeypatch, (d, 2, BLAKE3_MEMBER[d], 0), e, prog, _what(d, 2, BLAKE3_MEMBER[d], 0), 1, 2, 3, hasher="blake3")


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 4])
@pytest.mark.parametrize("terms", [2, 4])
def test_all_hbm_image_with_chained_replays_on_the_device(engine, monkeypatch, terms, ni):
    """GSV_LDS_SLOTS=0: every wire, and the zero slot that absent operands name, in the wire file; replays = 2 with the reader outputs
    fed back to the inputs — the second replay reads the zero label and the zero bit after the feedback epilogue ran."""
    e, prog, pairs = all_hbm_member(terms)
    _run_and_compare(engine, monkeypatch, ("hbm", terms), e, prog, "no LDS window (GSV_LDS_SLOTS=0), %d-wire records, member %s, replays = 2" % (terms, ALL_HBM[terms]),
                     ni, terms, 2 * ni + 1, replays=2, pairs=pairs)
