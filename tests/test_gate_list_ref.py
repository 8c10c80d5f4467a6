"""tests/gate_list_ref.py (the plain-Python gate-list garbler / evaluator the kernel step-shape tests compare the device with) pinned to
the CPU oracle on circuits the oracle knows: fed the raw gate stream the product's recorder sees (hostsim_lib.trace), it must reproduce
oracle_lib.garble and oracle_lib.evaluate exactly — ciphertexts, CBC-MAC, output labels, active labels and bits.  With a non-zero
gate_id_base no named oracle entry point exists: there it is compared with the host interpreter's gid_base (tests/hostsim), which
computes its tweaks in 64-bit host arithmetic, and with the oracle's own per-gate primitive."""
import numpy as np
import pytest

import gate_list_ref as G
import hostsim_lib as h
import oracle_lib as o

SPECS = ["driver_mix", "random_circuit:3"] + ["gate:%d" % t for t in range(11)]


def _traced(spec):
    t, a, b, c, ins, outs = h.trace(spec)
    return G.gates_of_trace(t, a, b, c), ins.tolist(), outs.tolist()


@pytest.mark.parametrize("spec", SPECS)
def test_gate_list_ref_reproduces_the_oracle_on_traced_circuits(spec):
    gates, ins, outs = _traced(spec)
    for seed in (7, 2**40 + 3):
        ref = o.garble(spec, seed)
        assert int(ref.gate_counts.sum()) == len(gates)
        g = G.garble(gates, ref.delta, (ref.false_label0, ref.true_label0), ref.input_label0, outs, input_wires=ins)
        assert g.n_ciphertexts == ref.n_ciphertexts and (g.ciphertexts == ref.ciphertexts).all()
        assert g.ct_hash == ref.ct_hash.tobytes()
        assert (g.output_label0 == ref.output_label0).all()
        n_in = len(ins)
        all_bits = [[x >> k & 1 for k in range(n_in)] for x in range(1 << n_in)] if n_in <= 2 else np.random.default_rng(seed).integers(0, 2, (2, n_in)).tolist()
        for bits in all_bits:
            bits = np.array(bits, np.uint8)
            act = np.where(bits[:, None] == 1, ref.input_label0 ^ ref.delta[None, :], ref.input_label0)
            ta, fa = ref.true_label0 ^ ref.delta, ref.false_label0
            e = G.evaluate(gates, (fa, ta), act, bits, ref.ciphertexts, outs, input_wires=ins)
            oe = o.evaluate(spec, ta.tobytes(), fa.tobytes(), act, bits, ref.ciphertexts)
            ob, _, _ = o.execute(spec, bits)
            assert (e.output_bits == oe.output_bits).all() and (e.output_bits == ob).all()
            assert (e.output_active == oe.output_active).all()
            assert (e.output_active == np.where(ob[:, None] == 1, ref.output_label0 ^ ref.delta[None, :], ref.output_label0)).all()
            assert e.n_consumed == oe.n_consumed and e.ct_hash == oe.ct_hash.tobytes() == g.ct_hash


def test_buffered_primitives_equal_the_oracle_wrappers():
    rng = np.random.default_rng(1)
    for k in range(200):
        a, b, d, ct = (rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(4))
        t, gid = k % 11, int(rng.integers(0, 2**63)) if k % 3 else k
        assert G.garble_gate(t, a, b, d, gid) == o.garble_gate(t, a, b, d, gid)
        for av in (0, 1):
            assert G.degarble_gate(t, ct, a, av, b, gid) == o.degarble_gate(t, ct, a, av, b, gid)


def test_gate_f_is_the_oracles_truth_table():
    for t in range(11):
        spec = "gate:%d" % t
        for a in (0, 1):
            for b in (0, 1):
                ob, _, _ = o.execute(spec, np.array([a, b], np.uint8))
                assert int(ob[0]) == G.gate_f(t, a, b)


@pytest.mark.parametrize("base", [1, 2**32 - 300, 2**32 + 12345, 2**55 + 987654321])
def test_gate_list_ref_gate_id_base_equals_the_host_interpreters(base):
    """gate i has id gate_id_base + i: the reference (64-bit Python integers handed to the oracle's garble_gate) against the host
    interpreter run with gid_base (program.hpp's records carry the index inside the replay, the interpreter adds the base in uint64_t) —
    on driver_mix (dead gates, constants) and a random circuit long enough for the carry out of the low 32 bits to land inside it."""
    for spec, seed in (("driver_mix", 5), ("random_circuit:3", 6)):
        gates, ins, outs = _traced(spec)
        sp = h.SimProgram(spec)
        labs = h.labels_from_seed(seed, 3 + len(ins))
        delta, consts, inputs = labs[0], labs[1:3], labs[3:]
        out, cts = sp.garble(delta, consts, inputs, gid_base=base)
        g = G.garble(gates, delta, consts, inputs, outs, gate_id_base=base, input_wires=ins)
        assert (g.ciphertexts == cts).all() and (g.output_label0 == out).all() and g.ct_hash == h.cbcmac(cts)
        assert g.n_ciphertexts == 0 or not (g.ciphertexts == G.garble(gates, delta, consts, inputs, outs, input_wires=ins).ciphertexts).all()
        bits = np.random.default_rng(seed).integers(0, 2, len(ins)).astype(np.uint8)
        act = np.where(bits[:, None] == 1, inputs ^ delta[None, :], inputs)
        ca = np.stack([consts[0], consts[1] ^ delta])
        oa, ob = sp.evaluate(ca, act, bits, cts, gid_base=base)
        e = G.evaluate(gates, ca, act, bits, cts, outs, gate_id_base=base, input_wires=ins)
        assert (e.output_active == oa).all() and (e.output_bits == ob).all()
        assert (e.output_active == np.where(ob[:, None] == 1, out ^ delta[None, :], out)).all()
