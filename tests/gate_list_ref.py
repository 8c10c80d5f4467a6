"""Gate-list reference garbler / evaluator (TEST INFRASTRUCTURE, CPU only).

Garbles and evaluates an EXPLICIT gate list gate by gate in plain Python, the way GarbleMode / EvaluateMode walk a stream
(garble_mode.rs:160-222, evaluate_mode.rs:123-158): gate i of the list has id gate_id_base + i, a dead gate (c is None / 0xFFFFFFFF)
consumes its id and nothing else, constants contribute their label0.  The only cryptography it touches are the oracle's level-0
primitives — oracle_lib.garble_gate, degarble_gate and cbcmac (known-answer tested in tests/test_oracle_kat.py; the two per-gate ones
are called through reused buffers, garble_gate / degarble_gate below: the wrappers in oracle_lib allocate five arrays per call, 21 us
against 2 us, and tests/test_gate_list_ref.py holds the two paths equal); free gates follow the oracle's alpha table
(gsv_oracle.cpp garble_gate / degarble_gate: Xor c0 = a0 ^ b0, Xnor c0 = a0 ^ b0 ^ delta, Not c0 = a0 ^ delta; the evaluator's active
label of a free gate is a ^ b, of a Not a).  It knows nothing of steps, lanes, records or fusion: it is the
reference for programs that no named oracle circuit describes (tests/test_kernel_step_shapes.py), and tests/test_gate_list_ref.py
pins it to oracle_lib.garble / evaluate on traced circuits the oracle does know.

Wire numbering is Program.from_gates': 0 / 1 the constants FALSE / TRUE, the inputs 2 .. 2 + n_inputs - 1 unless `input_wires` names
them (the SSA ids of hostsim_lib.trace), every other wire written once before it is read.
"""
import ctypes as C

import numpy as np

import oracle_lib as o

DEAD = 0xFFFFFFFF
XOR, XNOR, NOT = 8, 9, 10


def gate_f(t, a, b):
    """Plaintext function of gate type t (core/gate_type.rs): AND-family ((a ^ alpha_a) & (b ^ alpha_b)) ^ alpha_c with
    alpha_a, alpha_b, alpha_c = bits 2, 1, 0 of the type; Xor, Xnor, Not."""
    if t < 8:
        return (((a ^ (t >> 2)) & (b ^ (t >> 1))) ^ t) & 1
    return (a ^ b) & 1 if t == XOR else (a ^ b ^ 1) & 1 if t == XNOR else (a ^ 1) & 1


def _i(label):
    return int.from_bytes(bytes(label), "little")


def _b(v):
    return v.to_bytes(16, "little")


_bufs = [(C.c_char * 16)() for _ in range(5)]
_ptrs = [C.cast(x, C.POINTER(C.c_uint8)) for x in _bufs]


def garble_gate(t, a0, b0, delta, gate_id):
    """oracle_lib.garble_gate (gsvo_garble_gate) on 16-byte strings: (c0, ciphertext or None)."""
    _bufs[0].raw, _bufs[1].raw, _bufs[2].raw = a0, b0, delta
    has = o.lib().gsvo_garble_gate(t, _ptrs[0], _ptrs[1], _ptrs[2], gate_id, _ptrs[3], _ptrs[4])
    return _bufs[3].raw, (_bufs[4].raw if has else None)


def degarble_gate(t, ct, a, a_value, b, gate_id):
    """oracle_lib.degarble_gate (gsvo_degarble_gate) on 16-byte strings: the active output label."""
    _bufs[0].raw, _bufs[1].raw, _bufs[2].raw = ct, a, b
    o.lib().gsvo_degarble_gate(t, _ptrs[0], _ptrs[1], int(a_value), _ptrs[2], gate_id, _ptrs[3])
    return _bufs[3].raw


def _wires(n_inputs, input_wires):
    return list(range(2, 2 + n_inputs)) if input_wires is None else [int(w) for w in input_wires]


class GarbleRef:
    pass


def garble(gates, delta, consts, inputs, outputs, gate_id_base=0, input_wires=None):
    """gates: [(type, a, b, c-or-None)]; delta [16]; consts = (false_label0, true_label0); inputs [n_in,16] label0s; outputs: wire ids.
    Returns .ciphertexts [n_ct,16] in gate order, .ct_hash (CBC-MAC, bytes), .output_label0 [n_out,16], .n_gates, .n_dead."""
    d = _i(delta)
    lab = {0: _i(consts[0]), 1: _i(consts[1])}
    for w, l in zip(_wires(len(inputs), input_wires), inputs):
        lab[w] = _i(l)
    db = _b(d)
    cts = []
    n_dead = 0
    for i, (t, a, b, c) in enumerate(gates):
        a0, b0 = lab[a], lab[b if t != NOT else a]  # both operands are looked up before the id is taken (a Not names its operand twice)
        if c is None or c == DEAD:
            n_dead += 1
            continue
        if c in lab:
            raise ValueError("gate %d writes wire %d a second time" % (i, c))
        if t < 8:
            c0, ct = garble_gate(t, _b(a0), _b(b0), db, gate_id_base + i)
            cts.append(ct)
            lab[c] = _i(c0)
        else:
            lab[c] = a0 ^ b0 if t == XOR else a0 ^ b0 ^ d if t == XNOR else a0 ^ d
    r = GarbleRef()
    r.ciphertexts = np.frombuffer(b"".join(cts), np.uint8).reshape(-1, 16).copy()
    r.ct_hash = o.cbcmac(r.ciphertexts) if cts else bytes(16)
    r.output_label0 = np.frombuffer(b"".join(_b(lab[w]) for w in outputs), np.uint8).reshape(-1, 16).copy()
    r.n_gates, r.n_dead, r.n_ciphertexts = len(gates), n_dead, len(cts)
    return r


class EvalRef:
    pass


def evaluate(gates, consts_active, inputs_active, input_bits, ciphertexts, outputs, gate_id_base=0, input_wires=None):
    """consts_active = (false wire's active label = its label0, true wire's = its label1); inputs_active [n_in,16] with input_bits [n_in];
    ciphertexts [n_ct,16] consumed in gate order.  Returns .output_active [n_out,16], .output_bits [n_out], .ct_hash of what was
    consumed, .n_consumed."""
    lab = {0: (_i(consts_active[0]), 0), 1: (_i(consts_active[1]), 1)}
    for w, l, v in zip(_wires(len(inputs_active), input_wires), inputs_active, input_bits):
        lab[w] = (_i(l), int(v) & 1)
    cts = np.ascontiguousarray(ciphertexts, np.uint8).reshape(-1, 16)
    ct_bytes = cts.tobytes()
    k = 0
    for i, (t, a, b, c) in enumerate(gates):
        (la, va), (lb, vb) = lab[a], lab[b if t != NOT else a]
        if c is None or c == DEAD:
            continue
        if c in lab:
            raise ValueError("gate %d writes wire %d a second time" % (i, c))
        if t < 8:
            if k >= cts.shape[0]:
                raise ValueError("Ciphertext source exhausted at gate %d" % (gate_id_base + i))
            out = _i(degarble_gate(t, ct_bytes[16 * k:16 * k + 16], _b(la), va, _b(lb), gate_id_base + i))
            k += 1
        else:
            out = la if t == NOT else la ^ lb
        lab[c] = (out, gate_f(t, va, vb))
    r = EvalRef()
    r.output_active = np.frombuffer(b"".join(_b(lab[w][0]) for w in outputs), np.uint8).reshape(-1, 16).copy()
    r.output_bits = np.array([lab[w][1] for w in outputs], np.uint8)
    r.n_consumed = k
    r.ct_hash = o.cbcmac(cts[:k]) if k else bytes(16)
    return r


def gates_of_trace(t, a, b, c):
    """The arrays of hostsim_lib.trace as a gate list."""
    return [(int(tt), int(aa), int(bb), None if int(cc) == DEAD else int(cc)) for tt, aa, bb, cc in zip(t.tolist(), a.tolist(), b.tolist(), c.tolist())]
