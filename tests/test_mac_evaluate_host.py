"""sharding.evaluate_from(checkpoint_dir=) without a GPU, through the stand-in evaluator: the up-front check — each checkpoint file's
last state against the record's hash — runs on the host, and the stand-in may raise CiphertextMismatch itself.  Modelled on
test_blake3_evaluate.test_evaluate_from_with_blake3_records_through_the_stand_in; the references are the CPU oracle and the host
writer gsv.cbcmac_file_checkpoints."""
import os

import numpy as np
import pytest


def _case(tmp_path, circuit="u254_add", seed=5, k=4):
    import garbled_snark_verifier_amd as gsv
    import oracle_lib as o
    from garbled_snark_verifier_amd import sharding
    d = str(tmp_path)
    g = o.garble(circuit, seed)
    gc = os.path.join(d, gsv.gc_file_name(0))
    gsv.write_gc_file(gc, g.ciphertexts)
    mac = gsv.cbcmac_file_checkpoints(gc, k, os.path.join(d, gsv.checkpoint_file_name(0)))
    assert mac == g.ct_hash.tobytes()
    table = np.stack([sharding.commit_record(0, mac, g.output_label0, g.delta, g.false_label0, g.true_label0, g.input_label0)])
    n_in, n_out = g.input_label0.shape[0], g.output_label0.shape[0]
    bits = np.random.default_rng(1).integers(0, 2, n_in).astype(np.uint8)
    case = {"index": 0, "true_constant_wire": g.true_label0 ^ g.delta, "false_constant_wire": g.false_label0,
            "input_active": np.where(bits[:, None] == 1, g.input_label0 ^ g.delta[None, :], g.input_label0), "input_bits": bits}
    ob, _, _ = o.execute(circuit, bits)
    act = np.where(ob[:, None] == 1, g.output_label0 ^ g.delta[None, :], g.output_label0)
    return dict(d=d, g=g, mac=mac, table=table, case=case, n_out=n_out, act=act, ob=ob, circuit=circuit, k=k)


def test_evaluate_from_with_checkpoints_through_the_stand_in(tmp_path):
    import garbled_snark_verifier_amd as gsv
    from garbled_snark_verifier_amd import sharding
    c = _case(tmp_path)
    called = []

    def stand_in(index, t, f, a, b):
        called.append(index)
        return c["act"], c["ob"], c["mac"]

    run = lambda **kw: sharding.evaluate_from(c["table"], [c["case"]], c["circuit"], c["d"], c["n_out"], evaluate=stand_in, **kw)  # noqa: E731
    res = run(checkpoint_dir=c["d"])
    assert [r[0] for r in res] == [0] and (res[0][2] == c["ob"]).all() and called == [0]
    with pytest.raises(ValueError):
        run(checkpoint_dir=c["d"], commitment="blake3")  # the files hold the states of the CBC-MAC
    # the up-front check: the last state flipped, a truncated file, no file — before the stand-in is called
    ck = os.path.join(c["d"], gsv.checkpoint_file_name(0))
    clean = open(ck, "rb").read()
    for bad in (clean[:-1] + bytes([clean[-1] ^ 1]), clean[:-16], b"x" + clean[1:], None):
        del called[:]
        if bad is None:
            os.remove(ck)
        else:
            open(ck, "wb").write(bad)
        with pytest.raises(sharding.ConsistencyError) as ei:
            run(checkpoint_dir=c["d"])
        assert (ei.value.kind, ei.value.index) == ("CiphertextMismatch", 0) and not called
    open(ck, "wb").write(clean)
    # an inner state flipped passes the up-front check: the evaluator finds it, here the stand-in with the host checker's group
    inner = bytearray(clean)
    inner[24 + 16 * 2 + 5] ^= 0x20
    open(ck, "wb").write(bytes(inner))
    group = gsv.cbcmac_file_check(os.path.join(c["d"], gsv.gc_file_name(0)), ck)[1]
    assert group == 2

    def finds_it(index, t, f, a, b):
        raise gsv.CiphertextMismatch("gsv status 5: stand-in", 0, group, group << c["k"])

    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(c["table"], [c["case"]], c["circuit"], c["d"], c["n_out"], evaluate=finds_it, checkpoint_dir=c["d"])
    assert (ei.value.kind, ei.value.index) == ("CiphertextMismatch", 0) and "group" in str(ei.value) and str(group << c["k"]) in str(ei.value)
    open(ck, "wb").write(clean)
    # the checks that need no evaluation run first: a wrong input label of the case is reported, not the bad checkpoint file
    open(ck, "wb").write(clean[:-1] + bytes([clean[-1] ^ 1]))
    wrong = dict(c["case"], input_active=c["case"]["input_active"] ^ np.uint8(1))
    with pytest.raises(sharding.ConsistencyError) as ei:
        sharding.evaluate_from(c["table"], [wrong], c["circuit"], c["d"], c["n_out"], evaluate=stand_in, checkpoint_dir=c["d"])
    assert ei.value.kind == "InputLabelsMismatch"
