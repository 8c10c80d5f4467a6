"""records/s of Session.ciphertext_cbcmac_check (the resident stream verified where it lies) on fq12_mul, 64 instances, k = 8 and 12, three
rounds each behind a warm call, wall clock around the call (opening the checkpoint files included); beside it Session.ciphertext_hash of one
instance on the same session: the fetch-and-fold it replaces.  Prints one JSON line (profiles/mac_evaluate/resident_rate.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import garbled_snark_verifier_amd as gsv

eng = gsv.Engine(0)
prog = gsv.Program.from_circuit("fq12_mul")
n_in, n_ct = prog.info["n_inputs"], prog.info["n_ciphertexts"]
B = 64
labs = [gsv.labels_from_seed(100 + i, n_in) for i in range(B)]
sess = gsv.Session(eng, prog, B)
sess.set_garble_inputs(np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
sess.garble(); sess.sync()
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
out = {"circuit": "fq12_mul", "instances": B, "records_per_instance": n_ct, "rounds": []}
t0 = time.time(); h0 = sess.ciphertext_hash(0); t_hash = time.time() - t0
out["ciphertext_hash_one_instance_s"] = t_hash
out["ciphertext_hash_records_per_s"] = n_ct / t_hash
for k in (8, 12):
    for i in range(B):
        p = os.path.join(d, gsv.gc_file_name(i))
        gsv.write_gc_file(p, sess.read_ciphertexts(i))
        mac = gsv.cbcmac_file_checkpoints(p, k, os.path.join(d, gsv.checkpoint_file_name(i)))
        os.remove(p)
        if i == 0:
            assert mac == h0
    sess.ciphertext_cbcmac_check(d)  # warm
    for rnd in range(3):
        t0 = time.time(); macs = sess.ciphertext_cbcmac_check(d); dt = time.time() - t0
        assert macs[0] == h0
        out["rounds"].append({"k": k, "seconds_wall": dt, "records_per_s": B * n_ct / dt})
print(json.dumps(out))
