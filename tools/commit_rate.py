#!/usr/bin/env python3
"""What a commitment costs: whole verifier passes with the ciphertexts discarded, drained into the host's CBC-MACs, and hashed on the
device with BLAKE3 (DESIGN.md §3 "Commitment stage", §6), and the stand-alone rate of the BLAKE3 kernels.

    python tools/commit_rate.py [--instances 64,1024] [--rounds 2] [--kernel-gib 1] [--out profiles/commit_blake3]
    python tools/commit_rate.py --evaluator [--resident-instances 4] [--evaluate-instances 16] [--out profiles/commit_blake3]
    python tools/commit_rate.py --receive [--rounds 3] [--evaluate-instances 16] [--parent-so <the parent commit's libgsv_engine.so> [--parent-all-legs]] [--out profiles/verified_receive]
    python tools/commit_rate.py --receive --slices [--rounds 3] [--parent-so <the parent commit's libgsv_engine.so>] --out profiles/eval_slices

The driver touches no GPU.  Every GPU step is a child process of this file under its own `timeout`:
  kernel   gsv.blake3_streams on 16 streams of --kernel-gib GiB each, one segment: device seconds from the first hash kernel to the last
           (gsv_engine_blake3_streams_seconds), one digest compared with the host hasher's;
  check    the 16 instances of tests/golden/cc16_verifier_golden.json with commitment="both": every CBC-MAC equals the oracle's fixture in
           the very pass that produced the BLAKE3 digests, which the rounds below must reproduce for their first 16 instances;
  file     ONE instance (the fixture's first seed) in a pass of its own with commitment="blake3" and its stream written to gc_0.bin: the
           device's digest equals gsv.blake3_file of that file (47.7 GB through the host hasher) and the digest of the check pass;
  round    one batch size, warm (a discarded pass first), then the three legs in turn: discard, CBC-MAC drain, device BLAKE3 — `--rounds`
           children per batch size, so the legs alternate; GSV_DRAIN_STATS lines of the draining legs go to the log.
  resident (--evaluator) a retained fq_mul program session of --resident-instances instances x --kernel-gib GiB of stream (one launch range
           each by default): device seconds of Session.ciphertext_blake3() — the stream hashed in place through the position table
           (gsv_engine_blake3_streams_seconds) — one digest compared with the host hasher's over read_ciphertexts; then, for the same
           shape, the gather-then-hash cost of the drain: garble_streaming(commitment="blake3") minus garble_streaming(discard=True);
  evaluate (--evaluator) fq12_mix, --batch instances: gc files written by a garbling pass, then evaluate_streaming with
           commitment="cbcmac" and "blake3" in turn: wall seconds and host CPU seconds (user + system of the process) per pass;
           digests and MACs equal the garbler's.
  receive  (--receive) the receiving side, fq12_mix, --evaluate-instances instances: gc files and outboards written once by a garbling pass,
           then --rounds times, alternating, the parent library's evaluate_streaming(commitment="blake3") (--parent-so: the yardstick of
           the verified mode) and this library's legs — blake3_file over all files on the host, blake3_files on the device with and
           without outboards, evaluate_streaming unverified and verified: wall and host CPU seconds per leg, into <out>/receive_rate.{json,log}.
--evaluator runs these two only (the evaluator's and the resident halves), into <out>/evaluator_rate.{json,log}.
A child that fails, is killed at its time limit or dies ends the run: nothing more is started on the GPU.  At most 16 host threads
(--threads) serve a drain.  Results: <out>/commit_rate.json and <out>/commit_rate.log.  Batches run in ascending order; one whose CBC-MAC
leg — the plan's ciphertext bytes at the link rate the previous batch's CBC-MAC leg measured — cannot end within --leg-seconds is not
started and the JSON says so.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _child_setup():
    import threading
    t0 = time.time()

    def alive():  # a CBC-MAC leg of a large batch is minutes of silence: a line a minute shows the child is running
        while True:
            time.sleep(60)
            print("commit_rate: running, %.0f s" % (time.time() - t0), file=sys.stderr, flush=True)
    threading.Thread(target=alive, daemon=True).start()
    import numpy as np
    import bench_support as bs
    import garbled_snark_verifier_amd as gsv
    return np, bs, gsv, gsv.Engine(0)


def _load_plan(bs, gsv, eng, log):
    case = json.load(open(os.path.join(ROOT, "tests", "golden", bs.FIXTURE["verifier_compressed"])))
    args = argparse.Namespace(no_plan_cache=False, plan_cache=None)
    plan, info, _ = bs.get_plan(gsv, eng, args, case["circuit"], bs.VERIFIER_UNITS + ["fp254::exp_chunk"], 0, 0, 1, bs.Dist(1, None, None), log)
    log("plan %s in %.1f s" % (info.get("how"), info["seconds"]))
    return case, plan


def child_kernel(a):
    np, bs, gsv, eng = _child_setup()
    records = (a.kernel_gib << 30) // 16
    data = np.empty((16, records, 16), np.uint8)
    block = np.random.default_rng(1).integers(0, 256, (1 << 20, 16), dtype=np.uint8)
    for s in range(16):
        for off in range(0, records, 1 << 20):
            n = min(1 << 20, records - off)
            data[s, off:off + n] = block[:n] ^ np.uint8(s + 1)
    secs, digests = [], None
    for _ in range(11):
        digests, sec = gsv.blake3_streams(eng, data, [records], with_seconds=True)
        secs.append(sec)
    secs = sorted(secs[1:])  # (the first call also allocates)
    med = secs[len(secs) // 2]
    ok = digests[5] == gsv.blake3(data[5])
    print(json.dumps({"step": "kernel", "streams": 16, "gib_per_stream": a.kernel_gib, "calls": len(secs), "device_seconds_median": med, "device_seconds_min": secs[0], "device_seconds_max": secs[-1],
                      "bytes_per_s": data.size / med, "ciphertexts_per_s": data.size / 16 / med, "digest_matches_host_hasher": ok, "read_pattern": "one lane per chunk"}), flush=True)
    return 0 if ok else 1


def _work(np, bs, gsv, eng, plan, B, gold):
    seeds = [int(s) for s in gold["seeds"][:min(B, 16)]] + bs.instance_seeds(0, B)[:max(0, B - 16)]
    return bs.VerifierWork(gsv, eng, plan, B, seeds)


def child_check(a):
    np, bs, gsv, eng = _child_setup()
    log = lambda m: print("commit_rate: " + m, file=sys.stderr, flush=True)  # noqa: E731
    case, plan = _load_plan(bs, gsv, eng, log)
    gold = bs.cc16_verifier_fixture(case)
    w = _work(np, bs, gsv, eng, plan, 16, gold)
    w.new_pass()
    t0 = time.perf_counter()
    macs, digests = w.sess.garble_streaming(threads=a.threads, commitment="both")
    dt = time.perf_counter() - t0
    ok = [macs[i].hex() == gold["ct_hashes"][i] for i in range(16)]
    w.close()
    print(json.dumps({"step": "check", "instances": 16, "seconds": dt, "ciphertexts_per_instance": plan.info["n_ciphertexts"], "cbcmacs_equal_to_the_oracle_fixture": sum(ok), "blake3_digests": [d.hex() for d in digests]}), flush=True)
    return 0 if all(ok) else 1


def child_file(a):
    import shutil
    import tempfile
    np, bs, gsv, eng = _child_setup()
    log = lambda m: print("commit_rate: " + m, file=sys.stderr, flush=True)  # noqa: E731
    case, plan = _load_plan(bs, gsv, eng, log)
    gold = bs.cc16_verifier_fixture(case)
    need = plan.info["n_ciphertexts"] * 16
    roots = [d for d in ("/dev/shm", tempfile.gettempdir()) if os.path.isdir(d) and os.statvfs(d).f_bavail * os.statvfs(d).f_frsize > 1.25 * need]
    if not roots:
        print(json.dumps({"step": "file", "skipped": "no directory with room for a %.1f GB gc file" % (need / 1e9)}), flush=True)
        return 0
    d = tempfile.mkdtemp(prefix="gsv_commit_rate_", dir=roots[0])
    try:
        w = _work(np, bs, gsv, eng, plan, 1, gold)
        w.new_pass()
        t0 = time.perf_counter()
        digest = w.sess.garble_streaming(directory=d, threads=a.threads, commitment="blake3")[0]
        t1 = time.perf_counter()
        w.close()
        path = os.path.join(d, gsv.gc_file_name(0))
        size = os.path.getsize(path)
        file_digest = gsv.blake3_file(path)
        t2 = time.perf_counter()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    ok = digest == file_digest and size == need
    print(json.dumps({"step": "file", "instances": 1, "file_bytes": size, "pass_seconds": t1 - t0, "host_hash_seconds": t2 - t1, "host_hash_bytes_per_s": size / (t2 - t1),
                      "device_digest": digest.hex(), "blake3_file_digest": file_digest.hex(), "equal": ok}), flush=True)
    return 0 if ok else 1


def child_round(a):
    np, bs, gsv, eng = _child_setup()
    log = lambda m: print("commit_rate: " + m, file=sys.stderr, flush=True)  # noqa: E731
    case, plan = _load_plan(bs, gsv, eng, log)
    gold = bs.cc16_verifier_fixture(case)
    B, gates, n_ct = a.batch, plan.info["n_gates"], plan.info["n_ciphertexts"]
    w = _work(np, bs, gsv, eng, plan, B, gold)
    si = w.sess.schedule_info()
    out = {"step": "round", "instances": B, "gates_per_instance": gates, "ciphertexts_per_instance": n_ct, "windows": si["n_windows"], "segments": si["n_segments"],
           "segment_ct_records": si["segment_ct_records"], "instances_per_workgroup": w.sess.instances_per_workgroup, "legs": {}}
    w.run_pass()  # warm: first launches, allocations
    os.environ["GSV_DRAIN_STATS"] = "1"  # (read per pass: where the drain's host thread waited goes to the log, one line per draining leg)
    for leg in ("discard", "cbcmac", "blake3"):
        w.new_pass()
        t0 = time.perf_counter()
        if leg == "discard":
            w.sess.garble_streaming(discard=True)
        elif leg == "cbcmac":
            macs = w.sess.garble_streaming(threads=a.threads)
        else:
            digests = w.sess.garble_streaming(threads=a.threads, commitment="blake3")
        dt = time.perf_counter() - t0
        out["legs"][leg] = {"seconds": dt, "gates_per_s": gates * B / dt, "ciphertexts_per_s": n_ct * B / dt}
        log("%d instances, %s: %.2f s, %.3e gates/s" % (B, leg, dt, gates * B / dt))
    out["cbcmacs_equal_to_the_oracle_fixture"] = sum(macs[i].hex() == gold["ct_hashes"][i] for i in range(min(B, 16)))
    out["blake3_digests_first16"] = [d.hex() for d in digests[:16]]
    out["distinct_blake3_digests"] = len(set(digests))
    w.close()
    print(json.dumps(out), flush=True)
    return 0 if out["cbcmacs_equal_to_the_oracle_fixture"] == min(B, 16) else 1


def _median(v):
    return sorted(v)[len(v) // 2]


def child_resident(a):
    np, bs, gsv, eng = _child_setup()
    prog = gsv.Program.from_circuit("fq_mul")
    n_ct, n_in, B = prog.info["n_ciphertexts"], prog.info["n_inputs"], a.resident_instances
    replays = -(-((a.kernel_gib << 30) // 16) // n_ct)
    labs = [gsv.labels_from_seed(s, n_in) for s in range(1, B + 1)]
    inputs = (np.stack([x[0] for x in labs]), np.stack([np.stack([x[1], x[2]]) for x in labs]), np.stack([x[3] for x in labs]))
    sess = gsv.Session(eng, prog, B, replays)
    sess.set_garble_inputs(*inputs)
    sess.garble()
    sess.sync()
    secs, digests = [], None
    for _ in range(7):
        digests, sec = sess.ciphertext_blake3(with_seconds=True)
        secs.append(sec)
    secs = sorted(secs[1:])  # (the first call also allocates)
    ok = digests[B - 1] == gsv.blake3(sess.read_ciphertexts(B - 1))
    sess.close()
    stream_bytes = B * replays * n_ct * 16
    # the drain's way for the same shape: the whole stream is one segment, gathered into a gate-order buffer and hashed there
    drain = gsv.Session(eng, prog, B, replays)
    drain.set_garble_inputs(*inputs)
    drain.garble_streaming(discard=True)  # warm
    legs = {"discard": [], "blake3": []}
    drained = None
    for _ in range(3):
        for leg in ("discard", "blake3"):
            drain.set_garble_inputs(*inputs)
            t0 = time.perf_counter()
            if leg == "discard":
                drain.garble_streaming(discard=True)
            else:
                drained = drain.garble_streaming(commitment="blake3")
            legs[leg].append(time.perf_counter() - t0)
    drain.close()
    ok = ok and drained == digests
    med = _median(secs)
    print(json.dumps({"step": "resident", "circuit": "fq_mul", "instances": B, "replays": replays, "ciphertexts_per_replay": n_ct, "stream_bytes": stream_bytes, 
                      "engine_library": os.environ.get("GSV_ENGINE_SO", "default"), "in_place_device_seconds": secs, "in_place_device_seconds_median": med, "in_place_bytes_per_s": stream_bytes / med,
                      "drain_discard_seconds": legs["discard"], "drain_blake3_seconds": legs["blake3"], "gather_then_hash_seconds_median": _median(legs["blake3"]) - _median(legs["discard"]),
                      "digests_equal_host_hasher_and_drain": ok}), flush=True)
    return 0 if ok else 1


def child_evaluate(a):
    import resource
    import shutil
    import tempfile
    np, bs, gsv, eng = _child_setup()
    plan = gsv.Plan.from_circuit("fq12_mix", ["fq12::mul_montgomery", "fq12::square_montgomery"])
    B, n_in, n_ct = a.batch, plan.info["n_inputs"], plan.info["n_ciphertexts"]
    need = B * n_ct * 16
    roots = [d for d in ("/dev/shm", tempfile.gettempdir()) if os.path.isdir(d) and os.statvfs(d).f_bavail * os.statvfs(d).f_frsize > 1.25 * need]
    if not roots:
        print(json.dumps({"step": "evaluate", "skipped": "no directory with room for %.1f GB of gc files" % (need / 1e9)}), flush=True)
        return 0
    labs = [gsv.labels_from_seed(s, n_in) for s in range(1, B + 1)]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([np.stack([x[1], x[2]]) for x in labs]); inputs = np.stack([x[3] for x in labs])
    bits = np.random.default_rng(1).integers(0, 2, (B, n_in)).astype(np.uint8)
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    d = tempfile.mkdtemp(prefix="gsv_commit_rate_", dir=roots[0])
    try:
        g = gsv.Session(eng, plan, B, retain_stream=False)
        g.set_garble_inputs(delta, consts, inputs)
        macs, digests = g.garble_streaming(directory=d, threads=a.threads, commitment="both")
        out0 = g.read_outputs()
        g.close()
        ev = gsv.Session(eng, plan, B, retain_stream=False)

        def leg(commitment):
            ev.set_evaluate_inputs(consts_active, active, bits)
            r0, t0 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
            got = ev.evaluate_streaming(d, commitment=commitment)
            dt, r1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_SELF)
            return got, dt, (r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime)

        ok = leg("both")[0] == (macs, digests)  # warm
        legs = {"cbcmac": {"wall_seconds": [], "cpu_seconds": []}, "blake3": {"wall_seconds": [], "cpu_seconds": []}}
        for _ in range(a.rounds + 1):
            for c in ("cbcmac", "blake3"):
                got, dt, cpu = leg(c)
                ok = ok and got == (macs if c == "cbcmac" else digests)
                legs[c]["wall_seconds"].append(dt); legs[c]["cpu_seconds"].append(cpu)
        act, ob = ev.read_outputs(with_bits=True)
        ok = ok and bool((act == np.where(ob[:, :, None] == 1, out0 ^ delta[:, None, :], out0)).all())
        ev.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for v in legs.values():
        v["wall_seconds_median"], v["cpu_seconds_median"] = _median(v["wall_seconds"]), _median(v["cpu_seconds"])
    print(json.dumps({"step": "evaluate", "circuit": "fq12_mix", "instances": B, "ciphertexts_per_instance": n_ct, "file_bytes": need, "files_in": roots[0], "legs": legs,
                      "commitments_equal_the_garblers_and_outputs_select": ok}), flush=True)
    return 0 if ok else 1


def _receive_case(np, gsv, B):
    plan = gsv.Plan.from_circuit("fq12_mix", ["fq12::mul_montgomery", "fq12::square_montgomery"])
    n_in = plan.info["n_inputs"]
    labs = [gsv.labels_from_seed(s, n_in) for s in range(1, B + 1)]
    delta = np.stack([x[0] for x in labs]); consts = np.stack([np.stack([x[1], x[2]]) for x in labs]); inputs = np.stack([x[3] for x in labs])
    bits = np.random.default_rng(1).integers(0, 2, (B, n_in)).astype(np.uint8)
    return plan, delta, consts, inputs, bits


def child_receive_files(a):
    """--receive: the gc files and outboards every leg reads, written once into --dir by a garbling pass of this library."""
    np, bs, gsv, eng = _child_setup()
    B = a.batch
    plan, delta, consts, inputs, _ = _receive_case(np, gsv, B)
    g = gsv.Session(eng, plan, B, retain_stream=False)
    g.set_garble_inputs(delta, consts, inputs)
    t0 = time.perf_counter()
    digests = g.garble_streaming(directory=a.dir, threads=a.threads, commitment="blake3", outboard_dir=a.dir)
    dt = time.perf_counter() - t0
    np.save(os.path.join(a.dir, "out0.npy"), g.read_outputs())
    g.close()
    json.dump([x.hex() for x in digests], open(os.path.join(a.dir, "digests.json"), "w"))
    sizes = [os.path.getsize(os.path.join(a.dir, gsv.outboard_file_name(i))) for i in range(B)]
    same = all(open(os.path.join(a.dir, gsv.outboard_file_name(i)), "rb").read() == _host_outboard(gsv, a.dir, i) for i in (0, B - 1))
    print(json.dumps({"step": "receive_files", "circuit": "fq12_mix", "instances": B, "ciphertexts_per_instance": plan.info["n_ciphertexts"], "file_bytes": B * plan.info["n_ciphertexts"] * 16,
                      "outboard_bytes_per_instance": sizes[0], "garble_seconds": dt, "files_in": a.dir, "outboards_equal_the_host_writers": same}), flush=True)
    return 0 if same else 1


def _host_outboard(gsv, d, i):
    path = os.path.join(d, "host_%d.b3o" % i)
    gsv.blake3_file_outboard(os.path.join(d, gsv.gc_file_name(i)), 10, path)
    data = open(path, "rb").read()
    os.remove(path)
    return data


def child_receive_legs(a):
    """--receive: one round of the legs over the files in --dir, each after a warm run of its own: the host loop (blake3_file over all
    files), blake3_files on the device with and without outboards, evaluate_streaming(commitment="blake3") unverified and verified.
    With the parent commit's library (--parent-so) the unverified evaluation alone runs (the yardstick of the verified mode), or, with
    --parent-all-legs (a parent that has every entry point: a refactor's yardstick), all of them."""
    import ctypes
    import resource
    parent = os.environ.get("GSV_RECEIVE_PARENT")  # "1": the yardstick leg alone, "all": every leg (set by the driver, with GSV_ENGINE_SO naming that library)
    if parent in ("1", "slices"):
        # the parent's library lacks the entry points this change adds: they get a stand-in that is never called
        import garbled_snark_verifier_amd as g0

        class _Missing:
            argtypes = restype = None

        class _Compat:
            def __init__(self, so):
                self._l = ctypes.CDLL(so)

            def __getattr__(self, name):
                try:
                    return getattr(self._l, name)
                except AttributeError:
                    return _Missing()
        g0.C = type("C", (), dict(vars(ctypes), CDLL=_Compat))
    np, bs, gsv, eng = _child_setup()
    B = a.batch
    plan, delta, consts, inputs, bits = _receive_case(np, gsv, B)
    active = np.where(bits[:, :, None] == 1, inputs ^ delta[:, None, :], inputs)
    consts_active = np.stack([consts[:, 0], consts[:, 1] ^ delta], axis=1)
    digests = [bytes.fromhex(x) for x in json.load(open(os.path.join(a.dir, "digests.json")))]
    out0 = np.load(os.path.join(a.dir, "out0.npy"))
    files = [os.path.join(a.dir, gsv.gc_file_name(i)) for i in range(B)]
    obs = [os.path.join(a.dir, "gc_%d.b3o" % i) for i in range(B)]
    # (--slices: explicit launch windows of an eighth of the stream for every leg and both libraries — the default schedule of this shape is one window, and a slice is made of whole windows)
    ev = gsv.Session(eng, plan, B, retain_stream=False, **({"window_ct_records": plan.info["n_ciphertexts"] // 8} if a.slices else {}))

    def evaluate(**kw):
        ev.set_evaluate_inputs(consts_active, active, bits)
        return ev.evaluate_streaming(a.dir, commitment="blake3", **kw)

    def evaluate_sliced(restartable):
        """one window of the schedule per slice, verified (Session.evaluate_calls)"""
        ev.set_evaluate_inputs(consts_active, active, bits)
        got = None
        for first, n, _ in ev.windows():
            got = ev.evaluate_calls(first, n, directory=a.dir, commitment="blake3", outboard_dir=a.dir, expected=digests, restartable=restartable)
        return got

    legs = {"evaluate_unverified": lambda: evaluate()}
    if a.slices:
        # --slices: the verified evaluation unsliced (the parent's library: the baseline; this one: the thin caller) and, with this
        # library, in slices of one window without and with restart points
        legs = {"evaluate_verified": lambda: evaluate(outboard_dir=a.dir, expected=digests)}
        if not parent:
            legs.update({"evaluate_verified_sliced": lambda: evaluate_sliced(False), "evaluate_verified_sliced_restartable": lambda: evaluate_sliced(True)})
    elif parent != "1":
        legs = {"host_blake3_file": lambda: [gsv.blake3_file(f) for f in files],
                "device_blake3_files_outboards": lambda: gsv.blake3_files(eng, files, obs),
                "device_blake3_files": lambda: gsv.blake3_files(eng, files),
                "evaluate_unverified": lambda: evaluate(),
                "evaluate_verified": lambda: evaluate(outboard_dir=a.dir, expected=digests)}
    out, ok = {}, True
    for name, run in legs.items():
        if name != "host_blake3_file":
            ok = ok and run() == digests  # warm: first launches, allocations, the page cache
        r0, t0 = resource.getrusage(resource.RUSAGE_SELF), time.perf_counter()
        got = run()
        dt, r1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_SELF)
        ok = ok and got == digests
        out[name] = {"wall_seconds": dt, "cpu_seconds": (r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime)}
        if name.startswith("evaluate"):
            act, ob = ev.read_outputs(with_bits=True)
            ok = ok and bool((act == np.where(ob[:, :, None] == 1, out0 ^ delta[:, None, :], out0)).all())
    info = ev.schedule_info()
    ev.close()
    print(json.dumps({"step": "receive_legs", "library": "parent" if parent else "this", "instances": B, "file_bytes": sum(os.path.getsize(f) for f in files), "legs": out,
                      "n_windows": info["n_windows"], "wire_file_slots": info["wire_file_slots"],
                      "restart_point_bytes": 2 * B * info["wire_file_slots"] * 17,  # two copies of every wire file: labels and plaintext bits
                      "digests_equal_the_garblers_and_outputs_select": ok}), flush=True)
    return 0 if ok else 1


def driver_receive(a):
    """--receive: the files once, then --rounds times the parent library's unverified evaluation (with --parent-so) and this library's
    legs, alternating; medians, and for the evaluator the parent's own run-to-run spread, go to <out>/receive_rate.json."""
    import shutil
    import tempfile
    os.makedirs(a.out, exist_ok=True)
    log_f = open(os.path.join(a.out, "receive_rate.log"), "w")
    root = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="gsv_receive_rate_", dir=root)
    results, stopped = [], None

    def step(name, seconds, env=None):
        nonlocal stopped
        if stopped:
            return None
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.relpath(os.path.abspath(__file__), ROOT), "--child", name, "--threads", str(a.threads), "--batch", str(a.evaluate_instances), "--dir", d]
        if a.slices:
            cmd.append("--slices")
        log_f.write("$ " + " ".join(["python"] + cmd[5:]) + (" (parent library)" if env else "") + "\n"); log_f.flush()
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=log_f, text=True, cwd=ROOT, env=dict(os.environ, **(env or {})))
        log_f.write(p.stdout); log_f.flush()
        results.extend(json.loads(l) for l in p.stdout.splitlines() if l.startswith("{"))
        if p.returncode != 0:
            stopped = "%s ended with status %d: nothing more was started" % (name, p.returncode)

    try:
        step("receive_files", 600)
        for _ in range(a.rounds):
            if a.parent_so:
                step("receive_legs", 600 if a.parent_all_legs else 300, {"GSV_ENGINE_SO": os.path.abspath(a.parent_so), "GSV_RECEIVE_PARENT": "slices" if a.slices else "all" if a.parent_all_legs else "1"})
            step("receive_legs", 600)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    summary = {}
    for r in results:
        if r.get("step") == "receive_legs":
            for k, v in r["legs"].items():
                s = summary.setdefault(r["library"] + ":" + k, {"wall_seconds": [], "cpu_seconds": []})
                s["wall_seconds"].append(v["wall_seconds"]); s["cpu_seconds"].append(v["cpu_seconds"])
    n_bytes = next((r["file_bytes"] for r in results if r.get("step") == "receive_files"), 0)
    for s in summary.values():
        s["wall_seconds_median"], s["cpu_seconds_median"] = _median(s["wall_seconds"]), _median(s["cpu_seconds"])
        s["wall_seconds_spread"] = max(s["wall_seconds"]) - min(s["wall_seconds"])
        s["bytes_per_s_median"] = n_bytes / s["wall_seconds_median"] if s["wall_seconds_median"] else None
    json.dump({"results": results, "summary": summary, "stopped": stopped}, open(os.path.join(a.out, "receive_rate.json"), "w"), indent=1)
    print(json.dumps({"summary": summary, "stopped": stopped}))
    return 1 if stopped else 0


def driver(a):
    if a.receive:
        return driver_receive(a)
    os.makedirs(a.out, exist_ok=True)
    log_f = open(os.path.join(a.out, "evaluator_rate.log" if a.evaluator else "commit_rate.log"), "w")
    results, stopped = [], None

    def step(name, seconds, extra):
        nonlocal stopped
        if stopped:
            return None
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.relpath(os.path.abspath(__file__), ROOT), "--child", name, "--threads", str(a.threads), "--kernel-gib", str(a.kernel_gib),
               "--resident-instances", str(a.resident_instances), "--rounds", str(a.rounds)] + extra
        log_f.write("$ " + " ".join(["python"] + cmd[5:]) + "\n"); log_f.flush()
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=log_f, text=True, cwd=ROOT)
        log_f.write(p.stdout); log_f.flush()
        rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0:
            stopped = "%s %s ended with status %d: nothing more was started" % (name, " ".join(extra), p.returncode)
        results.extend(rows)
        save()
        return rows[0] if rows else None

    def save():
        summary = {}
        for r in results:
            if r.get("step") == "round" and "legs" in r:
                s = summary.setdefault(str(r["instances"]), {k: [] for k in r["legs"]})
                for k, v in r["legs"].items():
                    s[k].append(v["gates_per_s"])
        json.dump({"results": results, "gates_per_s_by_instances": summary, "stopped": stopped}, open(os.path.join(a.out, "evaluator_rate.json" if a.evaluator else "commit_rate.json"), "w"), indent=1)
        return summary

    if a.evaluator:
        step("resident", 600, [])
        step("evaluate", 600, ["--batch", str(a.evaluate_instances)])
        save()
        print(json.dumps({"results": results, "stopped": stopped}))
        return 1 if stopped else 0
    step("kernel", 300, [])
    check = step("check", a.leg_seconds, [])
    if not a.no_file_check:
        f = step("file", a.leg_seconds, [])
        if f and check and "device_digest" in f and f["device_digest"] != check["blake3_digests"][0]:
            stopped = stopped or "the digest of the file pass differs from the checked pass"
    link_bytes_per_s = None  # what the last CBC-MAC leg moved: a larger batch cannot be faster than that
    for B in sorted(a.instances):
        if link_bytes_per_s and check:
            need_s = B * check["ciphertexts_per_instance"] * 16 / link_bytes_per_s
            if need_s > 0.8 * a.leg_seconds:
                results.append({"step": "round", "instances": B, "skipped": "its CBC-MAC leg alone needs %.0f s (%d ciphertexts per instance at the %.1f GB/s the previous batch's CBC-MAC leg moved): beyond --leg-seconds %d"
                                % (need_s, check["ciphertexts_per_instance"], link_bytes_per_s / 1e9, a.leg_seconds)})
                continue
        for _ in range(a.rounds):
            r = step("round", a.leg_seconds, ["--batch", str(B)])
            if r and "legs" in r:
                link_bytes_per_s = r["legs"]["cbcmac"]["ciphertexts_per_s"] * 16
            if r and check and r["blake3_digests_first16"] != check["blake3_digests"][:len(r["blake3_digests_first16"])]:
                stopped = stopped or "the BLAKE3 digests of a round differ from the checked pass"
    summary = save()
    print(json.dumps({"gates_per_s_by_instances": summary, "kernel": next((r for r in results if r.get("step") == "kernel"), None), "stopped": stopped}))
    return 1 if stopped else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=lambda s: [int(x) for x in s.split(",")], default=[64, 1024])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--kernel-gib", type=int, default=1)
    ap.add_argument("--leg-seconds", type=int, default=1500)  # a 1 024-instance round: ~900 s of CBC-MAC leg alone
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commit_blake3"))
    ap.add_argument("--no-file-check", action="store_true")
    ap.add_argument("--evaluator", action="store_true")
    ap.add_argument("--resident-instances", type=int, default=4)
    ap.add_argument("--evaluate-instances", type=int, default=16)
    ap.add_argument("--receive", action="store_true")
    ap.add_argument("--slices", action="store_true")
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--parent-all-legs", action="store_true")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child", choices=["kernel", "check", "round", "file", "resident", "evaluate", "receive_files", "receive_legs"])
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    a.threads = max(1, min(16, a.threads))
    sys.exit({"kernel": child_kernel, "check": child_check, "round": child_round, "file": child_file, "resident": child_resident, "evaluate": child_evaluate, "receive_files": child_receive_files,
              "receive_legs": child_receive_legs, None: driver}[a.child](a))
