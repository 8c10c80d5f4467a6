#!/usr/bin/env python3
"""The stand-alone rate of the CBC-MAC check kernel (DESIGN.md §3 "Commitment stage", §6): gsv.cbcmac_streams_check over --streams
streams that share one segment of --segment-gib GiB (a gate-order buffer of the drain holds ONE segment of every instance), one
segment per call, for each k of --ks — device seconds from the first check kernel to the last failing-group word
(gsv_engine_cbcmac_streams_check_seconds), in blocks/s and GB/s.

    python tools/mac_check_rate.py [--streams 8,256] [--ks 8,10,12,14,16] [--segment-gib 1] [--calls 7] [--out profiles/mac_check]
    python tools/mac_check_rate.py --whole-pass 64 [--rounds 1] [--threads 16] [--out profiles/mac_check]

The driver touches no GPU.  Every stream count is a child process of this file under its own `timeout`; a child that fails, is killed
at its time limit or dies ends the run: nothing more is started on the GPU.  Every stream of a child holds the same records (the
checkpoints are computed once on the host, by gsv.cbcmac_file_checkpoints); each call must find every group in order, and one call per
k with a flipped record must name its (stream, group).  Beside the rates the JSON carries the three numbers they are read against,
from the project's records: the T-table AES ceiling (1.14e11 blocks/s), the PCIe link (54 GB/s) and what the garbling of 256
instances produces (the stand-alone BLAKE3 rate 1.10e12 B/s / 3.4).  GSV_MAC_GROUP_LOG2's default is the largest k whose
rate at 256 streams is within 10 % of the best of the range.  Results: <out>/mac_check_rate.json and <out>/mac_check_rate.log.
--whole-pass B: one child, B instances of bench.py's verifier plan, warm (a discarded pass), then per round the three legs in turn on the
same session: garble_streaming drained into the host's CBC-MACs (it also writes the checkpoint files, k = GSV_MAC_GROUP_LOG2),
garble_check against those files (nothing drained; its commitments must equal the drained leg's), garble_streaming(commitment="blake3").
Results: <out>/whole_pass.json and <out>/whole_pass.log."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YARDSTICKS = {"aes_ceiling_blocks_per_s": 1.14e11, "pcie_bytes_per_s": 54e9, "production_256_instances_bytes_per_s": 1.10e12 / 3.4}


def child(a):
    import numpy as np
    import garbled_snark_verifier_amd as gsv
    eng = gsv.Engine(0)
    n_streams = a.child
    records = ((a.segment_gib << 30) // 16) // n_streams
    one = np.random.default_rng(3).integers(0, 256, (records, 16), dtype=np.uint8)
    data = np.ascontiguousarray(np.broadcast_to(one, (n_streams, records, 16)))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "s.bin")
        open(path, "wb").write(one.tobytes())
        for k in a.ks:
            gsv.cbcmac_file_checkpoints(path, k, os.path.join(td, "s.mck"))
            cks = [open(os.path.join(td, "s.mck"), "rb").read()] * n_streams
            secs, ok = [], True
            for _ in range(a.calls + 1):
                found, sec = gsv.cbcmac_streams_check(eng, data, [records], cks, with_seconds=True)
                ok = ok and found is None
                secs.append(sec)
            secs = sorted(secs[1:])  # (the first call also allocates)
            med = secs[len(secs) // 2]
            bad = data.copy()
            victim, r = n_streams // 2, records - 3
            bad[victim, r, 4] ^= 1
            named = gsv.cbcmac_streams_check(eng, bad, [records], cks) == (victim, r >> k)
            del bad
            print(json.dumps({"step": "rate", "streams": n_streams, "k": k, "records_per_stream": records, "chains_per_stream": -(-records // (1 << k)), "calls": len(secs),
                              "device_seconds_median": med, "device_seconds_min": secs[0], "device_seconds_max": secs[-1], "blocks_per_s": n_streams * records / med,
                              "bytes_per_s": n_streams * records * 16 / med, "intact_streams_pass": ok, "flipped_record_named": named, "read_pattern": "one lane per chain, 16 bytes per trip"}), flush=True)
            if not (ok and named):
                return 1
    return 0


def child_whole_pass(a):
    import argparse as ap
    import bench_support as bs
    import garbled_snark_verifier_amd as gsv
    log = lambda m: print("mac_check_rate: " + m, file=sys.stderr, flush=True)  # noqa: E731
    eng = gsv.Engine(0)
    case = json.load(open(os.path.join(ROOT, "tests", "golden", bs.FIXTURE["verifier_compressed"])))
    plan, info, _ = bs.get_plan(gsv, eng, ap.Namespace(no_plan_cache=False, plan_cache=None), case["circuit"], bs.VERIFIER_UNITS + ["fp254::exp_chunk"], 0, 0, 1, bs.Dist(1, None, None), log)
    log("plan %s in %.1f s" % (info.get("how"), info["seconds"]))
    B, gates, n_ct = a.whole_pass, plan.info["n_gates"], plan.info["n_ciphertexts"]
    w = bs.VerifierWork(gsv, eng, plan, B, bs.instance_seeds(0, B))
    si = w.sess.schedule_info()
    out = {"step": "whole_pass", "instances": B, "gates_per_instance": gates, "ciphertexts_per_instance": n_ct, "windows": si["n_windows"], "segments": si["n_segments"],
           "segment_ct_records": si["segment_ct_records"], "mac_group_log2": int(os.environ.get("GSV_MAC_GROUP_LOG2", "8")), "rounds": []}
    w.run_pass()  # warm: first launches, allocations
    os.environ["GSV_DRAIN_STATS"] = "1"
    ok = True
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        for _ in range(a.rounds):
            legs = {}
            for leg in ("cbcmac_drained", "cbcmac_check", "blake3"):
                w.new_pass()
                t0 = time.perf_counter()
                if leg == "cbcmac_drained":
                    macs = w.sess.garble_streaming(threads=a.threads, checkpoint_dir=td)
                elif leg == "cbcmac_check":
                    ok = ok and w.sess.garble_check(td, expected=macs) == macs
                else:
                    w.sess.garble_streaming(threads=a.threads, commitment="blake3")
                dt = time.perf_counter() - t0
                legs[leg] = {"seconds": dt, "gates_per_s": gates * B / dt, "ciphertexts_per_s": n_ct * B / dt}
                log("%d instances, %s: %.2f s, %.3e gates/s" % (B, leg, dt, gates * B / dt))
            out["rounds"].append(legs)
    out["check_returns_the_drained_commitments"] = ok
    out["fallbacks"] = w.sess.fallback_count()
    w.close()
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="8,256")
    ap.add_argument("--ks", default="8,10,12,14,16")
    ap.add_argument("--segment-gib", type=int, default=1)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--child-seconds", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mac_check"))
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--whole-pass", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--whole-pass-seconds", type=int, default=1100)
    a = ap.parse_args()
    a.ks = [int(x) for x in str(a.ks).split(",")]
    if a.child == -1:
        return child_whole_pass(a)
    if a.child:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    if a.whole_pass:
        cmd = ["timeout", "-k", "10", str(a.whole_pass_seconds), sys.executable, os.path.abspath(__file__), "--child", "-1", "--whole-pass", str(a.whole_pass), "--rounds", str(a.rounds), "--threads", str(a.threads)]
        t0 = time.time()
        with open(os.path.join(a.out, "whole_pass.log"), "w") as wl:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=wl, text=True)
            wl.write("(exit %d, %.1f s)\n" % (r.returncode, time.time() - t0))
        rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        json.dump({"whole_pass": rows, "exit": r.returncode}, open(os.path.join(a.out, "whole_pass.json"), "w"), indent=1)
        print(r.stdout)
        return r.returncode
    log = open(os.path.join(a.out, "mac_check_rate.log"), "w")
    rows, failed = [], None
    for n in [int(x) for x in a.streams.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.child_seconds), sys.executable, os.path.abspath(__file__), "--child", str(n), "--ks", ",".join(map(str, a.ks)), "--segment-gib", str(a.segment_gib), "--calls", str(a.calls)]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True)
        log.write("$ %s\n%s%s(exit %d, %.1f s)\n" % (" ".join(["python", "tools/mac_check_rate.py"] + cmd[6:]), r.stdout, r.stderr, r.returncode, time.time() - t0))
        log.flush()
        rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        if r.returncode != 0:
            failed = "the child for %d streams ended with status %d: nothing more was started" % (n, r.returncode)
            break
    out = {"yardsticks": YARDSTICKS, "rates": rows, "failed": failed}
    at256 = [x for x in rows if x["streams"] == max(q["streams"] for q in rows)] if rows else []
    if at256 and not failed:
        best = max(x["blocks_per_s"] for x in at256)
        out["default_k_rule"] = {"streams": at256[0]["streams"], "best_blocks_per_s": best, "largest_k_within_10_percent": max(x["k"] for x in at256 if x["blocks_per_s"] >= 0.9 * best)}
    json.dump(out, open(os.path.join(a.out, "mac_check_rate.json"), "w"), indent=1)
    for x in rows:
        print("%4d streams  k = %2d  %.3e blocks/s  %7.1f GB/s  (x %.2f of the production of 256 instances, %.2f of the AES ceiling)" % (
            x["streams"], x["k"], x["blocks_per_s"], x["bytes_per_s"] / 1e9, x["bytes_per_s"] / YARDSTICKS["production_256_instances_bytes_per_s"], x["blocks_per_s"] / YARDSTICKS["aes_ceiling_blocks_per_s"]))
    if failed:
        print(failed, file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
