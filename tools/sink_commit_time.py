"""Wall time of Session.garble_to_sink on the two-instance small plan of tests/plan_small_lib.py: commitment="both" with outboards=True
beside commitment="cbcmac" — what the device hash and the outboard callback add to a drain that copies every ciphertext to the host.
One warm-up pass and REPEATS timed passes per form, alternating; prints every time and the medians.  No threshold: the small plan's
pass is launch- and latency-bound, so this is a number for the record, not a rate (profiles/callback_commit/sink_commit.log).

    python tools/sink_commit_time.py [log file]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REPEATS = 7


def main():
    import garbled_snark_verifier_amd as gsv
    import plan_small_lib as P
    import test_blake3_commit as Cm
    import test_blake3_evaluate as E
    import test_plan_small as T
    os.environ.setdefault("GSV_INSTANCES_PER_WG", "1")
    _, sp = T.small_plan()
    n_ct = sp.plan.info["n_ciphertexts"]
    seeds = [T.SEED0, T.SEED0 + 1]
    inputs = Cm._plan_inputs(gsv, sp, P, seeds)
    sess = gsv.Session(gsv.Engine(0), sp.plan, 2, **E._plan_opts("windows", n_ct))
    forms = {"cbcmac": dict(commitment="cbcmac"), "both+outboards": dict(commitment="both", outboards=True)}
    times = {k: [] for k in forms}
    sink = lambda inst, first, records: None  # noqa: E731 - the handler's own work is not what is measured
    for rep in range(REPEATS + 1):
        for name, kw in forms.items():
            sess.set_garble_inputs(*inputs)
            t0 = time.perf_counter()
            r = sess.garble_to_sink(sink, **kw)
            dt = time.perf_counter() - t0
            assert len(r.cbcmac) == 2 and (r.blake3 is None) == (name == "cbcmac")
            if rep:
                times[name].append(dt)
    sess.close()
    lines = ["garble_to_sink, small plan (%d ciphertexts per instance), 2 instances, GSV_B3_SUBTREE_LOG2=%s, %d passes per form after one warm-up" %
             (n_ct, os.environ.get("GSV_B3_SUBTREE_LOG2", "10 (default)"), REPEATS)]
    for name in forms:
        lines.append("%-16s median %.3f ms   [%s]" % (name, 1e3 * statistics.median(times[name]), " ".join("%.3f" % (1e3 * t) for t in times[name])))
    lines.append("difference of the medians: %+.3f ms" % (1e3 * (statistics.median(times["both+outboards"]) - statistics.median(times["cbcmac"]))))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
