#!/usr/bin/env python3
"""Times ONE cc.verify_aggregate_keys call against the loop of K cc.verify_aggregate calls, and ONE
cc.verify_batch_keys call against K cc.verify_batch calls: same inputs, same process, K keys x n proofs each.

    python scripts/bench_verify_keys.py --out profiles/verify_keys_bench.txt
    python scripts/bench_verify_keys.py --keys 8 --proofs 64 --out /dev/null        # one shape, e.g. under a kernel trace

Keys: test.zkey's and K - 1 phase-2 contributions to it (alpha, beta, gamma shared, delta differs: the snarkjs
situation); per key one proof of the product prover, n copies of it.  Per shape one warm-up of each of the four
measurements, then two repetitions; wall clock of the Python call, host packing included.  Every shape runs under
a time limit of its own (SIGALRM with its default action ends the process, also inside a library call).

What is measured against is the loop of the existing calls in this run, never a figure of another day.  The gate,
per shape and per pair (single call, loop), with spread = the larger of the two differences between repetitions:
K >= 2: the single call's slower repetition is faster than the loop's faster one; K = 1: the single call's faster
repetition is within the spread of the loop's.  The single-key calls are the one-group case of the code the _keys calls
run, so at K = 1 the script compares a code path with itself (the row shows the repetition spread and nothing else);
the K >= 2 gate is the one that decides.  A shape that misses it is reported, the record is still written,
and the exit status is 1."""
import argparse
import hashlib
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 2, 8, 32])
    ap.add_argument("--proofs", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per shape")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import bench
    import circom_compat_amd as cc
    from circom_compat_amd import _binding

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def reps(fn, want):
        assert fn() == want                                                          # warm-up
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            got = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert got == want
        return ts

    lib_path = _binding.load().path
    say(f"# verify_aggregate_keys / verify_batch_keys against the loop of single-key calls; library sha256 "
        f"{hashlib.sha256(open(lib_path, 'rb').read()).hexdigest()[:16]}")
    say("# ms per repetition (2 after 1 warm-up), wall clock of the Python call(s), host packing included")
    signal.alarm(args.step_timeout)
    pk, mats = cc.read_zkey(os.path.join(ROOT, "tests", "golden", "test.zkey"))
    keys = []
    for k in range(max(args.keys)):
        pk = cc.contribute_key(pk, 0xC0FFEE + k) if k else pk
        pr = cc.Prover(pk, mats)
        keys.append((pk.vk, pr.prove(12345 + k, 67890 + k, [1, 33, 3, 11])))
        pr.close()
    sampler = bench.ClockSampler(0)                                                  # bench.py's: sclk while the calls run
    sampler.mark("timed")
    failed = []
    for n in args.proofs:
        for K in args.keys:
            signal.alarm(args.step_timeout)
            groups = [(vk, [proof] * n, [[33]] * n) for vk, proof in keys[:K]]
            one = reps(lambda: cc.verify_aggregate_keys(groups), [True] * K)
            loop = reps(lambda: [cc.verify_aggregate(*g) for g in groups], [True] * K)
            bone = reps(lambda: cc.verify_batch_keys(groups), [[True] * n] * K)
            bloop = reps(lambda: [cc.verify_batch(*g) for g in groups], [[True] * n] * K)
            for name, a, b in (("aggregate", one, loop), ("per-proof", bone, bloop)):
                spread = max(abs(a[0] - a[1]), abs(b[0] - b[1]))
                ok = max(a) < min(b) if K >= 2 else min(a) - min(b) <= spread
                say(f"K={K:2d} n={n:4d} {name}: one call {a[0]:8.1f} {a[1]:8.1f}   loop of {K:2d} {b[0]:8.1f} {b[1]:8.1f}"
                    f"   loop/one {min(b) / min(a):5.2f}   spread {spread:5.1f}   gate {'pass' if ok else 'MISSED'}")
                if not ok:
                    failed.append((K, n, name))
    signal.alarm(0)
    sampler.stop()
    clock = sampler.summary()
    say(f"# box: sclk median {clock['timed']['sclk_mhz_median']} MHz (min {clock['timed']['sclk_mhz_min']}, max "
        f"{clock['timed']['sclk_mhz_max']}, {clock['timed']['samples']} samples, {clock['source']})")
    say(f"# gate missed: {failed}" if failed else "# gate: every shape passed")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
