#!/usr/bin/env python3
"""Times cc.rerandomize (g16_proofs_rerandomize) next to cc.verify_batch and cc.verify_aggregate on the same batch of
valid proofs of tests/golden/test.zkey, and checks the result: every output batch passes verify_aggregate for the
original public inputs, and no output proof equals its input.

    python scripts/bench_rerandomize.py --out profiles/rerandomize_bench.txt

Proofs come from Prover.prove_batch on the table path.  Wall times are those of the Python calls (packing the proofs
into one buffer and wrapping the results included); "C call" is the library call alone on a prepared buffer; the
phases are device times of the last call (the G1 and G2 ladders run side by side on two streams, so they add up to
more than the wall time).  One warm-up call of each entry point (HIP module load, first pinned allocation) precedes
the timed ones."""
import argparse
import ctypes as C
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 1000, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import bench
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        out, ts = None, []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return out, "  ".join(f"{t * 1e3:9.2f} ms" for t in ts), min(ts)

    lib = B.load()
    pk, mats = cc.read_zkey(open(os.path.join(ROOT, "tests", "golden", "test.zkey"), "rb").read())
    vk = pk.vk
    n_max = max(args.sizes)
    rng = random.Random(1)
    pr = cc.Prover(pk, mats, tables=1)
    proofs, pubs = [], []
    for at in range(0, n_max, 8192):
        m = min(8192, n_max - at)
        ab = [(rng.randrange(bench.R_MOD), rng.randrange(bench.R_MOD)) for _ in range(m)]
        ws = [[1, a * b % bench.R_MOD, a, b] for a, b in ab]
        rs = [(rng.randrange(bench.R_MOD), rng.randrange(bench.R_MOD)) for _ in range(m)]
        proofs += pr.prove_batch(rs, ws)
        pubs += [[w[1]] for w in ws]
    pr.close()

    say(f"# rerandomize vs verify_batch vs verify_aggregate on valid proofs of test.zkey; reps = {args.reps}; "
        f"times of each rep, ratios from the fastest")
    sampler = bench.ClockSampler(0)                                                  # bench.py's: sclk while the calls run
    sampler.mark("timed")
    cc.rerandomize(vk, proofs[:2])                                                   # warm-up
    cc.verify_batch(vk, proofs[:2], pubs[:2])
    cc.verify_aggregate(vk, proofs[:2], pubs[:2])
    delta = np.frombuffer(bytes(vk.delta_g2), dtype=np.uint8)
    for n in args.sizes:
        batch, pub = proofs[:n], pubs[:n]
        out, ts, best = timed(lambda: cc.rerandomize(vk, batch))
        say(f"n = {n:6d}: rerandomize       {ts}   {n / best / 1e3:9.1f} k proofs/s")
        say(f"n = {n:6d}:   device ms per phase, last call: "
            + "  ".join(f"{name} {ms:.3f}" for name, ms in cc.rerandomize_times().items()))
        buf = np.frombuffer(b"".join(p.raw for p in batch), dtype=np.uint8)
        res = np.empty_like(buf)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
        _, ts, best_c = timed(lambda: lib.check(lib.g16_proofs_rerandomize(0, ptr(delta), ptr(buf), n, None, ptr(res),
                                                                           None)))
        say(f"n = {n:6d}:   C call alone    {ts}")
        fresh = all(o.raw != p.raw for o, p in zip(out, batch)) and not np.array_equal(res, buf)
        good, ts_a, best_a = timed(lambda: cc.verify_aggregate(vk, out, pub))
        say(f"n = {n:6d}: verify_aggregate  {ts_a}   of the output: {good}; no output equals its input: {fresh}")
        assert good and fresh
        assert cc.verify_aggregate(vk, [res[i * 256:(i + 1) * 256].tobytes() for i in range(n)], pub)
        each, ts_b, best_b = timed(lambda: cc.verify_batch(vk, out, pub))
        say(f"n = {n:6d}: verify_batch      {ts_b}   all true: {all(each)}")
        assert all(each)
        say(f"n = {n:6d}:   rerandomize / verify_batch = {best / best_b:.3f}   rerandomize / verify_aggregate = "
            f"{best / best_a:.3f}   (C call alone: {best_c / best_b:.3f}, {best_c / best_a:.3f})")
    sampler.stop()
    clock = sampler.summary()
    say(f"# box: sclk median {clock['timed']['sclk_mhz_median']} MHz (min {clock['timed']['sclk_mhz_min']}, max "
        f"{clock['timed']['sclk_mhz_max']}, {clock['timed']['samples']} samples, {clock['source']})")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
