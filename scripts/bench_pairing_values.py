#!/usr/bin/env python3
"""Times the pairing-value calls (g16_pairing_products, g16_gt_multiexp, g16_gt_to_ark / g16_gt_from_ark) on one GPU,
in one process, on the same points.

    python scripts/bench_pairing_values.py --out profiles/gt_bench.txt

The points are those of valid proofs of tests/golden/test.zkey (Prover.prove_batch): product i is the three pairs
(A_i, B_i), (C_i, B_{i+1}), (A_{i+1}, B_{i+2}).  Per n:
  products   ONE g16_pairing_products call of n products, next to a loop of n g16_pairing_check calls on the same pairs
             (the only other route to the same Miller loops: its answer is a bit) and next to g16_verify_prepared on n
             proofs.  EVERY value of the batched call is compared with the single call on the same pairs.
  multiexp   ONE g16_gt_multiexp call of n groups of one element with a full-width scalar; every value (n <= 64) or 64
             of them (above) compared with a single call's
  codecs     g16_gt_to_ark, g16_gt_from_ark without and with the membership test; the round trip is compared
Wall clock of the C call on packed buffers, `--reps` repetitions after one warm-up of each shape (above n = 64 the
loop of single g16_pairing_check calls is timed once: it takes minutes); device phases of the last call from
g16_gt_times.

Exit status 1 (the record is written either way) on any mismatch, and if at n = 64 the SLOWEST repetition of the one
batched call is not faster than the FASTEST repetition of the 64 single g16_pairing_check calls."""
import argparse
import ctypes as C
import hashlib
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 4096])
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

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def fmt(ts):
        return "  ".join(f"{t * 1e3:10.3f}" for t in ts) + " ms"

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    lib = B.load()
    pk, mats = cc.read_zkey(open(os.path.join(ROOT, "tests", "golden", "test.zkey"), "rb").read())
    n_max = max(args.sizes)
    rng = random.Random(1)
    pr = cc.Prover(pk, mats, tables=1)
    ab = [(rng.randrange(bench.R_MOD), rng.randrange(bench.R_MOD)) for _ in range(n_max + 2)]
    ws = [[1, a * b % bench.R_MOD, a, b] for a, b in ab]
    rs = [(rng.randrange(bench.R_MOD), rng.randrange(bench.R_MOD)) for _ in range(n_max + 2)]
    proofs = [p.raw for p in pr.prove_batch(rs, ws)]
    pubs = [[w[1]] for w in ws]
    pr.close()
    pvk = cc.prepare_verifying_key(pk.vk)

    say(f"# pairing values on the points of valid proofs of test.zkey, 3 pairs per product; reps = {args.reps}; library "
        f"sha256 {hashlib.sha256(open(lib.path, 'rb').read()).hexdigest()[:16]}")
    sampler = bench.ClockSampler(0)
    sampler.mark("timed")
    ok_all, gate_ok = True, True

    def mismatch(what):
        nonlocal ok_all
        ok_all = False
        say(f"# MISMATCH: {what}")

    for n in args.sizes:
        g1 = np.frombuffer(b"".join(proofs[i][:64] + proofs[i][192:] + proofs[i + 1][:64] for i in range(n)), dtype=np.uint8)
        g2 = np.frombuffer(b"".join(proofs[i][64:192] + proofs[i + 1][64:192] + proofs[i + 2][64:192] for i in range(n)),
                           dtype=np.uint8)
        off = np.arange(0, 3 * n + 1, 3, dtype=np.uint32)
        out = np.zeros(n * 384, dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        one_off, unit_off = np.array([0, 3], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
        one_out, bit = np.zeros(384, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        vbuf = np.frombuffer(b"".join(proofs[:n]), dtype=np.uint8)
        vfr = np.ascontiguousarray(cc.fr_from_ints([x for p in pubs[:n] for x in p]))
        vok = np.zeros(n, dtype=np.uint8)

        def batched():
            lib.check(lib.g16_pairing_products(0, ptr(g1), ptr(g2), ptr(off), n, ptr(out), ptr(ok)))

        def check_loop():
            for i in range(n):
                lib.check(lib.g16_pairing_check(0, ptr(g1[192 * i:]), ptr(g2[384 * i:]), 3, ptr(bit)))

        def prepared():
            lib.check(lib.g16_verify_prepared(pvk._handle(), ptr(vbuf), ptr(vfr), n, ptr(vok)))

        calls = {"pairing_products, one call": batched, f"pairing_check x {n}": check_loop, "verify_prepared": prepared}
        loop = f"pairing_check x {n}"
        for name, fn in calls.items():                                              # warm-up of this shape; the loop's
            if name != loop or n <= 64:                                             # single call has no shape to warm
                fn()
        ts = {k: [] for k in calls}
        for rep in range(args.reps):
            for name, fn in calls.items():
                if name != loop or n <= 64 or rep == 0:                             # above 64 the loop is timed once
                    ts[name].append(clock(fn))
        batched()
        phases = cc.gt_times()
        for name in calls:
            say(f"n = {n:5d}: {name:28s} {fmt(ts[name])}")
        say(f"n = {n:5d}:   pairing_products device ms per phase, last call: " +
            "  ".join(f"{k} {v:.3f}" for k, v in phases.items()))
        if not (ok.all() and vok.all()):
            mismatch(f"n = {n}: a product or a proof was refused")
        t0 = time.perf_counter()
        for i in range(n):
            lib.check(lib.g16_pairing_products(0, ptr(g1[192 * i:]), ptr(g2[384 * i:]), ptr(one_off), 1, ptr(one_out), None))
            if not np.array_equal(one_out, out[384 * i:384 * i + 384]):
                mismatch(f"n = {n}: product {i} differs from the single call")
                break
        say(f"n = {n:5d}:   every value equals the single call's; {n} single pairing_products calls took "
            f"{(time.perf_counter() - t0) * 1e3:.3f} ms, comparison included")
        if n == 64:
            slow, fast = max(ts["pairing_products, one call"]), min(ts[f"pairing_check x {n}"])
            gate_ok = slow < fast
            say(f"# gate at n = 64: slowest batched call {slow * 1e3:.3f} ms {'<' if gate_ok else '>='} fastest loop of 64 "
                f"pairing_check calls {fast * 1e3:.3f} ms: {'passed' if gate_ok else 'MISSED'}")

        # multiexp: n groups of one element, full-width scalars
        sc = np.frombuffer(b"".join(rng.randrange(bench.R_MOD).to_bytes(32, "little") for _ in range(n)), dtype=np.uint64)
        moff = np.arange(0, n + 1, dtype=np.uint32)
        mout = np.zeros(n * 384, dtype=np.uint8)

        def multiexp():
            lib.check(lib.g16_gt_multiexp(0, ptr(out), ptr(sc), ptr(moff), n, ptr(mout)))

        multiexp()
        tm = [clock(multiexp) for _ in range(args.reps)]
        say(f"n = {n:5d}: {'gt_multiexp, one call':28s} {fmt(tm)}   kernels {cc.gt_times()['kernels']:.3f} ms")
        for i in (range(n) if n <= 64 else random.Random(2).sample(range(n), 64)):
            lib.check(lib.g16_gt_multiexp(0, ptr(out[384 * i:]), ptr(sc[4 * i:]), ptr(unit_off), 1, ptr(one_out)))
            if not np.array_equal(one_out, mout[384 * i:384 * i + 384]):
                mismatch(f"n = {n}: power {i} differs from the single call")
                break

        # codecs
        ark = np.zeros(n * 384, dtype=np.uint8)
        back = np.zeros(n * 384, dtype=np.uint8)
        why = np.zeros(n, dtype=np.uint8)
        codec = {"gt_to_ark": lambda: lib.check(lib.g16_gt_to_ark(0, ptr(out), n, ptr(ark))),
                 "gt_from_ark": lambda: lib.check(lib.g16_gt_from_ark(0, ptr(ark), n, 0, ptr(back), ptr(why))),
                 "gt_from_ark, validated": lambda: lib.check(lib.g16_gt_from_ark(0, ptr(ark), n, 1, ptr(back), ptr(why)))}
        for name, fn in codec.items():
            fn()
            tc = [clock(fn) for _ in range(args.reps)]
            say(f"n = {n:5d}: {name:28s} {fmt(tc)}   kernels {cc.gt_times()['kernels']:.3f} ms")
            if name != "gt_to_ark" and not (np.array_equal(back, out) and not why.any()):
                mismatch(f"n = {n}: {name} does not return what gt_to_ark was given")
    pvk.close()
    sampler.stop()
    clk = sampler.summary()
    say(f"# box: sclk median {clk['timed']['sclk_mhz_median']} MHz (min {clk['timed']['sclk_mhz_min']}, max "
        f"{clk['timed']['sclk_mhz_max']}, {clk['timed']['samples']} samples, {clk['source']})")
    say(f"# values: {'all equal' if ok_all else 'MISMATCH'}; gate: {'passed' if gate_ok else 'MISSED'}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if (ok_all and gate_ok) else 1


if __name__ == "__main__":
    sys.exit(main())
