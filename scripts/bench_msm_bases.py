#!/usr/bin/env python3
"""Times the MSM over caller-supplied bases, the division by (X - z) and KZG on one GPU, in one process.

    python scripts/bench_msm_bases.py --out profiles/kzg_bench.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_msm_bases.py --divide-only   (a run of its own)

Comparisons, every timed result compared byte for byte with an untimed single call, sides alternated, min / median of
--reps repetitions (wall clock of the C call; every call ends in a stream synchronise):
  1. g16_msm on a handle with full planes next to g16_msm_g1_dev on a ctx that holds the same points as its A query,
     same device-resident scalars, at 2^16 and 2^20 points: the same kernels on both sides.  GATE: the medians differ by
     no more than twice the spread (max - min) of the ctx call's own repetitions.
  2. g16_msm_once next to g16_msm_bases_create + one g16_msm with full planes; the number of reuses at which the
     planes start to pay is recorded (no gate).
  3. g16_kzg_open (the quotient stays on the device) next to g16_poly_divide_linear to the host followed by g16_msm from
     the host.  GATE: fused is not slower at 2^20.
  4. g16_kzg_verify at n = 1, 64, 4096 (recorded).
Exit status 1 (the record is written either way) on any byte mismatch or a missed gate."""
import argparse
import ctypes as C
import hashlib
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_fr(n, seed):
    """n canonical values below 2^253 < r as an (n, 32) uint8 array"""
    raw = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x1f
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--verify-sizes", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--divide-only", action="store_true", help="only the division at the largest size (kernel trace)")
    args = ap.parse_args()
    if not args.divide_only and not args.out:
        ap.error("--out is required")
    import bench
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    import torch

    lib = B.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def alternate(fns, reps):
        """{name: [ms]}: one warm-up of each, then reps rounds in which the sides take turns"""
        for fn in fns.values():
            fn()
        ts = {k: [] for k in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                ts[name].append(clock(fn))
        return ts

    def mm(ts):
        return f"min {min(ts):9.3f}  median {statistics.median(ts):9.3f} ms"

    if args.divide_only:
        n = 1 << max(args.logs)
        coeffs = cc.fr_from_canonical(random_fr(n, 1))
        z = cc.fr_from_ints([random.Random(2).randrange(bench.R_MOD)])
        d_in = torch.from_numpy(coeffs.view(np.int64)).cuda()
        d_q = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        rem = np.zeros((1, 4), dtype=np.uint64)
        for _ in range(1 + args.reps):
            lib.check(lib.g16_poly_divide_linear(0, d_in.data_ptr(), n, 1, ptr(z), B_FLAGS_DEVICE, d_q.data_ptr(), ptr(rem)))
        torch.cuda.synchronize()
        print(f"divided 2^{max(args.logs)} coefficients {1 + args.reps} times")
        return 0

    say(f"# MSM over caller-supplied bases, division by (X - z), KZG; reps = {args.reps}, sides alternated; library sha256 "
        f"{hashlib.sha256(open(lib.path, 'rb').read()).hexdigest()[:16]}")
    sampler = bench.ClockSampler(0)
    sampler.mark("timed")
    ok_all, gates = True, {}

    def mismatch(what):
        nonlocal ok_all
        ok_all = False
        say(f"# MISMATCH: {what}")

    rng = random.Random(3)
    for k in args.logs:
        # ---- 1. the new entry point next to the resident-key MSM: the same points, the same scalars
        mats, (A, Bm, Cm), w, n_vars = bench.chain_circuit(cc, k)
        pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, bench.R_MOD) for _ in range(5)])
        pts = np.ascontiguousarray(pk.a_query, dtype=np.uint8).reshape(-1, 64)[1:]
        n = pts.shape[0]
        pr = cc.Prover(pk, mats, tables=-1)
        scal = cc.fr_from_canonical(random_fr(n, 10 + k))
        d_s = torch.from_numpy(scal.view(np.int64)).cuda()
        h = cc.MsmBases(pts, "g1")
        info, pinfo = h.info(), pr.info()
        out_ctx, out_new = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
        fns = {"ctx": lambda: lib.check(lib.g16_msm_g1_dev(pr.ctx, B.QUERY_A, d_s.data_ptr(), n, ptr(out_ctx)), pr.ctx),
               "bases": lambda: lib.check(lib.g16_msm(h._h.ptr, d_s.data_ptr(), n, 1, n, B_FLAGS_DEVICE, ptr(out_new)))}
        ts = alternate(fns, args.reps)
        if out_ctx.tobytes() != out_new.tobytes():
            mismatch(f"2^{k}: g16_msm differs from g16_msm_g1_dev")
        spread = max(ts["ctx"]) - min(ts["ctx"])
        diff = statistics.median(ts["bases"]) - statistics.median(ts["ctx"])
        gates[f"entry point 2^{k}"] = abs(diff) <= 2 * spread
        say(f"n = {n} (2^{k} chain key, A query; window {info['window_bits']}, planes {info['planes']}, sets "
            f"{info['bucket_sets']}; ctx window {pinfo['c_w']}, planes {pinfo['planes_w']}, sets {pinfo['D_w']})")
        say(f"  1. g16_msm_g1_dev on the ctx       {mm(ts['ctx'])}   spread {spread:.3f} ms")
        say(f"     g16_msm on the handle           {mm(ts['bases'])}   median - median {diff:+.3f} ms, gate |diff| <= 2 x "
            f"spread: {'passed' if gates[f'entry point 2^{k}'] else 'MISSED'}")
        pr.close()

        # ---- 2. one-shot next to create + one multiply
        out_once = np.zeros(64, dtype=np.uint8)
        created = []

        def create():
            created.append(cc.MsmBases(pts, "g1"))

        def drop():
            created.pop().close()

        once = lambda: lib.check(lib.g16_msm_once(0, 0, ptr(pts), d_s.data_ptr(), n, B_FLAGS_DEVICE, ptr(out_once)))  # noqa: E731
        once()
        t_once, t_create = [], []
        for _ in range(args.reps):
            t_once.append(clock(once))
            t_create.append(clock(create))
            drop()
        if out_once.tobytes() != out_new.tobytes():
            mismatch(f"2^{k}: g16_msm_once differs from g16_msm")
        t_mul = statistics.median(ts["bases"])
        gain = statistics.median(t_once) - t_mul
        reuse = "never" if gain <= 0 else str(int(np.ceil(statistics.median(t_create) / gain)))
        say(f"  2. g16_msm_once (points from the host) {mm(t_once)}")
        say(f"     create with {info['planes']} planes           {mm(t_create)}   + one multiply {t_mul:.3f} ms; the planes pay "
            f"from {reuse} multiplications on")

        # ---- 3. fused open next to divide-to-host + MSM-from-host
        srs = cc.Srs(pts, np.zeros((2, 128), dtype=np.uint8), np.zeros((2, 64), dtype=np.uint8),
                     np.zeros((2, 64), dtype=np.uint8), bytes(128))     # any points serve as powers for a timing
        key = cc.KzgKey(srs, max_len=n)
        z = cc.fr_from_ints([rng.randrange(bench.R_MOD)])
        y_f, pi_f = np.zeros((1, 4), dtype=np.uint64), np.zeros(64, dtype=np.uint8)
        quot, y_u, pi_u = np.zeros((n - 1, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64), np.zeros(64, dtype=np.uint8)

        def fused():
            lib.check(lib.g16_kzg_open(key._h.ptr, ptr(scal), n, 1, n, ptr(z), 0, ptr(y_f), ptr(pi_f)))

        def unfused():
            lib.check(lib.g16_poly_divide_linear(0, ptr(scal), n, 1, ptr(z), 0, ptr(quot), ptr(y_u)))
            lib.check(lib.g16_msm(h._h.ptr, ptr(quot), n - 1, 1, n - 1, 0, ptr(pi_u)))

        to = alternate({"fused": fused, "unfused": unfused}, args.reps)
        phases = cc.kzg_times()
        if y_f.tobytes() != y_u.tobytes() or pi_f.tobytes() != pi_u.tobytes():
            mismatch(f"2^{k}: g16_kzg_open differs from divide + msm")
        gates[f"fused open 2^{k}"] = statistics.median(to["fused"]) <= statistics.median(to["unfused"])
        say(f"  3. g16_kzg_open, fused               {mm(to['fused'])}   device ms: " +
            "  ".join(f"{a} {b:.3f}" for a, b in phases.items()))
        say(f"     divide to host + msm from host    {mm(to['unfused'])}   gate fused <= unfused"
            f"{'' if k == max(args.logs) else ' (recorded; the gate is at the largest size)'}: "
            f"{'passed' if gates[f'fused open 2^{k}'] else 'MISSED'}")
        if k != max(args.logs):
            del gates[f"fused open 2^{k}"]
        key.close()
        h.close()

    # ---- 4. batch verification
    srs = cc.trapdoor_srs(4, (rng.randrange(1, bench.R_MOD), 3, 5))
    key = cc.KzgKey(srs, max_len=8, max_batch=64)
    nv = max(args.verify_sizes)
    polys = random_fr(nv * 8, 40).reshape(nv, 8, 32)
    zs = [rng.randrange(bench.R_MOD) for _ in range(nv)]
    cms = key.commit(polys)
    opened = key.open(polys, zs)
    cm = np.frombuffer(b"".join(cms), dtype=np.uint8)
    pf = np.frombuffer(b"".join(p for _, p in opened), dtype=np.uint8)
    zz, yy = cc.fr_from_ints(zs), cc.fr_from_ints([y for y, _ in opened])
    t2 = np.frombuffer(key.tau_g2, dtype=np.uint8)
    for n in args.verify_sizes:
        ok = C.c_uint8(0)

        def verify():
            lib.check(lib.g16_kzg_verify(0, ptr(t2), ptr(cm), ptr(zz), ptr(yy), ptr(pf), n, None, C.byref(ok)))

        verify()
        tv = [clock(verify) for _ in range(args.reps)]
        if not ok.value:
            mismatch(f"kzg_verify refused {n} valid openings")
        say(f"  4. g16_kzg_verify, n = {n:5d}          {mm(tv)}   device ms: " +
            "  ".join(f"{a} {b:.3f}" for a, b in cc.kzg_times().items()))
    key.close()
    sampler.stop()
    clk = sampler.summary()
    say(f"# box: sclk median {clk['timed']['sclk_mhz_median']} MHz (min {clk['timed']['sclk_mhz_min']}, max "
        f"{clk['timed']['sclk_mhz_max']}, {clk['timed']['samples']} samples, {clk['source']})")
    missed = [g for g, v in gates.items() if not v]
    say(f"# values: {'all equal' if ok_all else 'MISMATCH'}; gates: {'passed' if not missed else 'MISSED: ' + ', '.join(missed)}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if (ok_all and not missed) else 1


B_FLAGS_DEVICE = 2   # G16_MSM_SCALARS_DEVICE

if __name__ == "__main__":
    sys.exit(main())
