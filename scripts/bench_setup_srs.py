#!/usr/bin/env python3
"""Times cc.setup_from_srs (g16_setup_from_srs) next to cc.trapdoor_setup (g16_setup_create) on the same circuits
and compares the two keys byte for byte.

    python scripts/bench_setup_srs.py --logs 12 16 20 [--out profiles/setup_srs_bench.txt]

Circuits: squaring chains (bench.chain_circuit), n_vars = domain = 2^log, coefficients 1 and r - 1 as circom emits
them.  The SRS is minted by cc.trapdoor_srs from the same (tau, alpha, beta); minting it is timed apart.  The
per-phase split is the library's own (g16_setup_from_srs_times: host clock around a stream synchronisation per
phase).  Every size runs in a child process of its own, after one warm-up call at 2^6 (HIP module load), under
--timeout seconds: a size that runs past it is ended and reported as such, and the run stops there (the sizes come
in ascending order)."""
import argparse
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--reduction", default="circom")
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is None:
        return parent(args)
    import numpy as np
    import bench
    import circom_compat_amd as cc

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def same(a, b):
        return (all(np.array_equal(getattr(a, q), getattr(b, q)) for q in QUERIES)
                and np.array_equal(a.vk.gamma_abc_g1, b.vk.gamma_abc_g1)
                and all(bytes(getattr(a, f)) == bytes(getattr(b, f)) for f in ("beta_g1", "delta_g1"))
                and all(bytes(getattr(a.vk, f)) == bytes(getattr(b.vk, f))
                        for f in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2")))

    def one(k, quiet=False):
        _mats, (A, Bm, Cm), _w, n_vars = bench.chain_circuit(cc, k)
        rng = random.Random(k)
        tox = [rng.randrange(2, bench.R_MOD) for _ in range(3)]
        t0 = time.perf_counter()
        srs = cc.trapdoor_srs(k, tox)
        t1 = time.perf_counter()
        got = cc.setup_from_srs(A, Bm, Cm, n_vars, 1, srs, reduction=args.reduction)
        t2 = time.perf_counter()
        ph = cc.setup_from_srs_times()
        want = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, tox + [1, 1], reduction=args.reduction)
        t3 = time.perf_counter()
        eq = same(got, want)
        if not quiet:
            say(f"2^{k}: n_vars = {n_vars}  trapdoor_srs {t1 - t0:8.3f} s  setup_from_srs {t2 - t1:8.3f} s  "
                f"trapdoor_setup {t3 - t2:8.3f} s  ratio {(t2 - t1) / (t3 - t2):6.1f}  keys equal: {eq}")
            say(f"2^{k}:   phases [ms]  " + "  ".join(f"{n} {v:.1f}" for n, v in ph.items()))
        assert eq, "setup_from_srs differs from trapdoor_setup(tau, alpha, beta, 1, 1)"

    one(6, quiet=True)
    one(args.child)


def parent(args):
    lines = [f"# setup_from_srs vs trapdoor_setup, reduction = {args.reduction}; phases: ntt_g1 = three size-n G1 "
             f"transforms, ntt_g2 = one size-n G2 transform, ntt_h = first stage of the size-2n transform + a size-n "
             f"G1 transform"]
    print(lines[0], flush=True)
    status = 0
    for k in sorted(args.logs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(k), "--reduction", args.reduction]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            out = r.stdout.strip().splitlines()
            if r.returncode:
                out.append(f"2^{k}: FAILED with status {r.returncode}: {r.stderr.strip().splitlines()[-1:]}")
                status = 1
        except subprocess.TimeoutExpired:
            out = [f"2^{k}: did NOT finish within {args.timeout} s"]
            status = 3
        for line in out:
            print(line, flush=True)
        lines += out
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if status:
            break
    return status


if __name__ == "__main__":
    sys.exit(main())
