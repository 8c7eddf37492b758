#!/usr/bin/env python3
"""Times cc.check_key (g16_key_check) next to the cost a user already pays for the same key: Prover(...)
creation (g16_ctx_create: upload, point planes, tables).

    python scripts/bench_keycheck.py --logs 16 20 --reps 2 [--out profiles/keycheck_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_keycheck.py --logs 20 --reps 1 --no-prover

Keys: squaring chains minted by the GPU key generator (bench.chain_circuit + cc.trapdoor_setup), so
n_vars = domain_size = 2^log: 4 * 2^log G1 points and 2^log G2 points.  Wall times include the host-side
staging copies; one warm-up call (HIP module load, first pinned allocation) precedes the timed ones."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-prover", action="store_true", help="skip the Prover(...) creation timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import circom_compat_amd as cc

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# check_key vs Prover creation; chunk = {os.environ.get('G16_KEYCHECK_CHUNK', 'default (2^18 points)')}")
    warm = False
    for k in args.logs:
        mats, (A, Bm, Cm), _w, n_vars = bench.chain_circuit(cc, k)
        rng = random.Random(k)
        t0 = time.perf_counter()
        pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, bench.R_MOD) for _ in range(5)])
        say(f"2^{k}: n_vars = {n_vars}, key minted in {time.perf_counter() - t0:.2f} s")
        if not warm:
            cc.check_key(pk, max_listed=0)
            warm = True
        checks = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rep = cc.check_key(pk)
            checks.append(time.perf_counter() - t0)
            assert rep.ok, rep
        say(f"2^{k}: check_key        " + "  ".join(f"{t * 1e3:9.1f} ms" for t in checks) + f"   ok={rep.ok}")
        if not args.no_prover:
            creates = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                pr = cc.Prover(pk, mats)
                creates.append(time.perf_counter() - t0)
                pr.close()
            say(f"2^{k}: Prover creation  " + "  ".join(f"{t * 1e3:9.1f} ms" for t in creates))
            say(f"2^{k}: check_key / Prover creation = {min(checks) / min(creates):.2f} (best of {args.reps} each)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
