#!/usr/bin/env python3
"""Times cc.check_srs (g16_srs_check) next to what is built on the same string: cc.setup_from_srs of a squaring
chain over it and cc.check_key of the resulting key.

    python scripts/bench_srs_check.py --logs 16 20 --reps 2 [--out profiles/srs_check_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_srs_check.py --logs 20 --reps 1 --only-check
    G16_SRSCHECK_SLICED=1 python scripts/bench_srs_check.py ...     the shifted sums as two ladders in two slices

Strings: cc.trapdoor_srs(log) -- 4 * 2^log - 1 G1 points and 2^log G2 points.  Wall times include the host-side
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
    ap.add_argument("--only-check", action="store_true", help="skip setup_from_srs and check_key")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import circom_compat_amd as cc

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
        return out, "  ".join(f"{t * 1e3:9.1f} ms" for t in ts)

    say(f"# check_srs vs setup_from_srs vs check_key; chunk = {os.environ.get('G16_SRSCHECK_CHUNK', 'default (2^18 points)')}"
        f"; sums = {'two slices' if os.environ.get('G16_SRSCHECK_SLICED') == '1' else 'fused chain'}")
    warm = False
    for k in args.logs:
        rng = random.Random(k)
        t0 = time.perf_counter()
        srs = cc.trapdoor_srs(k, [rng.randrange(2, bench.R_MOD) for _ in range(3)])
        say(f"2^{k}: string minted in {time.perf_counter() - t0:.2f} s")
        if not warm:
            cc.check_srs(cc.trapdoor_srs(4, [3, 5, 7]), max_listed=0)
            warm = True
        rep, ts = timed(lambda: cc.check_srs(srs))
        assert rep.ok, rep
        say(f"2^{k}: check_srs        {ts}   ok={rep.ok}")
        if args.only_check:
            continue
        _mats, (A, Bm, Cm), _w, n_vars = bench.chain_circuit(cc, k)
        pk, ts = timed(lambda: cc.setup_from_srs(A, Bm, Cm, n_vars, 1, srs))
        say(f"2^{k}: setup_from_srs   {ts}")
        rep, ts = timed(lambda: cc.check_key(pk))
        assert rep.ok, rep
        say(f"2^{k}: check_key        {ts}   ok={rep.ok}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
