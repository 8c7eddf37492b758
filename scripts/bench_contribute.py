#!/usr/bin/env python3
"""Times cc.contribute_key (g16_key_contribute) and cc.check_contribution (g16_key_contribution_check) next to
what a user already pays for the same key: cc.check_key and Prover(...) creation.

    python scripts/bench_contribute.py --logs 16 20 --reps 2 [--out profiles/contribute_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_contribute.py --logs 20 --reps 1 --only

Keys: squaring chains minted by the GPU key generator (bench.chain_circuit + cc.trapdoor_setup), so
n_vars = domain_size = 2^log: a contribution multiplies 2 * 2^log - 2 G1 points.  Wall times include the
host-side staging copies; one warm-up call of each entry point (HIP module load, first pinned allocation)
precedes the timed ones.  The contributed key is compared with the key the generator mints for delta * d."""
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
    ap.add_argument("--only", action="store_true", help="contribute_key and check_contribution alone (profiling)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import bench
    import circom_compat_amd as cc

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        ts, out = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return ts, out

    fmt = lambda ts: "  ".join(f"{t * 1e3:9.1f} ms" for t in ts)
    say(f"# contribute_key / check_contribution; chunk = {os.environ.get('G16_CONTRIB_CHUNK', 'default (2^18 points)')}")
    warm = False
    for k in args.logs:
        mats, (A, Bm, Cm), _w, n_vars = bench.chain_circuit(cc, k)
        rng = random.Random(k)
        tox = [rng.randrange(1, bench.R_MOD) for _ in range(5)]
        d = rng.randrange(1, bench.R_MOD)
        t0 = time.perf_counter()
        pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, tox)
        say(f"2^{k}: n_vars = {n_vars}, key minted in {time.perf_counter() - t0:.2f} s")
        if not warm:
            cc.check_contribution(pk, cc.contribute_key(pk, d), max_listed=0)
            warm = True
        contribs, new = timed(lambda: cc.contribute_key(pk, d))
        say(f"2^{k}: contribute_key      {fmt(contribs)}   ({2 * n_vars - 2} points)")
        checks, rep = timed(lambda: cc.check_contribution(pk, new))
        assert rep.ok, rep
        say(f"2^{k}: check_contribution  {fmt(checks)}   ok={rep.ok}")
        if args.only:
            continue
        want = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, tox[:4] + [tox[4] * d % bench.R_MOD])
        same = (np.array_equal(new.l_query, want.l_query) and np.array_equal(new.h_query, want.h_query)
                and bytes(new.delta_g1) == bytes(want.delta_g1) and bytes(new.vk.delta_g2) == bytes(want.vk.delta_g2))
        assert same, "the contributed key differs from the generator's key for delta * d"
        say(f"2^{k}: equals trapdoor_setup(delta * d): {same}")
        del want
        keychecks, krep = timed(lambda: cc.check_key(pk))
        assert krep.ok, krep
        say(f"2^{k}: check_key           {fmt(keychecks)}")

        creates = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pr = cc.Prover(pk, mats)
            creates.append(time.perf_counter() - t0)
            pr.close()
        say(f"2^{k}: Prover creation     {fmt(creates)}")
        say(f"2^{k}: contribute_key / Prover creation = {min(contribs) / min(creates):.2f}, "
            f"check_contribution / check_key = {min(checks) / min(keychecks):.2f} (best of {args.reps} each)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
