#!/usr/bin/env python3
"""Times cc.contribute_srs (g16_srs_contribute) next to cc.trapdoor_srs and cc.check_srs on the same size, and
compares the contributed string byte for byte with cc.trapdoor_srs of the product trapdoor.

    python scripts/bench_srs_contribute.py --logs 16 20 --reps 2 --out profiles/srs_contribute_bench.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_srs_contribute.py --logs 16 --reps 1 --out /dev/null

Strings: cc.trapdoor_srs(log) -- 4 * 2^log - 1 G1 points and 2^log G2 points.  At 2^20 the longest array has 2^21 - 1
points: the default chunk of 2^18 is crossed seven times there, three times in the other arrays.  Wall times include the
host-side staging copies; the phases are device times summed over the chunks (the copies run under the kernels, so
they add up to more than the wall time).  One warm-up call (HIP module load, first pinned allocation) precedes the
timed ones."""
import argparse
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", required=True)
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
        return out, "  ".join(f"{t * 1e3:9.1f} ms" for t in ts), min(ts)

    say(f"# contribute_srs vs trapdoor_srs vs check_srs; chunk = "
        f"{os.environ.get('G16_SRSCONTRIB_CHUNK', 'default (2^18 points)')}; reps = {args.reps}")
    sampler = bench.ClockSampler(0)                                                  # bench.py's: sclk while the calls run
    sampler.mark("timed")
    cc.contribute_srs(cc.trapdoor_srs(4, [3, 5, 7]), (2, 3, 4))                      # warm-up
    for k in args.logs:
        rng = random.Random(k)
        tox = [rng.randrange(2, bench.R_MOD) for _ in range(3)]
        sec = [rng.randrange(2, bench.R_MOD) for _ in range(3)]
        srs, ts, _ = timed(lambda: cc.trapdoor_srs(k, tox))
        say(f"2^{k}: trapdoor_srs     {ts}")
        got, ts, best = timed(lambda: cc.contribute_srs(srs, sec))
        points = 4 * (1 << k) - 1 + (1 << k)
        say(f"2^{k}: contribute_srs   {ts}   {points / best / 1e6:.2f} M points/s")
        say(f"2^{k}:   device ms per phase, last call: "
            + "  ".join(f"{name} {ms:.1f}" for name, ms in cc.contribute_srs_times().items()))
        want = cc.trapdoor_srs(k, [x * y % bench.R_MOD for x, y in zip(tox, sec)])
        same = all(np.array_equal(getattr(got, n), getattr(want, n))
                   for n in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")) and got.beta_g2 == want.beta_g2
        say(f"2^{k}:   bytes equal trapdoor_srs of the product trapdoor: {same}")
        assert same
        del want
        rep, ts, _ = timed(lambda: cc.check_srs(got))
        say(f"2^{k}: check_srs        {ts}   ok={rep.ok}")
        assert rep.ok, rep
    sampler.stop()
    clock = sampler.summary()
    say(f"# box: sclk median {clock['timed']['sclk_mhz_median']} MHz (min {clock['timed']['sclk_mhz_min']}, max "
        f"{clock['timed']['sclk_mhz_max']}, {clock['timed']['samples']} samples, {clock['source']})")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
