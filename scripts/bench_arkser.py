#!/usr/bin/env python3
"""Times the ark-serialize codec (g16_points_from_ark / g16_points_to_ark, cc.read_ark_key / cc.write_ark_key) on the
arrays of one proving key, next to the costs a user already pays for the same key: cc.check_key and Prover(...)
creation.

    python scripts/bench_arkser.py --logs 16 20 --reps 2 --out profiles/arkser_bench.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_arkser.py --logs 16 --reps 1 --out /dev/null

Keys: squaring chains minted by the GPU key generator (bench.chain_circuit + cc.trapdoor_setup), so n_vars =
domain_size = 2^log: 4 * 2^log G1 points and 2^log G2 points.  Per size: encode and decode of a_query (G1) and
b_g2_query (G2), compressed and uncompressed, the G2 decode with and without G16_ARK_VALIDATE; then the whole key
through write_ark_key / read_ark_key.  Every decode is compared byte for byte with the array that was encoded.  Wall
times of the Python calls, host-side staging copies included; one warm-up call (HIP module load, first pinned
allocation) precedes the timed ones.  No arkworks CPU figure can be measured here: the record is the deliverable."""
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
    ap.add_argument("--no-prover", action="store_true", help="skip the Prover(...) creation timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arkser_bench.txt"))
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

    say(f"# ark-serialize codec vs check_key vs Prover creation; chunk = "
        f"{os.environ.get('G16_ARKSER_CHUNK', 'default (2^18 points)')}; reps = {args.reps}")
    sampler = bench.ClockSampler(0)                                                  # bench.py's: sclk while the calls run
    sampler.mark("timed")
    warm = False
    for k in args.logs:
        mats, (A, Bm, Cm), _w, n_vars = bench.chain_circuit(cc, k)
        rng = random.Random(k)
        t0 = time.perf_counter()
        pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, bench.R_MOD) for _ in range(5)])
        say(f"2^{k}: n_vars = {n_vars}, key minted in {time.perf_counter() - t0:.2f} s")
        if not warm:
            cc.points_from_ark(cc.points_to_ark(pk.b_g2_query[:64], "g2"), "g2")
            cc.check_key(pk, max_listed=0)
            warm = True
        for group, arr in (("g1", pk.a_query), ("g2", pk.b_g2_query)):
            n = arr.shape[0]
            for compressed in (True, False):
                mode = "compressed  " if compressed else "uncompressed"
                ark, ts, best = timed(lambda: cc.points_to_ark(arr, group, compressed=compressed))
                say(f"2^{k}: {group} encode {mode}           {ts}   {n / best / 1e6:7.2f} M points/s")
                for validate in ((True, False) if group == "g2" else (False,)):
                    (got, _why, bad), ts, best = timed(
                        lambda: cc.points_from_ark(ark, group, compressed=compressed, validate=validate))
                    assert bad == 0 and np.array_equal(got, arr), (group, compressed, validate, bad)
                    tag = "validate" if validate else "        "
                    say(f"2^{k}: {group} decode {mode} {tag}  {ts}   {n / best / 1e6:7.2f} M points/s   bytes equal")
        for compressed in (True, False):
            mode = "compressed  " if compressed else "uncompressed"
            blob, ts, _ = timed(lambda: cc.write_ark_key(pk, compressed=compressed))
            say(f"2^{k}: write_ark_key {mode}         {ts}   {len(blob) / 2 ** 20:.1f} MiB")
            back, ts, _ = timed(lambda: cc.read_ark_key(blob, compressed=compressed, validate=True))
            same = all(np.array_equal(getattr(back, q), getattr(pk, q))
                       for q in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query"))
            assert same
            say(f"2^{k}: read_ark_key  {mode} validate {ts}   arrays equal")
            del blob, back
        rep, ts, best_check = timed(lambda: cc.check_key(pk))
        assert rep.ok, rep
        say(f"2^{k}: check_key                          {ts}   ok={rep.ok}")
        if not args.no_prover:
            def create():
                cc.Prover(pk, mats).close()
            _, ts, _ = timed(create)
            say(f"2^{k}: Prover creation                    {ts}")
    sampler.stop()
    clock = sampler.summary()
    say(f"# box: sclk median {clock['timed']['sclk_mhz_median']} MHz (min {clock['timed']['sclk_mhz_min']}, max "
        f"{clock['timed']['sclk_mhz_max']}, {clock['timed']['samples']} samples, {clock['source']})")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
