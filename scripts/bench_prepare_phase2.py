#!/usr/bin/env python3
"""Times the prepared-powers-of-tau calls: cc.prepare_phase2 (g16_srs_prepare), cc.check_lagrange
(g16_srs_lagrange_check) next to cc.check_srs on the same string, and cc.setup_from_srs with and without lagrange=
on a squaring chain whose domain is 2^power.

    python scripts/bench_prepare_phase2.py [--powers 12 16] [--reps 5] --out profiles/prepare_phase2_bench.txt

Everything runs in this one process; one warm-up call of every timed function (HIP module load, first pinned
allocation) precedes the timed ones; the figure is the median of --reps wall times, host-side staging included.
No time is fixed in advance.  The script exits non-zero unless
  (a) setup_from_srs(lagrange=...) is faster than the plain call at every power: it runs a strict subset of its
      device work on inputs of the same size;
  (b) check_lagrange is faster than prepare_phase2 at power 16 (when 16 is among --powers): by operation count it is
      about 2^P * 510 ladder steps against about 2^P * P * 255, so a check slower than recomputing would be pointless;
and every key and every Lagrange set timed is the same bytes on every repetition and the two keys are equal."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")


def same_set(a, b):
    return a.power == b.power and all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ARRAYS)


def same_key(a, b):
    return (all(np.array_equal(np.asarray(getattr(a, q)), np.asarray(getattr(b, q))) for q in QUERIES)
            and np.array_equal(np.asarray(a.vk.gamma_abc_g1), np.asarray(b.vk.gamma_abc_g1))
            and all(bytes(getattr(a.vk, f)) == bytes(getattr(b.vk, f)) for f in ("alpha_g1", "beta_g2", "gamma_g2",
                                                                                 "delta_g2"))
            and bytes(a.beta_g1) == bytes(b.beta_g1) and bytes(a.delta_g1) == bytes(b.delta_g1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--powers", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    import circom_compat_amd as cc

    lines, failures = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, same):
        """median wall time of --reps calls behind one warm-up call; every result equals the warm-up's"""
        first = fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
            if not same(out, first):
                failures.append("a repetition returned other bytes")
        return first, statistics.median(ts), ts

    def show(ts):
        return "  ".join(f"{t * 1e3:.1f}" for t in ts)

    say(f"# prepare_phase2 / check_lagrange / setup_from_srs(lagrange=); median of {args.reps} wall times in ms "
        f"(all of them in brackets), one warm-up call each; chunk = "
        f"{os.environ.get('G16_LAGCHECK_CHUNK', 'default (2^18 points)')}")
    for k in args.powers:
        rng = random.Random(k)
        srs = cc.trapdoor_srs(k, [rng.randrange(2, bench.R_MOD) for _ in range(3)])
        lag, t_prep, ts = timed(lambda: cc.prepare_phase2(srs), same_set)
        say(f"2^{k}: prepare_phase2           {t_prep * 1e3:10.1f} ms   [{show(ts)}]   phases {cc.prepare_phase2_times()}")
        rep, t_chk, ts = timed(lambda: cc.check_lagrange(srs, lag, max_listed=0), lambda a, b: a.ok and b.ok)
        if not rep.ok:
            failures.append(f"2^{k}: check_lagrange rejects the set prepare_phase2 made: {rep}")
        say(f"2^{k}: check_lagrange           {t_chk * 1e3:10.1f} ms   [{show(ts)}]   ok={rep.ok}")
        rep, t_srs, ts = timed(lambda: cc.check_srs(srs, max_listed=0), lambda a, b: a.ok and b.ok)
        say(f"2^{k}: check_srs                {t_srs * 1e3:10.1f} ms   [{show(ts)}]   ok={rep.ok}")
        _mats, (A, Bm, Cm), _w, n_vars = bench.chain_circuit(cc, k)
        plain, t_plain, ts = timed(lambda: cc.setup_from_srs(A, Bm, Cm, n_vars, 1, srs), same_key)
        say(f"2^{k}: setup_from_srs           {t_plain * 1e3:10.1f} ms   [{show(ts)}]")
        prep, t_lag, ts = timed(lambda: cc.setup_from_srs(A, Bm, Cm, n_vars, 1, srs, lagrange=lag), same_key)
        say(f"2^{k}: setup_from_srs(lagrange) {t_lag * 1e3:10.1f} ms   [{show(ts)}]")
        if plain.domain_size != 1 << k or not same_key(plain, prep):
            failures.append(f"2^{k}: the two keys differ")
        say(f"2^{k}: ratios  setup plain / prepared = {t_plain / t_lag:.2f}   prepare_phase2 / check_lagrange = "
            f"{t_prep / t_chk:.2f}   check_lagrange / check_srs = {t_chk / t_srs:.2f}")
        if not t_lag < t_plain:
            failures.append(f"2^{k}: (a) setup_from_srs(lagrange=) {t_lag * 1e3:.1f} ms is not faster than the plain "
                            f"call {t_plain * 1e3:.1f} ms")
        if k == 16 and not t_chk < t_prep:
            failures.append(f"2^16: (b) check_lagrange {t_chk * 1e3:.1f} ms is not faster than prepare_phase2 "
                            f"{t_prep * 1e3:.1f} ms")
    for f in failures:
        say("FAILED: " + f)
    if not failures:
        say("# all byte comparisons held; (a) and (b) hold")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
