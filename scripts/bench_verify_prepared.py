#!/usr/bin/env python3
"""Times cc.verify_prepared (g16_verify_prepared: one workgroup per proof under a prepared key) next to
cc.verify_batch and cc.verify_aggregate (one lane per proof) on the same valid proofs of tests/golden/test.zkey.

    python scripts/bench_verify_prepared.py --out profiles/verify_prepared_bench.txt

One process.  Proofs come from Prover.prove_batch.  Every shape is warmed up once with each of the three calls; then
`--reps` repetitions in which the three calls ALTERNATE on the same inputs.  Wall clock of the Python call (packing
included) and of the C call alone on a packed buffer; cc.prepare_verifying_key is timed on its own; the phases are
device times of the last call (the tests of B run beside the inputs and the pairing on a second stream).  Every
verdict list is compared with verify_batch's.  The record also names the smallest measured n at which verify_batch,
and verify_aggregate, is faster than verify_prepared.

GATE (exit status 1 when missed; the record is written either way): at n = 1 the SLOWEST repetition of
verify_prepared is under one fifth of the FASTEST repetition of verify_batch."""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 1000, 4096, 65536])
    ap.add_argument("--reps", type=int, default=5)
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
        out = fn()
        return out, time.perf_counter() - t0

    def fmt(ts):
        return "  ".join(f"{t * 1e3:9.3f}" for t in ts) + " ms"

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

    say(f"# verify_prepared vs verify_batch vs verify_aggregate on valid proofs of test.zkey; reps = {args.reps}, the "
        f"three calls alternate; library sha256 {hashlib.sha256(open(lib.path, 'rb').read()).hexdigest()[:16]}")
    sampler = bench.ClockSampler(0)                                                  # bench.py's: sclk while the calls run
    sampler.mark("timed")
    prep = []
    for _ in range(args.reps + 1):
        pvk, t = clock(lambda: cc.prepare_verifying_key(vk))
        prep.append(t)
        kernel_ms = cc.verify_prepared_times()["prepare"]
        pvk.close()
    say(f"prepare_verifying_key (first call, then {args.reps}): {fmt(prep)}; its kernel, last call: {kernel_ms:.3f} ms")
    pvk = cc.prepare_verifying_key(vk)
    h = pvk._handle()
    d, _ic = cc._vk_desc(vk)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    gate_ok, cross = True, {"verify_batch": None, "verify_aggregate": None}
    for n in args.sizes:
        batch, pub = proofs[:n], pubs[:n]
        buf = np.frombuffer(b"".join(p.raw for p in batch), dtype=np.uint8)
        fr = np.ascontiguousarray(cc.fr_from_ints([x for p in pub for x in p]))
        ok_p, ok_b, ok_a = (np.zeros(n, dtype=np.uint8) for _ in range(3))
        calls = {
            "verify_prepared": lambda: cc.verify_prepared(pvk, batch, pub),
            "verify_batch": lambda: cc.verify_batch(vk, batch, pub),
            "verify_aggregate": lambda: cc.verify_aggregate(vk, batch, pub),
            "C verify_prepared": lambda: lib.check(lib.g16_verify_prepared(h, ptr(buf), ptr(fr), n, ptr(ok_p))),
            "C verify_batch": lambda: lib.check(lib.g16_verify_batch(0, C.byref(d), ptr(buf), ptr(fr), n, ptr(ok_b))),
            "C verify_aggregate": lambda: lib.check(lib.g16_verify_aggregate(0, C.byref(d), ptr(buf), ptr(fr), n, None,
                                                                             ptr(ok_a), None)),
        }
        for fn in calls.values():                                                   # warm-up of this shape
            fn()
        ts = {k: [] for k in calls}
        phases = None
        for _ in range(args.reps):
            for name, fn in calls.items():
                out, t = clock(fn)
                ts[name].append(t)
                if name == "verify_prepared":
                    got = out
                    phases = cc.verify_prepared_times()
                elif name == "verify_batch":
                    assert got == out and all(out), "verdicts differ from verify_batch's"
                elif name == "verify_aggregate":
                    assert out is True
            assert np.array_equal(ok_p, ok_b) and ok_b.all() and ok_a[0] == 1
        for name in calls:
            say(f"n = {n:6d}: {name:20s} {fmt(ts[name])}")
        say(f"n = {n:6d}:   device ms per phase, last call: " + "  ".join(f"{k} {v:.3f}" for k, v in phases.items()))
        best = {k: min(v) for k, v in ts.items()}
        say(f"n = {n:6d}:   fastest verify_batch / slowest verify_prepared = "
            f"{best['verify_batch'] / max(ts['verify_prepared']):.1f}   fastest verify_aggregate / slowest verify_prepared"
            f" = {best['verify_aggregate'] / max(ts['verify_prepared']):.1f}   (C calls alone: "
            f"{best['C verify_batch'] / max(ts['C verify_prepared']):.1f}, "
            f"{best['C verify_aggregate'] / max(ts['C verify_prepared']):.1f})")
        for other in cross:
            if cross[other] is None and best[other] < best["verify_prepared"]:
                cross[other] = n
        if n == 1:
            gate_ok = max(ts["verify_prepared"]) * 5 < best["verify_batch"]
            say(f"# gate at n = 1: slowest verify_prepared {max(ts['verify_prepared']) * 1e3:.3f} ms x 5 "
                f"{'<' if gate_ok else '>='} fastest verify_batch {best['verify_batch'] * 1e3:.3f} ms: "
                f"{'passed' if gate_ok else 'MISSED'}")
    for other, n in cross.items():
        say(f"# smallest measured n at which {other} is faster than verify_prepared: "
            f"{n if n is not None else 'none up to ' + str(max(args.sizes))}")
    pvk.close()
    sampler.stop()
    clk = sampler.summary()
    say(f"# box: sclk median {clk['timed']['sclk_mhz_median']} MHz (min {clk['timed']['sclk_mhz_min']}, max "
        f"{clk['timed']['sclk_mhz_max']}, {clk['timed']['samples']} samples, {clk['source']})")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if gate_ok else 1


if __name__ == "__main__":
    sys.exit(main())
