"""Throughput of g16_verify_batch (one lane per proof): n copies of a valid proof of the reference's
test.zkey + one wrong public input at a known position.  python scripts/verify_bench.py [n=16384]
--aggregate times g16_verify_aggregate (one combined check per batch) on the same n proofs instead:
per repetition the all-valid batch (accepted) and the batch with the wrong input (rejected)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import circom_compat_amd as cc

args = [a for a in sys.argv[1:] if a != "--aggregate"]
aggregate = len(args) != len(sys.argv) - 1
n = int(args[0]) if args else 16384
pk, mats = cc.read_zkey(os.path.join(ROOT, "tests", "golden", "test.zkey"))
proof = cc.Prover(pk, mats).prove(12345, 67890, [1, 33, 3, 11])
pubs = [[33]] * n
if aggregate:
    bad = list(pubs)
    bad[n // 3] = [34]
    for rep in range(2):
        t = time.perf_counter()
        ok = cc.verify_aggregate(pk.vk, [proof] * n, pubs)
        dt = time.perf_counter() - t
        t = time.perf_counter()
        rejected = not cc.verify_aggregate(pk.vk, [proof] * n, bad)
        dt_bad = time.perf_counter() - t
        assert ok and rejected
        print(f"aggregate n={n} rep={rep}: {dt * 1e3:.1f} ms, {n / dt:.0f} proofs/s; "
              f"with one wrong input {dt_bad * 1e3:.1f} ms (host packing included)")
    sys.exit(0)
pubs[n // 3] = [34]
for rep in range(2):
    t = time.perf_counter()
    ok = cc.verify_batch(pk.vk, [proof] * n, pubs)
    dt = time.perf_counter() - t
    assert ok.count(False) == 1 and ok[n // 3] is False
    print(f"n={n} rep={rep}: {dt * 1e3:.1f} ms, {n / dt:.0f} proofs/s (host packing included)")
