"""From a .wtns file to a proof: the host-converting path against canonical ingestion on the device, on one MI355X.

For squaring chains of 2^16, 2^20 and 2^22 constraints (trapdoor key minted on the GPU, the library's automatic table
rule) a .wtns is written, and in ONE process, with the same (r, s):
  old   cc.read_wtns(path) + prover.prove(r, s, w)      the host loop of g16_wtns_read, then g16_prove
  new   prover.prove_wtns(path, r, s)                   g16_wtns_open (mmap) + g16_prove_canonical
each after one untimed pass, --reps timed passes (at least 5): median and range.  The two proofs must be byte-equal.
Breakdown of the new path (medians of the same number of passes): map = open_wtns; upload = staging + H2D +
conversion + the wait for them (upload_witness_canonical, host-timed); convert = the conversion kernel alone over the
same values (HIP events, g16_fr_convert_times); proof = prove_dev from the resident witness.
The old path is the yardstick: the script exits non-zero unless the new path is faster at every size.
    python scripts/bench_wtns.py [--sizes 16,20,22] [--reps 5] --out profiles/wtns_ingest_bench.txt"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench
import circom_compat_amd as cc

R = bench.R_MOD


def timed(fn, reps):
    fn()                                   # untimed pass
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(5, args.reps)
    rng = random.Random(2207)
    lines, ok = [], True
    with tempfile.TemporaryDirectory() as tmp:
        for k in [int(x) for x in args.sizes.split(",")]:
            mats, (A, B, Cm), w, n_vars = bench.chain_circuit(cc, k)
            pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, R) for _ in range(5)])
            path = os.path.join(tmp, f"chain{k}.wtns")
            cc.write_wtns(path, w)
            del w
            prover = cc.Prover(pk, mats, tables=0)
            r, s = cc.fr_from_ints([rng.randrange(R), rng.randrange(R)])
            old, p_old = timed(lambda: prover.prove(r, s, cc.read_wtns(path)), reps)
            new, p_new = timed(lambda: prover.prove_wtns(path, r, s), reps)
            equal = p_old.raw == p_new.raw
            t_map, wt = timed(lambda: cc.open_wtns(path), reps)
            t_up, ptr = timed(lambda: prover.upload_witness_canonical(wt), reps)
            t_proof, p_dev = timed(lambda: prover.prove_dev(r, s, ptr), reps)
            conv = []
            for _ in range(reps + 1):
                cc.fr_from_canonical(wt.canonical)
                conv.append(cc.fr_from_canonical_times()["convert"])
            faster = new["median_ms"] < old["median_ms"]
            ok = ok and equal and faster and p_dev.raw == p_old.raw
            lines.append(dict(circuit=f"chain{k}", n_vars=n_vars, tables=prover.info()["fixed_tables"], reps=reps, old=old,
                              new=new, speedup=round(old["median_ms"] / new["median_ms"], 2), bytes_equal=equal,
                              new_is_faster=faster,
                              breakdown_ms=dict(map=t_map["median_ms"], upload=t_up["median_ms"],
                                                convert_kernel=round(statistics.median(conv[1:]), 4),
                                                proof=t_proof["median_ms"])))
            print(json.dumps(lines[-1]), flush=True)
            prover.close()
            del wt, pk, prover
    if args.out:
        with open(args.out, "w") as f:
            f.write("# scripts/bench_wtns.py: read_wtns + prove (old) against prove_wtns (new), one process, same (r, s);\n"
                    "# host-timed milliseconds, median and range of %d passes after one untimed pass\n" % reps)
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
