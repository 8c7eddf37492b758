"""Batched proving (g16_prove_batch / g16_prove_batch_dev) against one proof at a time, on one MI355X.

For each circuit -- the reference bench family at 1000 x 1000 and 1000 x 10^4 (bench.complex_shape_circuit),
the reference bench's own circuit (bench.complex_circuit) and the squaring chain 2^14 -- with a trapdoor key
minted on the GPU and the library's automatic table rule (tables=0), and for each batch size B, one JSON line.
Bucket-path circuits: bchain15 .. bchain20 = squaring chains of 2^15 .. 2^20 constraints with tables=-1 (no
fixed-base tables: the sort / bucket MSMs); for them only the device-resident legs are timed unless --full.
--force-chunks: batch the bucket path above its size threshold as well (G16_BATCH_BUCKET_MAX_N, measurement
only) -- the data the threshold is read from.
  batch_dev / batch_host   ms per batch call and proofs/s, witnesses resident in HBM / from host memory
  loop                     prove_dev over the same resident inputs, one call per proof
  siblings                 two ctxs sharing the tables (g16_ctx_create_sibling), one host thread each
  bytes_equal              every batched proof == the loop's proof of the same inputs
    python scripts/bench_batch.py [--sizes 1,8,64,256,1024] [--reps 3] [--circuits ...] > profiles/<file>"""
import argparse
import json
import os
import random
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench
import circom_compat_amd as cc

R = bench.R_MOD


def chain_witness(x0, m):
    xs = [x0 % R]
    for _ in range(m):
        xs.append(xs[-1] * xs[-1] % R)
    return [1, xs[m]] + xs[:m]


def circuit(name):
    if name == "1000x1000":
        return bench.complex_shape_circuit(cc, 1000, 1000)
    if name == "1000x10000":
        return bench.complex_shape_circuit(cc, 1000, 10 ** 4)
    if name == "reference":
        return bench.complex_circuit(cc)
    if name == "chain14":
        return bench.chain_circuit(cc, 14)
    if name.startswith("bchain"):
        return bench.chain_circuit(cc, int(name[6:]))
    raise SystemExit(f"unknown circuit {name}")


def witnesses(name, n_vars, count, distinct=8):
    """`distinct` different satisfying witnesses, repeated up to `count` (the cost of a proof does not depend on
    the witness values: the repeat keeps host preparation short at B = 1024)"""
    if name == "reference":
        r1cs = cc.R1CS.from_file(os.path.join(ROOT, "tests", "golden", "complex-circuit-10000-10000.r1cs"))
        base = [cc.fr_from_ints(bench.solve_r1cs_forward(r1cs, {0: 1, 2: 3 + i})) for i in range(distinct)]
    else:
        m = n_vars - 2 if "chain" in name else 1000
        base = [cc.fr_from_ints(chain_witness(3 + i, m)) for i in range(distinct)]
    return np.ascontiguousarray(np.stack([base[i % distinct] for i in range(count)]))


def timed(fn, reps):
    fn()  # warm-up (first call of a size grows the batch workspace)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return min(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--circuits", default="1000x1000,1000x10000,reference,chain14")
    ap.add_argument("--full", action="store_true", help="bucket circuits: also the host-witness and sibling legs")
    ap.add_argument("--force-chunks", action="store_true", help="bucket circuits: chunks above the size threshold too")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    for name in args.circuits.split(","):
        t0 = time.perf_counter()
        mats, (A, B, Cm), _, n_vars = circuit(name)
        rng = random.Random(len(name))
        pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, R) for _ in range(5)])
        bucket = name.startswith("bchain")
        tables = -1 if bucket else 0
        lean = bucket and not args.full
        pr = cc.Prover(pk, mats, tables=tables)
        sib = cc.Prover(pk, mats, tables=tables, sibling_of=pr)
        info = pr.info()
        wall = witnesses(name, n_vars, max(sizes))
        w_dev = torch.from_numpy(wall.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        wb = n_vars * 32
        base = w_dev.data_ptr()
        line = dict(circuit=name, n_vars=n_vars, num_constraints=mats.num_constraints,
                    fixed_tables=info["fixed_tables"], batched=info["batched"], c_w=info["c_w"], D_w=info["D_w"],
                    setup_s=round(time.perf_counter() - t0, 2), rows=[])
        for count in sizes:
            rs = [tuple(v) for v in cc.fr_from_ints([rng.randrange(R) for _ in range(2 * count)]).reshape(count, 2, 4)]
            t_dev, got = timed(lambda: pr.prove_batch_dev(rs, base, count), args.reps)
            t_host, got_h = (t_dev, got) if lean else timed(lambda: pr.prove_batch(rs, wall[:count]), args.reps)
            t_loop, loop = timed(lambda: [pr.prove_dev(r, s, base + i * wb) for i, (r, s) in enumerate(rs)], args.reps)

            def two():
                half = (count + 1) // 2
                res = [None] * count

                def run(p, lo, hi):
                    for i in range(lo, hi):
                        res[i] = p.prove_dev(rs[i][0], rs[i][1], base + i * wb)
                th = threading.Thread(target=run, args=(sib, half, count))
                th.start()
                run(pr, 0, half)
                th.join()
                return res
            t_sib, sib_out = (t_loop, loop) if lean else timed(two, args.reps)
            ok = ([p.raw for p in got] == [p.raw for p in loop] and [p.raw for p in got_h] == [p.raw for p in loop]
                  and [p.raw for p in sib_out] == [p.raw for p in loop])
            row = dict(B=count,
                       batch_dev_ms=round(t_dev * 1e3, 3), batch_dev_proofs_per_s=round(count / t_dev, 1),
                       batch_host_ms=round(t_host * 1e3, 3), batch_host_proofs_per_s=round(count / t_host, 1),
                       loop_ms=round(t_loop * 1e3, 3), loop_proofs_per_s=round(count / t_loop, 1),
                       siblings_ms=round(t_sib * 1e3, 3), siblings_proofs_per_s=round(count / t_sib, 1),
                       batch_over_loop=round(t_loop / t_dev, 2), batch_over_siblings=round(t_sib / t_dev, 2),
                       bytes_equal=ok)
            if lean:  # not timed
                for k in ("batch_host_ms", "batch_host_proofs_per_s", "siblings_ms", "siblings_proofs_per_s",
                          "batch_over_siblings"):
                    row.pop(k)
            line["rows"].append(row)
            print(json.dumps(dict(circuit=name, **row)), file=sys.stderr, flush=True)
        print(json.dumps(line), flush=True)
        del w_dev
        sib.close()
        pr.close()


if __name__ == "__main__":
    if "--force-chunks" in sys.argv:
        os.environ["G16_BATCH_BUCKET_MAX_N"] = str(1 << 27)  # read once, when the first batch call is made
    main()
