"""Batched proving: many witnesses under one key (g16_prove_batch / g16_prove_batch_dev / g16_witness_map_batch).

Proof i of a batch equals, byte for byte, what g16_prove returns for (r_i, s_i, w_i): on table-path ctxs a chunk
goes through every kernel in one pass (grid.y / grid.z = proof index), on the other ctxs the call loops over the
single-proof path."""
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vk_dict(pk):
    return dict(alpha_g1=o.g1_from_bytes(bytes(pk.vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(pk.vk.beta_g2)),
                gamma_g2=o.g2_from_bytes(bytes(pk.vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(pk.vk.delta_g2)),
                ic=[o.g1_from_bytes(bytes(x)) for x in pk.vk.gamma_abc_g1])


def _chain_witness(x0, m):
    """bench.chain_circuit / complex_shape_circuit wire order for another input: [1, x_m, x_0, .., x_{m-1}]"""
    xs = [x0 % o.R_MOD]
    for _ in range(m):
        xs.append(xs[-1] * xs[-1] % o.R_MOD)
    return [1, xs[m]] + xs[:m]


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_prove_batch_test_zkey_vs_oracle(lib, golden, monkeypatch):
    """The reference's zkey on the table path: five witnesses [1, a b, a, b] and five distinct (r, s), among them
    (0, 0) and (r - 1, r - 1).  Every batched proof == the oracle's == prove(); the same batch again with the
    free device memory forced so low that every chunk holds one proof gives the same bytes, and so does a
    bucket-path ctx (the fallback loop)."""
    import circom_compat_amd as cc
    pk, mats = cc.read_zkey(os.path.join(golden, "test.zkey"), lib=lib)
    opk, omats = o.read_zkey(open(os.path.join(golden, "test.zkey"), "rb").read())
    ab = [(3, 11), (5, 7), (0, 9), (o.R_MOD - 1, 2), (123456789, 987654321)]
    ws = [[1, a * b % o.R_MOD, a, b] for a, b in ab]
    rs = [(3413513218498352040262653353725127729454431939539290118844322056224532443637,
           6077776500692565155461894309070795882353485867345896979329447163197530625403), (0, 0), (5, 0),
          (o.R_MOD - 1, o.R_MOD - 1), (17, 19)]
    want = [o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(opk, r, s, omats, 2, 1, w))
            for (r, s), w in zip(rs, ws)]
    pr = cc.Prover(pk, mats, lib=lib, tables=1)
    assert pr.info()["fixed_tables"] == 1
    got = pr.prove_batch(rs, ws)
    assert [p.raw for p in got] == want
    assert [pr.prove(r, s, w).raw for (r, s), w in zip(rs, ws)] == want
    # a (count, n_vars, 4) Montgomery array is the same input
    warr = np.stack([cc.fr_from_ints(w, lib) for w in ws])
    assert [p.raw for p in pr.prove_batch(rs, warr)] == want
    # chunks of one proof (the chunk rule sees almost no free memory): the loop over chunks
    monkeypatch.setenv("G16_EMU_FREE_BYTES", "1")
    assert [p.raw for p in pr.prove_batch(rs, ws)] == want
    monkeypatch.delenv("G16_EMU_FREE_BYTES")
    assert [p.raw for p in pr.prove_batch(rs[1:4], ws[1:4])] == want[1:4]
    # a sibling keeps its own batch workspace and borrows the tables
    sib = cc.Prover(pk, mats, lib=lib, sibling_of=pr, tables=0)
    assert [p.raw for p in sib.prove_batch(rs, ws)] == want
    sib.close()
    # bucket path: the fallback loop, same bytes
    never = cc.Prover(pk, mats, lib=lib, tables=-1)
    assert never.info()["fixed_tables"] == 0
    assert [p.raw for p in never.prove_batch(rs, ws)] == want
    never.close()
    pr.close()


@pytest.mark.parametrize("red", ["circom", "libsnark"])
def test_prove_batch_circuits_vs_oracle(lib, golden, red):
    """More than one row: a squaring chain (circom reduction) with distinct inputs x0, and LibsnarkReduction on
    the reference's mycircuit.r1cs with distinct (a, b) -- the batched coset NTTs and k_libsnark_* kernels."""
    import circom_compat_amd as cc
    rng = random.Random(31337 + len(red))
    if red == "circom":
        cases = [H.squaring_chain(3, x0=x0) for x0 in (3, 5, 2 ** 200 + 7)]
        cons, _, n_vars, n_pub = cases[0]
        ws = [c[1] for c in cases]
    else:
        r1 = o.read_r1cs(open(os.path.join(golden, "mycircuit.r1cs"), "rb").read())
        cons, n_vars, n_pub = r1["constraints"], r1["n_wires"], r1["num_inputs"] - 1
        ws = [[1, a * b % o.R_MOD, a, b] for a, b in ((3, 11), (4, 4), (o.R_MOD - 2, 77))]
    tox = [rng.randrange(1, o.R_MOD) for _ in range(5)]
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *tox, reduction=red)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
    pr = cc.Prover(H.pk_from_oracle(opk), mats, lib=lib, tables=1, reduction=red)
    assert pr.info()["fixed_tables"] == 1
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in ws]
    want = [o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(
        opk, r, s, dict(a=a_rows, b=b_rows), n_pub + 1, len(cons), w, reduction=red)) for (r, s), w in zip(rs, ws)]
    assert [p.raw for p in pr.prove_batch(rs, ws)] == want
    pr.close()


def _row_class_matrices(rng):
    """rows of every SpMV class (spmv.h): 1 term, 4 | 5, 64 | 65, an empty A row, one row of more than 64 terms"""
    P = o.R_MOD
    n_w = 48
    lens = [(1, 1), (4, 4), (5, 1), (1, 5), (64, 64), (65, 1), (1, 65), (0, 3), (130, 7), (2, 3)]

    def lc(k):
        return [(0 if (j == 0 and k > 4) else rng.randrange(2, n_w),
                 1 if rng.random() < 0.4 else rng.randrange(P)) for j in range(k)]
    cons = [(lc(la), lc(lb), [(2, 1)]) for la, lb in lens]
    return cons, n_w


def test_witness_map_batch_row_classes_vs_oracle(lib):
    """g16_witness_map_batch on a witness-map-only ctx over rows of every SpMV class: the batched k_spmv_abc,
    k_spmv_medium, k_spmv_tasks / k_spmv_huge, NTTs and k_mul_sub.  Three distinct assignments; each h ==
    the oracle's witness_map_from_matrices == g16_witness_map."""
    import circom_compat_amd as cc
    rng = random.Random(777)
    cons, n_w = _row_class_matrices(rng)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    mats = H.matrices_from_rows(a_rows, b_rows, 2, n_w, lib)
    ws = [[1] + [rng.randrange(o.R_MOD) for _ in range(n_w - 1)] for _ in range(3)]
    pr = cc.Prover(None, mats, lib=lib, n_vars=n_w)
    h = pr.witness_map_batch(ws)
    assert h.shape == (3, pr.domain_size, 4)
    for i, w in enumerate(ws):
        want = o.witness_map_from_matrices(a_rows, b_rows, 2, len(cons), w)
        assert H.fr_from_mont_arr(h[i]) == want, i
        assert np.array_equal(h[i], pr.witness_map(w))
    pr.close()


def test_prove_batch_errors(lib, golden):
    """A wrong n_vars and a dist_wm ctx are errors; count 0 returns [] and writes nothing."""
    import circom_compat_amd as cc
    pk, mats = cc.read_zkey(os.path.join(golden, "test.zkey"), lib=lib)
    pr = cc.Prover(pk, mats, lib=lib, tables=1)
    assert pr.prove_batch([], []) == []
    with pytest.raises(cc.G16Error):
        pr.prove_batch([(1, 2)], [[1, 33, 3, 11, 5]])
    with pytest.raises(cc.G16Error):
        pr.witness_map_batch([[1, 33, 3]])
    pr.close()
    dist = cc.Prover(pk, mats, lib=lib, rank=0, world=2, dist_wm=True)
    with pytest.raises(cc.G16Error) as e:
        dist.prove_batch([(1, 2)], [[1, 33, 3, 11]])
    assert "dist_wm" in str(e.value) or "world" in str(e.value)
    with pytest.raises(cc.G16Error):
        dist.witness_map_batch([[1, 33, 3, 11]])
    dist.close()


# ---- GPU ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("logm", [10, 13, 14])
def test_prove_batch_chains_gpu(gpulib, logm):
    """Squaring chains with a GPU-minted key on the table path (tables=0), B = 1, 7, 64 with distinct x0 and
    (r, s): every proof == prove(); first and last == the CPU restatement; one pairing-verifies and a wrong
    public input is rejected."""
    import circom_compat_amd as cc
    import cpu_ref
    bench = _bench()
    mats, (A, B, Cm), _, n_vars = bench.chain_circuit(cc, logm)
    m = n_vars - 2
    rng = random.Random(900 + logm)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=0)
    assert pr.info()["fixed_tables"] == 1
    for count in (1, 7, 64):
        w_ints = [_chain_witness(rng.randrange(2, o.R_MOD), m) for _ in range(count)]
        warr = np.stack([cc.fr_from_ints(w) for w in w_ints])
        rs = [tuple(cc.fr_from_ints([rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)])) for _ in range(count)]
        got = pr.prove_batch(rs, warr)
        assert [p.raw for p in got] == [pr.prove(r, s, warr[i]).raw for i, (r, s) in enumerate(rs)]
        for i in {0, count - 1}:
            r, s = rs[i]
            assert got[i].raw == cpu_ref.prove(pk, mats, r.reshape(1, 4).copy(), s.reshape(1, 4).copy(), warr[i])
    assert o.verify_proof(_vk_dict(pk), [w_ints[-1][1]], H.proof_from_bytes(got[-1].raw))
    assert not o.verify_proof(_vk_dict(pk), [(w_ints[-1][1] + 1) % o.R_MOD], H.proof_from_bytes(got[-1].raw))
    pr.close()


@pytest.mark.gpu
def test_prove_batch_reference_bench_circuit_gpu(gpulib):
    """The reference bench's circuit (complex-circuit-10000-10000.r1cs) with 16 inputs a: batch == the loop."""
    import circom_compat_amd as cc
    bench = _bench()
    mats, (A, B, Cm), _, n_vars = bench.complex_circuit(cc)
    r1cs = cc.R1CS.from_file(os.path.join(ROOT, "tests", "golden", "complex-circuit-10000-10000.r1cs"))
    rng = random.Random(16)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=0)
    assert pr.info()["fixed_tables"] == 1
    warr = np.stack([cc.fr_from_ints(bench.solve_r1cs_forward(r1cs, {0: 1, 2: a})) for a in range(3, 19)])
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in range(16)]
    got = pr.prove_batch(rs, warr)
    assert [p.raw for p in got] == [pr.prove(r, s, warr[i]).raw for i, (r, s) in enumerate(rs)]
    pr.close()


@pytest.mark.gpu
def test_prove_batch_dev_from_torch_gpu(gpulib):
    """g16_prove_batch_dev with the witnesses in a torch device tensor == g16_prove_batch."""
    import torch
    import circom_compat_amd as cc
    bench = _bench()
    mats, (A, B, Cm), _, n_vars = bench.chain_circuit(cc, 10)
    rng = random.Random(7)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=0)
    warr = np.stack([cc.fr_from_ints(_chain_witness(x0, n_vars - 2)) for x0 in range(5, 25)])
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in range(20)]
    t = torch.from_numpy(warr.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    dev = pr.prove_batch_dev(rs, t.data_ptr(), 20)
    assert [p.raw for p in dev] == [p.raw for p in pr.prove_batch(rs, warr)]
    del t
    pr.close()


@pytest.mark.gpu
def test_prove_batch_fallback_ctxs_gpu(gpulib):
    """Ctxs without tables loop over the single-proof path: a bucket-path ctx (tables=-1, chain 2^12) and a
    devices=[0, 0] ctx.  Batch == the loop of prove()."""
    import circom_compat_amd as cc
    bench = _bench()
    mats, (A, B, Cm), _, n_vars = bench.chain_circuit(cc, 12)
    rng = random.Random(12)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    warr = np.stack([cc.fr_from_ints(_chain_witness(x0, n_vars - 2)) for x0 in (3, 4, 5, 6)])
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in range(4)]
    for kw in (dict(tables=-1), dict(devices=[0, 0], tables=-1)):
        pr = cc.Prover(pk, mats, **kw)
        assert pr.info()["fixed_tables"] == 0
        loop = [pr.prove(r, s, warr[i]).raw for i, (r, s) in enumerate(rs)]
        assert [p.raw for p in pr.prove_batch(rs, warr)] == loop, kw
        pr.close()


@pytest.mark.gpu
def test_prove_batch_crosses_chunk_cap_gpu(gpulib):
    """B = 300 on the 1000 x 1000 circuit: more proofs than one chunk holds (cap 256) -> two chunks; == the loop."""
    import circom_compat_amd as cc
    bench = _bench()
    mats, (A, B, Cm), _, n_vars = bench.complex_shape_circuit(cc, 1000, 1000)
    rng = random.Random(300)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=0)
    assert pr.info()["fixed_tables"] == 1
    warr = np.stack([cc.fr_from_ints(_chain_witness(x0, n_vars - 2)) for x0 in range(3, 303)])
    rs = [tuple(v) for v in cc.fr_from_ints([rng.randrange(o.R_MOD) for _ in range(600)]).reshape(300, 2, 4)]
    got = pr.prove_batch(rs, warr)
    assert [p.raw for p in got] == [pr.prove(r, s, warr[i]).raw for i, (r, s) in enumerate(rs)]
    pr.close()
