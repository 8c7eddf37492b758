"""Batched proving on the bucket path (ctxs without fixed-base tables): a chunk of g16_prove_batch is ONE sort, one
accumulation and one reduction per MSM for every proof of the chunk (proof z's buckets are z nb + set B + digit),
and the finalisation kernels take the proof index from the grid.  Proof i must equal, byte for byte, what
g16_prove returns for (r_i, s_i, w_i) -- and the oracle's proof."""
import json
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT, REDUCE = "msm_sort", "msm_reduce"
ACC = ("msm_accumulate_g1", "msm_accumulate_g2", "msm_accumulate_g1_pair", "msm_fixup")


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _chain_witness(x0, m):
    """bench.chain_circuit wire order for another input: [1, x_m, x_0, .., x_{m-1}]"""
    xs = [x0 % o.R_MOD]
    for _ in range(m):
        xs.append(xs[-1] * xs[-1] % o.R_MOD)
    return [1, xs[m]] + xs[:m]


def _launches(pr, fn):
    """what fn() returns, and the stage launch counts of that call (profiling on)"""
    pr.set_profiling(True)
    pr.stage_times()
    out = fn()
    t = pr.stage_times()
    pr.set_profiling(False)
    return out, {k: v[1] for k, v in t.items()}


def _oracle_case(cons, n_vars, n_pub, seed, red="circom"):
    rng = random.Random(seed)
    tox = [rng.randrange(1, o.R_MOD) for _ in range(5)]
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *tox, reduction=red)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    want = lambda r, s, w: o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(
        opk, r, s, dict(a=a_rows, b=b_rows), n_pub + 1, len(cons), w, reduction=red))
    return opk, a_rows, b_rows, want


def _check(pr, rs, ws, want):
    """batch == the oracle's proofs == prove() one at a time"""
    assert [p.raw for p in pr.prove_batch(rs, ws)] == want
    assert [pr.prove(r, s, w).raw for (r, s), w in zip(rs, ws)] == want


def _is_emu(lib):
    return os.path.basename(lib.path or "").startswith("libg16_emu")


def test_bucket_ctx_is_batched(lib, golden):
    """info()["batched"]: set on a bucket-path ctx and on a table ctx"""
    import circom_compat_amd as cc
    pk, mats = cc.read_zkey(os.path.join(golden, "test.zkey"), lib=lib)
    for tables in (-1, 1):
        pr = cc.Prover(pk, mats, lib=lib, tables=tables)
        assert pr.info()["fixed_tables"] == (tables == 1)
        assert pr.info()["batched"] == 1
        pr.close()


def test_chunk_launch_counts_do_not_grow(lib, golden):
    """With profiling on, the sort, accumulation and reduction stages of a B = 6 batch count as many launches as
    those of a B = 1 batch (one loop iteration per proof would give 6x); the proofs still equal the loop's."""
    import circom_compat_amd as cc
    pk, mats = cc.read_zkey(os.path.join(golden, "test.zkey"), lib=lib)
    pr = cc.Prover(pk, mats, lib=lib, tables=-1)
    ws = [[1, a * b % o.R_MOD, a, b] for a, b in ((3, 11), (2, 9), (5, 5), (7, 1), (0, 4), (13, 17))]
    rs = [(17 + i, 1000 + 7 * i) for i in range(6)]
    one, c1 = _launches(pr, lambda: pr.prove_batch(rs[:1], ws[:1]))
    six, c6 = _launches(pr, lambda: pr.prove_batch(rs, ws))
    assert c1[SORT] > 0 and c1[REDUCE] > 0
    for k in (SORT, REDUCE) + ACC:
        assert c6[k] == c1[k], (k, c1[k], c6[k])
    assert [p.raw for p in six] == [pr.prove(r, s, w).raw for (r, s), w in zip(rs, ws)]
    assert six[0].raw == one[0].raw
    pr.close()


def test_bucket_batch_test_zkey_vs_oracle(lib, golden, monkeypatch):
    """The reference's zkey: five witnesses and five (r, s), among them (0, 0) and (r - 1, r - 1); every batched
    proof == the oracle's == prove().  On the emulator also: a count that is no multiple of the chunk (the free
    memory the chunk rule sees is raised until a chunk holds more than one proof but fewer than five -- told by
    the sort launches: one per chunk), chunks of one (G16_EMU_FREE_BYTES=1); then a sibling ctx, which keeps its
    own batch workspace and borrows the planes."""
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
    pr = cc.Prover(pk, mats, lib=lib, tables=-1)
    assert pr.info()["fixed_tables"] == 0 and pr.info()["batched"] == 1
    _check(pr, rs, ws, want)
    if _is_emu(lib):
        _, c1 = _launches(pr, lambda: pr.prove_batch(rs[:1], ws[:1]))
        free = 1 << 12
        while True:
            monkeypatch.setenv("G16_EMU_FREE_BYTES", str(free))
            got, c5 = _launches(pr, lambda: pr.prove_batch(rs, ws))
            assert [p.raw for p in got] == want
            chunks = c5[SORT] // c1[SORT]
            if chunks < 5:
                break
            free *= 2
        assert chunks in (2, 3), chunks  # chunks of 2 (2 + 2 + 1) or of 3 / 4 (3 + 2, 4 + 1)
        monkeypatch.setenv("G16_EMU_FREE_BYTES", "1")  # chunks of one: the single-proof enqueue per proof
        got, c5 = _launches(pr, lambda: pr.prove_batch(rs, ws))
        assert c5[SORT] == 5 * c1[SORT]
        assert [p.raw for p in got] == want
        monkeypatch.delenv("G16_EMU_FREE_BYTES")
    sib = cc.Prover(pk, mats, lib=lib, sibling_of=pr, tables=-1)
    assert sib.info()["batched"] == 1
    assert [p.raw for p in sib.prove_batch(rs[::-1], ws[::-1])] == want[::-1]
    assert [p.raw for p in pr.prove_batch(rs[1:4], ws[1:4])] == want[1:4]
    sib.close()
    pr.close()


@pytest.mark.parametrize("red", ["circom", "libsnark"])
def test_bucket_batch_circuit2_vs_oracle(lib, golden, red):
    """circuit2.r1cs with both reductions: the safe-circuit witness and two variants of it"""
    import circom_compat_amd as cc
    r1 = o.read_r1cs(open(os.path.join(golden, "circuit2.r1cs"), "rb").read())
    cons, n_vars, n_pub = r1["constraints"], r1["n_wires"], r1["num_inputs"] - 1
    w0 = [int(x) % o.R_MOD for x in json.load(open(os.path.join(golden, "safe-circuit-witness.json")))]
    assert len(w0) == n_vars
    rng = random.Random(2 + len(red))
    ws = [w0]
    for _ in range(2):  # other private values (an unsatisfied assignment has a proof all the same)
        w = list(w0)
        for j in rng.sample(range(n_pub + 1, n_vars), 5):
            w[j] = rng.randrange(o.R_MOD)
        ws.append(w)
    opk, a_rows, b_rows, want_of = _oracle_case(cons, n_vars, n_pub, 41 + len(red), red)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
    pr = cc.Prover(H.pk_from_oracle(opk), mats, lib=lib, tables=-1, reduction=red)
    assert pr.info()["batched"] == 1
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in ws]
    _check(pr, rs, ws, [want_of(r, s, w) for (r, s), w in zip(rs, ws)])
    pr.close()


@pytest.mark.parametrize("wb,planes", [(5, 3), (9, 0)])
def test_bucket_batch_windows_vs_oracle(lib, wb, planes):
    """Forced windows: 3 planes of c = 5 give D = 18 bucket sets per MSM (k_horner per proof on grid.y), full
    planes of c = 9 (29 windows) give D = 1"""
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub = H.squaring_chain(6, x0=3)
    ws = [w] + [H.squaring_chain(6, x0=x0)[1] for x0 in (5, 2 ** 130 + 1, 0)]
    opk, a_rows, b_rows, want_of = _oracle_case(cons, n_vars, n_pub, 5 + wb)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
    pr = cc.Prover(H.pk_from_oracle(opk), mats, lib=lib, tables=-1, window_bits=wb, planes=planes)
    info = pr.info()
    assert info["c_w"] == wb and (info["D_w"] > 1) == (planes == 3), info
    rng = random.Random(wb)
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in ws]
    _check(pr, rs, ws, [want_of(r, s, x) for (r, s), x in zip(rs, ws)])
    pr.close()


def test_bucket_batch_dense_skewed_and_zero_witness_vs_oracle(lib):
    """helpers.dense_skewed_circuit (most scalars 0 / 1: hot buckets, whose entries span lanes, repeat in every proof
    of the chunk), a variant of its witness, and a witness whose private part is all zero (every bucket of that
    proof empty)"""
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub = H.dense_skewed_circuit(120, seed=3, long_rows=(40,))
    rng = random.Random(77)
    w2 = list(w)
    for j in rng.sample(range(2, n_vars), 10):
        w2[j] = 0 if w2[j] == 1 else 1
    ws = [w, w2, [1, 0] + [0] * (n_vars - 2)]
    opk, a_rows, b_rows, want_of = _oracle_case(cons, n_vars, n_pub, 12)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
    pr = cc.Prover(H.pk_from_oracle(opk), mats, lib=lib, tables=-1, window_bits=4)
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in ws]
    _check(pr, rs, ws, [want_of(r, s, x) for (r, s), x in zip(rs, ws)])
    pr.close()


# ---- GPU ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_bucket_batch_poseidon_2_16_sparse_b_gpu(gpulib):
    """bench.poseidon_chain_circuit at 2^16 (the filtered B view active), B = 16 with distinct (r, s): every proof ==
    the loop's; four pairing-verify"""
    import circom_compat_amd as cc
    bench = _bench()
    mats, (A, B, Cm), w_int, n_vars = bench.poseidon_chain_circuit(cc, 16)
    rng = random.Random(1616)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=-1)
    info = pr.info()
    assert info["sparse_b"] == 1 and info["batched"] == 1 and info["fixed_tables"] == 0, info
    warr = np.stack([cc.fr_from_ints(w_int)] * 16)
    rs = [tuple(v) for v in cc.fr_from_ints([rng.randrange(o.R_MOD) for _ in range(32)]).reshape(16, 2, 4)]
    got = pr.prove_batch(rs, warr)
    assert [p.raw for p in got] == [pr.prove(r, s, warr[i]).raw for i, (r, s) in enumerate(rs)]
    assert len({p.raw for p in got}) == 16
    assert all(cc.verify_batch(pk.vk, got[:4], [[w_int[1]]] * 4))
    pr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("logm,count", [(15, 64), (18, 8)])
def test_bucket_batch_chains_gpu(gpulib, logm, count):
    """Squaring chains (distinct inputs and (r, s)) on the bucket path: batch == the loop, byte for byte; the first
    and last pairing-verify and a wrong public input is rejected"""
    import circom_compat_amd as cc
    bench = _bench()
    mats, (A, B, Cm), _, n_vars = bench.chain_circuit(cc, logm)
    m = n_vars - 2
    rng = random.Random(1800 + logm)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=-1)
    assert pr.info()["batched"] == 1 and pr.info()["fixed_tables"] == 0
    w_ints = [_chain_witness(rng.randrange(2, o.R_MOD), m) for _ in range(count)]
    warr = np.stack([cc.fr_from_ints(w) for w in w_ints])
    rs = [tuple(v) for v in cc.fr_from_ints([rng.randrange(o.R_MOD) for _ in range(2 * count)]).reshape(count, 2, 4)]
    got = pr.prove_batch(rs, warr)
    assert [p.raw for p in got] == [pr.prove(r, s, warr[i]).raw for i, (r, s) in enumerate(rs)]
    assert all(cc.verify_batch(pk.vk, [got[0], got[-1]], [[w_ints[0][1]], [w_ints[-1][1]]]))
    assert not any(cc.verify_batch(pk.vk, [got[0]], [[(w_ints[0][1] + 1) % o.R_MOD]]))
    pr.close()
