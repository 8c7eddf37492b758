"""Aggregate batch verification (g16_verify_aggregate / cc.verify_aggregate / cc.verify_batch_fast): all
proofs of a batch under one key in ONE combined pairing check with coefficients rho_i,
  prod_i ML(B_i, rho_i A_i) ML(beta, -(sum rho_i) alpha) ML(gamma, -sum rho_i X_i) ML(delta, -sum rho_i C_i) -> 1.
Expected verdicts come from the oracle (oracle/bn254_ref.py), never from the library: _oracle_aggregate
evaluates the same equation for the same rho, o.verify_proof gives the per-proof truth."""
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_verify import _twist_point_outside_g2, _vk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 64            # lanes per block of the aggregate kernels
BIG = BLOCK + 3       # above one block, not a multiple of it: the in-block and the cross-block product passes
                      # and a partially filled last block (3 proof lanes + the 3 key lanes) all run


def _oracle_aggregate(opk, raws, pubs, rho):
    """the combined equation on the CPU, for well-formed proofs"""
    ic = opk["ic"]
    f = o.miller_loop(None, None)
    rho_sum, c_sum, x_sum = 0, None, None
    for raw, pub, k in zip(raws, pubs, rho):
        p = H.proof_from_bytes(raw)
        if not (o.G1.on_curve(p["a"]) and o.G1.on_curve(p["c"]) and o.G2.on_curve(p["b"])):
            return False
        f = o._f12_mul(f, o.miller_loop(p["b"], o.G1.mul(p["a"], k)))
        x = ic[0]
        for v, P in zip(pub, ic[1:]):
            x = o.G1.add(x, o.G1.mul(P, v % o.R_MOD))
        x_sum = o.G1.add(x_sum, o.G1.mul(x, k))
        c_sum = o.G1.add(c_sum, o.G1.mul(p["c"], k))
        rho_sum += k
    f = o._f12_mul(f, o.miller_loop(opk["beta_g2"], o.G1.neg(o.G1.mul(opk["alpha_g1"], rho_sum))))
    f = o._f12_mul(f, o.miller_loop(opk["gamma_g2"], o.G1.neg(x_sum)))
    f = o._f12_mul(f, o.miller_loop(opk["delta_g2"], o.G1.neg(c_sum)))
    return o.final_exponentiation(f) == o.miller_loop(None, None)


def _rho(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


_cache = {}


def _test_zkey_batch(lib, golden, n):
    """n proofs of test.zkey by the product prover: distinct witnesses [1, a b, a, b], distinct (r, s)"""
    import circom_compat_amd as cc
    key = (id(lib), n)
    if key not in _cache:
        data = open(os.path.join(golden, "test.zkey"), "rb").read()
        pk, mats = cc.read_zkey(data, lib=lib)
        opk, _ = o.read_zkey(data)
        rng = random.Random(n)
        ab = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in range(n)]
        ws = [[1, a * b % o.R_MOD, a, b] for a, b in ab]
        rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in range(n)]
        pr = cc.Prover(pk, mats, lib=lib, tables=1)
        raws = [p.raw for p in pr.prove_batch(rs, ws)]
        pr.close()
        assert len(set(raws)) == n
        _cache[key] = (_vk(cc, opk), opk, raws, [[w[1]] for w in ws])
    return _cache[key]


@pytest.mark.parametrize("n", [1, 2, 5])
def test_aggregate_accepts_valid_batches(lib, golden, n):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, n)
    rho = _rho(n, n)
    assert all(o.verify_proof(opk, p, H.proof_from_bytes(r)) for r, p in zip(raws, pubs))
    assert _oracle_aggregate(opk, raws, pubs, rho) is True
    assert cc.verify_aggregate(vk, raws, pubs, rho=rho, lib=lib) is True
    assert cc.verify_aggregate(vk, raws, pubs, lib=lib) is True                      # rho from the OS
    assert cc.verify_aggregate(vk, [cc.Proof(r) for r in raws], pubs, rho=rho, lib=lib) is True
    # the extreme coefficients: 1 and 2^128 - 1
    assert cc.verify_aggregate(vk, raws, pubs, rho=[1] * n, lib=lib) is True
    assert cc.verify_aggregate(vk, raws, pubs, rho=[(1 << 128) - 1] * n, lib=lib) is True
    # one wrong public input: the oracle's helper and the library both reject
    bad = [list(p) for p in pubs]
    bad[-1][0] = (bad[-1][0] + 1) % o.R_MOD
    assert _oracle_aggregate(opk, raws, bad, rho) is False
    assert cc.verify_aggregate(vk, raws, bad, rho=rho, lib=lib) is False


def test_aggregate_above_one_block(lib, golden):
    """BIG proofs: accepted with drawn and with explicit coefficients; one wrong public input is found at the
    first index, the last, the last lane of the first block and the first lane of the second; so is an A that
    is another curve point"""
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, BIG)
    rho = _rho(7, BIG)
    assert o.verify_proof(opk, pubs[BLOCK], H.proof_from_bytes(raws[BLOCK]))
    assert cc.verify_aggregate(vk, raws, pubs, lib=lib) is True
    ok, structural = cc.verify_aggregate(vk, raws, pubs, rho=rho, lib=lib, return_structural=True)
    assert ok is True and structural == [True] * BIG
    for pos in (0, BIG - 1, BLOCK - 1, BLOCK):
        bad = [list(p) for p in pubs]
        bad[pos][0] = (bad[pos][0] + 1) % o.R_MOD
        assert cc.verify_aggregate(vk, raws, bad, rho=rho, lib=lib) is False, pos
    swapped = list(raws)
    swapped[BLOCK + 1] = o.g1_to_bytes(o.G1_GEN) + raws[BLOCK + 1][64:]
    ok, structural = cc.verify_aggregate(vk, swapped, pubs, rho=rho, lib=lib, return_structural=True)
    assert ok is False and structural == [True] * BIG                                # well formed, just wrong


def test_aggregate_coefficients_are_used(lib, golden):
    """Why rho must not be known to the prover: against a KNOWN rho two invalid proofs that cancel in
    sum rho_i C_i are forged from valid ones (C_0' = C_0 + rho_1 D, C_1' = C_1 - rho_0 D).  Each is invalid on its
    own; the batch passes under exactly that rho (oracle and library: this pins the equation, not only the
    verdict) and fails under any other."""
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 2)
    rho = _rho(31, 2)
    D = o.G1.mul(o.G1_GEN, 0xD15EA5E)
    c0 = o.G1.add(o.g1_from_bytes(raws[0][192:]), o.G1.mul(D, rho[1]))
    c1 = o.G1.add(o.g1_from_bytes(raws[1][192:]), o.G1.neg(o.G1.mul(D, rho[0])))
    forged = [raws[0][:192] + o.g1_to_bytes(c0), raws[1][:192] + o.g1_to_bytes(c1)]
    for raw, pub in zip(forged, pubs):
        assert not o.verify_proof(opk, pub, H.proof_from_bytes(raw))
    assert cc.verify_batch(vk, forged, pubs, lib=lib) == [False, False]
    assert _oracle_aggregate(opk, forged, pubs, rho) is True
    assert cc.verify_aggregate(vk, forged, pubs, rho=rho, lib=lib) is True
    other = _rho(32, 2)
    assert other != rho and _oracle_aggregate(opk, forged, pubs, other) is False
    assert cc.verify_aggregate(vk, forged, pubs, rho=other, lib=lib) is False
    assert cc.verify_aggregate(vk, forged, pubs, rho=[rho[1], rho[0]], lib=lib) is False
    assert cc.verify_aggregate(vk, forged, pubs, lib=lib) is False                   # drawn by the library


def _malformed_batch(lib, golden):
    """the malformed proofs of test_verify_batch_rejects_what_deserialisation_rejects and of
    test_verify_batch_on_the_reference_zkey between valid ones; (vk, opk, batch, pubs, indices of the malformed)"""
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 5)
    good = raws[0]
    T = _twist_point_outside_g2(1)
    cof = good[:64] + o.g2_to_bytes(T) + good[192:]
    B = H.proof_from_bytes(good)["b"]
    mixed = good[:64] + o.g2_to_bytes(o.G2.add(B, o.G2.mul(T, o.R_MOD))) + good[192:]

    def plus_q(raw, off):
        v = int.from_bytes(raw[off:off + 32], "little") + o.Q_MOD
        assert v < 1 << 256
        return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]
    noncanon = [plus_q(good, off) for off in (0, 32, 64, 160, 192, 224)]
    off = bytearray(good)
    off[0] ^= 1
    bad = [cof, mixed] + noncanon + [bytes(off)]
    batch = [raws[0]] + bad[:2] + [raws[1]] + bad[2:5] + [raws[2], raws[3]] + bad[5:] + [raws[4]]
    bpubs = [pubs[0]] + [pubs[0]] * 2 + [pubs[1]] + [pubs[0]] * 3 + [pubs[2], pubs[3]] + [pubs[0]] * (len(bad) - 5) + [pubs[4]]
    where = [i for i, r in enumerate(batch) if r not in raws]
    assert len(where) == len(bad) == 9 and len(batch) == 14
    return vk, opk, batch, bpubs, where


def test_aggregate_structural_rejects(lib, golden):
    import circom_compat_amd as cc
    vk, opk, batch, pubs, where = _malformed_batch(lib, golden)
    rho = _rho(5, len(batch))
    ok, structural = cc.verify_aggregate(vk, batch, pubs, rho=rho, lib=lib, return_structural=True)
    assert ok is False
    assert structural == [i not in where for i in range(len(batch))]
    keep = [i for i in range(len(batch)) if i not in where]
    ok, structural = cc.verify_aggregate(vk, [batch[i] for i in keep], [pubs[i] for i in keep],
                                         rho=[rho[i] for i in keep], lib=lib, return_structural=True)
    assert ok is True and structural == [True] * len(keep)


def test_aggregate_edges(lib, golden):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 2)
    assert cc.verify_aggregate(vk, [], [], lib=lib) is True
    assert cc.verify_aggregate(vk, [], [], rho=[], lib=lib, return_structural=True) == (True, [])
    # the all-infinity proof alone: whatever verify_batch (and the oracle) say about it
    inf = bytes(256)
    want = cc.verify_batch(vk, [inf], [pubs[0]], lib=lib)[0]
    assert want == bool(o.verify_proof(opk, pubs[0], H.proof_from_bytes(inf)))
    assert cc.verify_aggregate(vk, [inf], [pubs[0]], rho=[12345], lib=lib, return_structural=True) == (want, [True])
    for kw in (dict(rho=[5, 0]), dict(rho=[5]), dict(rho=[5, 6, 7]), dict(rho=[5, 1 << 128]), dict(rho=[5, -1])):
        with pytest.raises(cc.G16Error) as e:
            cc.verify_aggregate(vk, raws, pubs, lib=lib, **kw)
        assert e.value.status == B.G16_ERR_INVALID, kw
    with pytest.raises(cc.G16Error) as e:
        cc.verify_aggregate(vk, raws, [pubs[0], pubs[1] + [1]], lib=lib)
    assert e.value.status == B.G16_ERR_INVALID
    with pytest.raises(cc.G16Error):
        cc.verify_aggregate(vk, raws, pubs[:1], lib=lib)
    # the C ABI itself refuses a zero coefficient
    import ctypes as C
    d, buf, pb, n, _ic = cc._verify_args(vk, raws, pubs, lib)
    rho = np.array([[5, 0], [0, 0]], dtype=np.uint64)
    ok = np.full(1, 7, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.g16_verify_aggregate(0, C.byref(d), ptr(buf), ptr(pb), n, ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    rho[1, 1] = 1                                                                    # 2^64: non-zero in the high word only
    assert lib.g16_verify_aggregate(0, C.byref(d), ptr(buf), ptr(pb), n, ptr(rho), ptr(ok), None) == B.G16_OK
    assert ok[0] == 1


@pytest.mark.parametrize("n_pub", [0, 3])
def test_aggregate_public_input_counts(lib, n_pub):
    """no public inputs (sum rho_i X_i = (sum rho_i) IC_0) and several, on a trapdoor key as in
    test_verify_batch_public_input_counts: three proofs of different witnesses"""
    import circom_compat_amd as cc
    P = o.R_MOD
    m = 3
    base = 1 + n_pub
    n_vars = base + m + 1
    cons = [([(base + i, 1)], [(base + i, 1)], [(base + i + 1, 1)]) for i in range(m)]
    rng = random.Random(100 + n_pub)
    tox = [rng.randrange(1, P) for _ in range(5)]
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *tox)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
    pr = cc.Prover(H.pk_from_oracle(opk), mats, lib=lib)
    raws, pubs = [], []
    for k in range(3):
        w = [1] + [rng.randrange(P) for _ in range(n_pub)] + [3 + k]
        for _ in range(m):
            w.append(w[-1] * w[-1] % P)
        raws.append(pr.prove(rng.randrange(P), rng.randrange(P), w).raw)
        pubs.append(w[1:1 + n_pub])
    vk = _vk(cc, opk)
    rho = _rho(n_pub, 3)
    assert all(o.verify_proof(opk, p, H.proof_from_bytes(r)) for r, p in zip(raws, pubs))
    assert _oracle_aggregate(opk, raws, pubs, rho) is True
    assert cc.verify_aggregate(vk, raws, pubs, rho=rho, lib=lib) is True
    assert cc.verify_aggregate(vk, raws, pubs, lib=lib) is True
    for j in range(n_pub):                                                           # every column is summed
        bad = [list(p) for p in pubs]
        bad[j % 3][j] = (bad[j % 3][j] + 1) % P
        assert cc.verify_aggregate(vk, raws, bad, rho=rho, lib=lib) is False, j
    if n_pub == 0:                                                                   # one statement: any order is valid
        assert cc.verify_aggregate(vk, raws[::-1], pubs, rho=rho, lib=lib) is True
    else:                                                                            # proofs 0 and 2 beside the wrong inputs
        assert cc.verify_aggregate(vk, raws[::-1], pubs, rho=rho, lib=lib) is False


def test_verify_batch_fast_equals_verify_batch(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 5)
    assert cc.verify_batch_fast(vk, raws, pubs, lib=lib) == cc.verify_batch(vk, raws, pubs, lib=lib) == [True] * 5
    bad = [list(p) for p in pubs]
    for i in (1, 4):
        bad[i][0] = (bad[i][0] + 1) % o.R_MOD
    want = [bool(o.verify_proof(opk, p, H.proof_from_bytes(r))) for r, p in zip(raws, bad)]
    assert want == [True, False, True, True, False]
    assert cc.verify_batch_fast(vk, raws, bad, lib=lib) == cc.verify_batch(vk, raws, bad, lib=lib) == want
    vk, opk, batch, bpubs, where = _malformed_batch(lib, golden)
    want = [i not in where for i in range(len(batch))]
    assert cc.verify_batch_fast(vk, batch, bpubs, lib=lib) == cc.verify_batch(vk, batch, bpubs, lib=lib) == want
    assert cc.verify_batch_fast(vk, [], [], lib=lib) == []


def test_aggregate_is_deterministic(lib, golden):
    """same batch, same coefficients: same verdict, valid or not"""
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 5)
    rho = _rho(77, 5)
    bad = [list(p) for p in pubs]
    bad[2][0] = (bad[2][0] + 1) % o.R_MOD
    for _ in range(2):
        assert cc.verify_aggregate(vk, raws, pubs, rho=rho, lib=lib) is True
        assert cc.verify_aggregate(vk, raws, bad, rho=rho, lib=lib) is False


@pytest.mark.gpu
def test_aggregate_after_prove_batch_gpu(gpulib):
    """the use the feature is for: prove_batch of 300 proofs on the table path (squaring chain 2^10, distinct
    inputs), then ONE check of the whole batch; one changed public input turns it False and verify_batch_fast
    names it"""
    import circom_compat_amd as cc
    sys.path.insert(0, ROOT)
    import bench
    count = 300
    mats, (A, Bm, Cm), _, n_vars = bench.chain_circuit(cc, 10)
    m = n_vars - 2
    rng = random.Random(4242)
    pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
    pr = cc.Prover(pk, mats, tables=0)
    assert pr.info()["fixed_tables"] == 1
    w_ints = []
    for _ in range(count):
        xs = [rng.randrange(2, o.R_MOD)]
        for _ in range(m):
            xs.append(xs[-1] * xs[-1] % o.R_MOD)
        w_ints.append([1, xs[m]] + xs[:m])
    warr = np.stack([cc.fr_from_ints(w) for w in w_ints])
    rs = [(rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)) for _ in range(count)]
    proofs = pr.prove_batch(rs, warr)
    pr.close()
    pubs = [[w[1]] for w in w_ints]
    vk_dict = dict(alpha_g1=o.g1_from_bytes(bytes(pk.vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(pk.vk.beta_g2)),
                   gamma_g2=o.g2_from_bytes(bytes(pk.vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(pk.vk.delta_g2)),
                   ic=[o.g1_from_bytes(bytes(x)) for x in pk.vk.gamma_abc_g1])
    assert o.verify_proof(vk_dict, pubs[-1], H.proof_from_bytes(proofs[-1].raw))
    rho = _rho(1, count)
    assert cc.verify_aggregate(pk.vk, proofs, pubs, lib=gpulib) is True
    assert cc.verify_aggregate(pk.vk, proofs, pubs, rho=rho, lib=gpulib) is True
    bad = [list(p) for p in pubs]
    bad[200][0] = (bad[200][0] + 1) % o.R_MOD
    assert cc.verify_aggregate(pk.vk, proofs, bad, lib=gpulib) is False
    assert cc.verify_aggregate(pk.vk, proofs, bad, rho=rho, lib=gpulib) is False
    assert cc.verify_batch_fast(pk.vk, proofs, bad, lib=gpulib) == [i != 200 for i in range(count)]
    assert cc.verify_batch_fast(pk.vk, proofs, pubs, lib=gpulib) == [True] * count
