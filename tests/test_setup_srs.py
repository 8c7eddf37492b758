"""Groth16 setup from a powers-of-tau string on the GPU: cc.trapdoor_srs (g16_srs_create), cc.setup_from_srs
(g16_setup_from_srs) and cc.check_key_circuit.

The key computed from the SRS of (tau, alpha, beta) is, byte for byte, the trapdoor key of (tau, alpha, beta, 1, 1):
canonical affine encodings are unique.  Expected bytes come from the oracle (oracle/bn254_ref.py: G1.mul, G2.mul for
the SRS, trapdoor_setup for the key) and, at sizes where forming points in Python takes too long, from the library's
own trapdoor generator, which tests/test_kernels.py::test_trapdoor_setup_vs_oracle pins to the oracle.

Time limits of the GPU cases: the transforms cost about 255 doublings and 85 additions per butterfly, (n / 2) log n
butterflies per transform, five transforms: ~3 10^9 field multiplications at 2^12 and ~8 10^10 at 2^16, well under a
second of kernel time either way; the trapdoor key it is compared with is cheaper.  The limits below (60 s and 120 s
for both keys together) are hang guards two orders of magnitude above that, not performance gates."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

R = o.R_MOD
QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")
UNCHANGED_MISMATCH, PAIR_L = 1, 4
D1 = 0x1D0C0FFEE0DDBA11F00D5EED0FACADE5C0DEC0DE1234567890ABCDEF13579BDF % R


def _same_key(a, b):
    """every field of two ProvingKeys, as bytes"""
    assert (a.n_vars, a.n_public, a.domain_size) == (b.n_vars, b.n_public, b.domain_size)
    for name in ("beta_g1", "delta_g1"):
        assert bytes(getattr(a, name)) == bytes(getattr(b, name)), name
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert bytes(getattr(a.vk, name)) == bytes(getattr(b.vk, name)), name
    assert np.array_equal(np.asarray(a.vk.gamma_abc_g1), np.asarray(b.vk.gamma_abc_g1)), "gamma_abc_g1"
    for q in QUERIES:
        x, y = np.asarray(getattr(a, q)), np.asarray(getattr(b, q))
        assert x.shape == y.shape, q
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert bad.size == 0, (q, bad[:8])


def _clone(cc, pk):
    vk = cc.VerifyingKey(bytes(pk.vk.alpha_g1), bytes(pk.vk.beta_g2), bytes(pk.vk.gamma_g2), bytes(pk.vk.delta_g2),
                         np.array(pk.vk.gamma_abc_g1, dtype=np.uint8, copy=True))
    return cc.ProvingKey(pk.n_vars, pk.n_public, pk.domain_size, vk, bytes(pk.beta_g1), bytes(pk.delta_g1),
                         *(np.array(getattr(pk, q), dtype=np.uint8, copy=True) for q in QUERIES))


def _csrs(cc, cons, lib):
    return tuple(cc.Csr.from_rows([[(cf, idx) for idx, cf in row[j]] for row in cons], lib) for j in range(3))


def _tox3(seed):
    rng = random.Random(seed)
    return [rng.randrange(2, R) for _ in range(3)]


def _wide_circuit(m=20, n_pub=3, n_vars=40, seed=9):
    """m rows over n_vars wires with n_pub public inputs: domain 32 < 40 wires; every wire occurs"""
    rng = random.Random(seed)
    cons = []
    for i in range(m):
        lc = lambda k: [(w, rng.randrange(1, R)) for w in rng.sample(range(n_vars), k)]
        cons.append((lc(3) + [(i % n_vars, 1)], lc(2) + [((2 * i + 1) % n_vars, 5)], lc(2) + [((i + 20) % n_vars, 7)]))
    return cons, n_vars, n_pub


def _mixed_circuit(k, n_pub=2, seed=5):
    """2^k - n_pub - 1 rows (domain exactly 2^k) over 2^k wires.  The constant wire 0 is in the A side of EVERY row
    (the long-row class) and in some B and C sides; the last wire is in no row (its query entries are infinity);
    coefficients are drawn from 1, r - 1, small integers of either sign and full-width values."""
    rng = random.Random(seed)
    m = (1 << k) - n_pub - 1
    n_vars = 1 << k
    used = n_vars - 1

    def coeff():
        kind = rng.randrange(6)
        if kind == 0:
            return 1
        if kind == 1:
            return R - 1
        if kind == 2:
            return rng.randrange(2, 1 << 16)
        if kind == 3:
            return R - rng.randrange(2, 1 << 16)
        if kind == 4:
            return rng.randrange(1 << 31, 1 << 33)
        return rng.randrange(1, R)

    def lc(n):
        return [(w, coeff()) for w in rng.sample(range(1, used), n)]

    cons = []
    for i in range(m):
        a = [(0, coeff())] + lc(2) + [(1 + i % (used - 1), 1)]
        b = lc(2) + ([(0, coeff())] if i % 3 == 0 else [])
        c = lc(1) + ([(0, R - 1)] if i % 5 == 0 else [])
        cons.append((a, b, c))
    return cons, n_vars, n_pub


def _py_srs(cc, log2_domain, tox):
    """the SRS of (tau, alpha, beta) from the oracle's scalar multiplications"""
    tau, alpha, beta = tox
    n = 1 << log2_domain
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    g1 = lambda s: o.g1_to_bytes(o.G1.mul(o.G1_GEN, s % R))
    g2 = lambda s: o.g2_to_bytes(o.G2.mul(o.G2_GEN, s % R))
    arr = lambda bs, w: np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(-1, w)
    return cc.Srs(arr([g1(p) for p in pw], 64), arr([g2(p) for p in pw[:n]], 128),
                  arr([g1(alpha * p) for p in pw[:n]], 64), arr([g1(beta * p) for p in pw[:n]], 64), g2(beta))


def _same_srs(a, b):
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.beta_g2 == b.beta_g2


_py_cache = {}


def _cached_py_srs(cc, log2_domain, seed):
    if (log2_domain, seed) not in _py_cache:
        _py_cache[(log2_domain, seed)] = _py_srs(cc, log2_domain, _tox3(seed))
    return _py_cache[(log2_domain, seed)]


# ---- 1. oracle exactness ---------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_oracle_key_wide_circuit(lib, reduction):
    """several public inputs, more wires (40) than domain points (32): SRS and expected key both from the oracle"""
    import circom_compat_amd as cc
    cons, n_vars, n_pub = _wide_circuit()
    tox = _tox3(31)
    srs = _cached_py_srs(cc, 5, 31)
    want = H.pk_from_oracle(o.trapdoor_setup(cons, n_vars, n_pub, *tox, 1, 1, reduction=reduction))
    assert want.domain_size == 32 and want.n_vars == 40
    got = cc.setup_from_srs(*_csrs(cc, cons, lib), n_vars, n_pub, srs, lib=lib, reduction=reduction)
    _same_key(got, want)
    if reduction == "libsnark":
        assert not got.h_query[-1].any()


@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_oracle_key_domain_8(lib, reduction):
    import circom_compat_amd as cc
    cons, _w, n_vars, n_pub = H.squaring_chain(3)
    tox = _tox3(32)
    srs = _cached_py_srs(cc, 3, 32)
    want = H.pk_from_oracle(o.trapdoor_setup(cons, n_vars, n_pub, *tox, 1, 1, reduction=reduction))
    assert want.domain_size == 8
    _same_key(cc.setup_from_srs(*_csrs(cc, cons, lib), n_vars, n_pub, srs, lib=lib, reduction=reduction), want)


# ---- 2. the SRS generator ----------------------------------------------------------------------------
@pytest.mark.parametrize("log2_domain,seed", [(3, 32), (5, 31)])
def test_trapdoor_srs_vs_oracle(lib, log2_domain, seed):
    import circom_compat_amd as cc
    srs = cc.trapdoor_srs(log2_domain, _tox3(seed), lib=lib)
    n = 1 << log2_domain
    assert srs.tau_g1.shape == (2 * n - 1, 64) and srs.tau_g2.shape == (n, 128)
    assert srs.alpha_tau_g1.shape == srs.beta_tau_g1.shape == (n, 64)
    _same_srs(srs, _cached_py_srs(cc, log2_domain, seed))


# ---- 3. trapdoor equivalence at size -------------------------------------------------------------------
def _equivalence(cc, lib, k, reduction, seed=77):
    cons, n_vars, n_pub = _mixed_circuit(k)
    csrs = _csrs(cc, cons, lib)
    tox = _tox3(seed)
    srs = cc.trapdoor_srs(k, tox, lib=lib)
    t0 = time.perf_counter()
    got = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib, reduction=reduction)
    t1 = time.perf_counter()
    want = cc.trapdoor_setup(*csrs, n_vars, n_pub, tox + [1, 1], lib=lib, reduction=reduction)
    t2 = time.perf_counter()
    print(f"setup_from_srs 2^{k} {reduction}: {t1 - t0:.3f} s (trapdoor_setup {t2 - t1:.3f} s) "
          f"phases {cc.setup_from_srs_times(lib)}")
    assert got.domain_size == 1 << k
    _same_key(got, want)
    # the wire in no row: infinity in every query; the constant wire's entries are proper points
    assert not got.a_query[-1].any() and not got.b_g1_query[-1].any() and not got.b_g2_query[-1].any()
    assert not got.l_query[-1].any()
    assert got.a_query[0].any() and got.b_g2_query[0].any()
    return t2 - t0


@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_trapdoor_equivalence_2_6(lib, reduction):
    import circom_compat_amd as cc
    _equivalence(cc, lib, 6, reduction)


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_trapdoor_equivalence_2_12_gpu(gpulib, reduction):
    import circom_compat_amd as cc
    assert _equivalence(cc, gpulib, 12, reduction) < 60.0


@pytest.mark.gpu
def test_trapdoor_equivalence_2_16_gpu(gpulib):
    import circom_compat_amd as cc
    assert _equivalence(cc, gpulib, 16, "circom") < 120.0


# ---- 4. the full chain ---------------------------------------------------------------------------------
_chain = {}


def _chain_keys(cc, lib):
    """(circuit csrs, witness, n_vars, srs, fresh, key1) of the squaring chain at 2^6"""
    if id(lib) not in _chain:
        cons, w, n_vars, n_pub = H.squaring_chain(6)
        csrs = _csrs(cc, cons, lib)
        srs = cc.trapdoor_srs(6, _tox3(55), lib=lib)
        fresh = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib)
        _chain[id(lib)] = (cons, csrs, w, n_vars, n_pub, srs, fresh, cc.contribute_key(fresh, D1, lib=lib))
    return _chain[id(lib)]


def test_full_chain(lib):
    import circom_compat_amd as cc
    cons, csrs, w, n_vars, n_pub, srs, fresh, key1 = _chain_keys(cc, lib)
    _same_key(key1, cc.trapdoor_setup(*csrs, n_vars, n_pub, _tox3(55) + [1, D1], lib=lib))
    assert cc.check_contribution(fresh, key1, lib=lib).ok
    assert cc.check_key(key1, lib=lib).ok
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    pr = cc.Prover(key1, H.matrices_from_rows(a_rows, b_rows, 2, n_vars, lib), lib=lib)
    proof = pr.prove(1234567, 7654321, w)
    pr.close()
    assert cc.verify_batch(key1.vk, [proof], [w[1:2]], lib=lib) == [True]
    assert cc.verify_batch(key1.vk, [proof], [[(w[1] + 1) % R]], lib=lib) == [False]


# ---- 5. circuit binding --------------------------------------------------------------------------------
def test_check_key_circuit(lib):
    import circom_compat_amd as cc
    cons, csrs, w, n_vars, n_pub, srs, fresh, key1 = _chain_keys(cc, lib)
    rep = cc.check_key_circuit(key1, *csrs, srs, lib=lib)
    assert rep.ok and rep.failed is None and rep.contribution.ok and rep.describe() == "ok"
    assert cc.check_key_circuit(fresh, *csrs, srs, lib=lib).ok

    # the same circuit with one coefficient of a private wire changed
    wire, cf = cons[10][0][0]
    other = list(cons)
    other[10] = ([(wire, (cf + 1) % R)], cons[10][1], cons[10][2])
    key_other = cc.contribute_key(cc.setup_from_srs(*_csrs(cc, other, lib), n_vars, n_pub, srs, lib=lib), D1, lib=lib)
    assert cc.check_key(key_other, lib=lib).ok                    # well formed, but of another circuit
    rep = cc.check_key_circuit(key_other, *csrs, srs, lib=lib)
    assert not rep.ok and rep.failed == "contribution"
    assert rep.contribution.relations_failed & UNCHANGED_MISMATCH
    assert "contribution" in rep.describe()

    # one l_query point replaced
    bad = _clone(cc, key1)
    bad.l_query[7] = np.frombuffer(o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE)), dtype=np.uint8)
    rep = cc.check_key_circuit(bad, *csrs, srs, lib=lib)
    assert not rep.ok and rep.failed == "contribution" and rep.contribution.relations_failed == PAIR_L

    # IC replaced
    bad = _clone(cc, key1)
    bad.vk.gamma_abc_g1[1] = np.frombuffer(o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xBEEF)), dtype=np.uint8)
    rep = cc.check_key_circuit(bad, *csrs, srs, lib=lib)
    assert not rep.ok and rep.failed == "gamma_abc_g1" and rep.contribution is None
    assert "gamma_abc_g1" in rep.describe()


# ---- 6. arguments ----------------------------------------------------------------------------------------
def test_arguments(lib):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    cons, csrs, w, n_vars, n_pub, srs, fresh, key1 = _chain_keys(cc, lib)

    def status(s, reduction="circom"):
        try:
            cc.setup_from_srs(*csrs, n_vars, n_pub, s, lib=lib, reduction=reduction)
        except cc.G16Error as e:
            return e.status
        return B.G16_OK

    assert srs.tau_g1.shape[0] == 127 and srs.tau_g2.shape[0] == 64
    short_g1 = cc.Srs(srs.tau_g1[:-1], srs.tau_g2, srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2)
    short_g2 = cc.Srs(srs.tau_g1, srs.tau_g2[:-1], srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2)
    assert status(short_g1) == B.G16_ERR_INVALID
    assert status(short_g2) == B.G16_ERR_INVALID
    assert status(srs) == B.G16_OK
    # a bad reduction and NULL arguments, through the C ABI
    empty = B.Csr()
    d = srs.to_c()
    h = C.c_void_p()
    cat, cbt, cct = (m.to_c() for m in cc._setup_matrices(*csrs, n_vars, n_pub, lib))
    call = lambda *a: lib.g16_setup_from_srs(0, *a, C.byref(h))
    assert call(C.byref(cat), C.byref(cbt), C.byref(cct), n_vars, n_pub, len(cons), C.byref(d), 7) == B.G16_ERR_INVALID
    assert call(C.byref(cat), C.byref(cbt), C.byref(cct), n_vars, n_pub, len(cons), None, 0) == B.G16_ERR_INVALID
    assert call(None, C.byref(cbt), C.byref(cct), n_vars, n_pub, len(cons), C.byref(d), 0) == B.G16_ERR_INVALID
    # the domain limit fires on the sizes alone: no array exists here
    none = B.SrsDesc()
    st = call(C.byref(empty), C.byref(empty), C.byref(empty), 1 << 27, 0, 1 << 27, C.byref(none), 0)
    assert st == B.G16_ERR_DOMAIN_TOO_LARGE
    with pytest.raises(cc.SynthesisError):
        cc.trapdoor_srs(28, _tox3(1), lib=lib)
    # a longer SRS than needed: the same key as the exact-length one
    longer = cc.trapdoor_srs(7, _tox3(55), lib=lib)
    assert longer.tau_g1.shape[0] == 255
    _same_key(cc.setup_from_srs(*csrs, n_vars, n_pub, longer, lib=lib), fresh)


# ---- 7. repeatability --------------------------------------------------------------------------------------
def test_repeatable(lib):
    import circom_compat_amd as cc
    cons, n_vars, n_pub = _mixed_circuit(6, seed=8)
    csrs = _csrs(cc, cons, lib)
    srs = cc.trapdoor_srs(6, _tox3(3), lib=lib)
    _same_srs(srs, cc.trapdoor_srs(6, _tox3(3), lib=lib))
    _same_key(cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib), cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib))
