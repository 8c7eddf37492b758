"""Powers-of-tau contributions on the GPU: cc.contribute_srs (g16_srs_contribute) and cc.new_srs.

A contribution (t, a, b) turns the string of (tau, alpha, beta) into the string of (tau t, alpha a, beta b): entry i of
tau_g1 / tau_g2 times t^i, of alpha_tau_g1 times a t^i, of beta_tau_g1 times b t^i, beta_g2 times b.  Canonical affine
encodings are unique, so every comparison here is of bytes: with the oracle's scalar multiplications
(oracle/bn254_ref.py: G1.mul, G2.mul) at 2^3, and with cc.trapdoor_srs of the product trapdoor at the larger sizes --
tests/test_setup_srs.py::test_trapdoor_srs_vs_oracle pins trapdoor_srs to the oracle.

A string of 2^k has 2 2^k - 1 / 2^k / 2^k G1 points and 2^k G2 points; the sizes are the smallest that reach each seam
(G16_SRSCONTRIB_CHUNK sets the points per staged chunk; the shared inversion runs over groups of 8 x 64 points)."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, Q = o.R_MOD, o.Q_MOD
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
CHUNK_ENV = "G16_SRSCONTRIB_CHUNK"
D1 = 0x1D0C0FFEE0DDBA11F00D5EED0FACADE5C0DEC0DE1234567890ABCDEF13579BDF % R


def _secrets(seed, n=3):
    rng = random.Random(seed)
    return [rng.randrange(2, R) for _ in range(n)]


def _prod(x, y):
    return [p * q % R for p, q in zip(x, y)]


def _same_srs(a, b):
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape, name
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8])
    assert a.beta_g2 == b.beta_g2, "beta_g2"


def _copy_srs(cc, s):
    out = cc.Srs(*(np.array(getattr(s, n), dtype=np.uint8, copy=True) for n in ARRAYS), bytes(s.beta_g2))
    out.power, out.ceremony_power = s.power, s.ceremony_power
    return out


_minted = {}


def _trapdoor(cc, lib, k, tox):
    """cc.trapdoor_srs, minted once per library and trapdoor; callers do not write to it"""
    key = (id(lib), k, tuple(tox))
    if key not in _minted:
        _minted[key] = cc.trapdoor_srs(k, list(tox), lib=lib)
    return _minted[key]


def _neg_g1(row):
    p = o.g1_from_bytes(bytes(row))
    return np.frombuffer(o.g1_to_bytes((p[0], Q - p[1])), dtype=np.uint8)


def _neg_g2(row):
    x, (y0, y1) = o.g2_from_bytes(bytes(row))
    return np.frombuffer(o.g2_to_bytes((x, ((Q - y0) % Q, (Q - y1) % Q))), dtype=np.uint8)


# ---- 1. oracle bytes ---------------------------------------------------------------------------------------
def test_oracle_bytes_2_3(lib):
    import circom_compat_amd as cc
    tox, (t, a, b) = _secrets(301), _secrets(302)
    srs = _trapdoor(cc, lib, 3, tox)
    before = _copy_srs(cc, srs)
    got = cc.contribute_srs(srs, (t, a, b), lib=lib)
    assert got.tau_g1.shape == (15, 64) and got.tau_g2.shape == (8, 128)
    assert got.alpha_tau_g1.shape == got.beta_tau_g1.shape == (8, 64)
    for name, c in (("tau_g1", 1), ("alpha_tau_g1", a), ("beta_tau_g1", b)):
        for i, row in enumerate(getattr(srs, name)):
            want = o.g1_to_bytes(o.G1.mul(o.g1_from_bytes(bytes(row)), c * pow(t, i, R) % R))
            assert bytes(getattr(got, name)[i]) == want, (name, i)
    for i, row in enumerate(srs.tau_g2):
        want = o.g2_to_bytes(o.G2.mul(o.g2_from_bytes(bytes(row)), pow(t, i, R)))
        assert bytes(got.tau_g2[i]) == want, ("tau_g2", i)
    assert bytes(got.tau_g1[0]) == o.g1_to_bytes(o.G1_GEN)
    assert bytes(got.tau_g2[0]) == o.g2_to_bytes(o.G2_GEN)
    assert got.beta_g2 == o.g2_to_bytes(o.G2.mul(o.g2_from_bytes(srs.beta_g2), b))
    _same_srs(srs, before)                                                   # the input is not written


# ---- 2. trapdoor equivalence -------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 24, 20])
def test_trapdoor_equivalence_2_5(lib, monkeypatch, chunk):
    """default chunk; 24: 63 = 24 + 24 + 15 and 32 = 24 + 8, ragged ends; 20: no multiple of the 8-point run"""
    import circom_compat_amd as cc
    if chunk is None:
        monkeypatch.delenv(CHUNK_ENV, raising=False)
    else:
        monkeypatch.setenv(CHUNK_ENV, str(chunk))
    tox, sec = _secrets(501), _secrets(502)
    got = cc.contribute_srs(_trapdoor(cc, lib, 5, tox), sec, lib=lib)
    assert got.tau_g1.shape[0] == 63 and got.tau_g2.shape[0] == 32
    _same_srs(got, _trapdoor(cc, lib, 5, _prod(tox, sec)))


# ---- 3. edge scalars and points ----------------------------------------------------------------------------
def test_edge_scalars_2_3(lib):
    import circom_compat_amd as cc
    tox = _secrets(303)
    srs = _trapdoor(cc, lib, 3, tox)
    _same_srs(cc.contribute_srs(srs, (1, 1, 1), lib=lib), srs)

    # t = r - 1: t^i = (-1)^i, P at even and -P (same x, y -> q - y) at odd indices
    got = cc.contribute_srs(srs, (R - 1, 1, 1), lib=lib)
    for name in ARRAYS:
        neg = _neg_g2 if name == "tau_g2" else _neg_g1
        for i, row in enumerate(getattr(srs, name)):
            want = neg(row) if i & 1 else row
            assert np.array_equal(getattr(got, name)[i], want), (name, i)
    assert got.beta_g2 == srs.beta_g2

    # a = b = r - 1: every alpha / beta entry negated, beta_g2 too, the tau arrays as they were
    got = cc.contribute_srs(srs, (1, R - 1, R - 1), lib=lib)
    assert np.array_equal(got.tau_g1, srs.tau_g1) and np.array_equal(got.tau_g2, srs.tau_g2)
    for name in ("alpha_tau_g1", "beta_tau_g1"):
        for i, row in enumerate(getattr(srs, name)):
            assert np.array_equal(getattr(got, name)[i], _neg_g1(row)), (name, i)
    assert got.beta_g2 == bytes(_neg_g2(np.frombuffer(srs.beta_g2, dtype=np.uint8)))

    # long runs of one bits and of zero bits
    ones, sparse = ((1 << 253) - 1) % R, 1 << 200
    for sec in ((ones, sparse, ones), (sparse, ones, sparse)):
        _same_srs(cc.contribute_srs(srs, sec, lib=lib), _trapdoor(cc, lib, 3, _prod(tox, sec)))


def test_infinity_stays_infinity_2_3(lib, monkeypatch):
    """the all-zero entry at the first index, the last index and on both sides of a chunk seam of each array"""
    import circom_compat_amd as cc
    monkeypatch.setenv(CHUNK_ENV, "5")                                       # 15 = 5 + 5 + 5, 8 = 5 + 3
    tox, sec = _secrets(304), _secrets(305)
    srs = _trapdoor(cc, lib, 3, tox)
    want = _trapdoor(cc, lib, 3, _prod(tox, sec))
    holed = _copy_srs(cc, srs)
    holes = {name: (0, 4, 5, len(getattr(srs, name)) - 1) for name in ARRAYS}
    for name, idx in holes.items():
        getattr(holed, name)[list(idx)] = 0
    got = cc.contribute_srs(holed, sec, lib=lib)
    for name, idx in holes.items():
        for i in range(len(getattr(srs, name))):
            if i in idx:
                assert not getattr(got, name)[i].any(), (name, i)
            else:
                assert np.array_equal(getattr(got, name)[i], getattr(want, name)[i]), (name, i)
    assert got.beta_g2 == want.beta_g2
    # beta_g2 at infinity
    holed = cc.Srs(srs.tau_g1, srs.tau_g2, srs.alpha_tau_g1, srs.beta_tau_g1, bytes(128))
    got = cc.contribute_srs(holed, sec, lib=lib)
    assert got.beta_g2 == bytes(128)
    assert np.array_equal(got.beta_tau_g1, want.beta_tau_g1)


# ---- 4. composition ------------------------------------------------------------------------------------------
def test_composition_2_4(lib):
    import circom_compat_amd as cc
    tox, s1, s2 = _secrets(401), _secrets(402), _secrets(403)
    srs = _trapdoor(cc, lib, 4, tox)
    twice = cc.contribute_srs(cc.contribute_srs(srs, s1, lib=lib), s2, lib=lib)
    _same_srs(twice, cc.contribute_srs(srs, _prod(s1, s2), lib=lib))
    _same_srs(twice, _trapdoor(cc, lib, 4, _prod(tox, _prod(s1, s2))))
    fresh = cc.new_srs(4, lib=lib)
    _same_srs(fresh, _trapdoor(cc, lib, 4, (1, 1, 1)))
    assert all(bytes(p) == o.g1_to_bytes(o.G1_GEN) for p in fresh.tau_g1)
    assert all(bytes(p) == o.g2_to_bytes(o.G2_GEN) for p in fresh.tau_g2)
    _same_srs(cc.contribute_srs(fresh, s1, lib=lib), _trapdoor(cc, lib, 4, s1))


# ---- 5. a ceremony end to end --------------------------------------------------------------------------------
def test_ceremony_end_to_end_2_6(lib):
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub = H.squaring_chain(6)
    csrs = tuple(cc.Csr.from_rows([[(cf, idx) for idx, cf in row[j]] for row in cons], lib) for j in range(3))
    s1, s2 = _secrets(601), _secrets(602)
    srs = cc.contribute_srs(cc.contribute_srs(cc.new_srs(6, lib=lib), s1, lib=lib), s2, lib=lib)
    d = srs.to_c()
    rng = random.Random(603)
    rho = [rng.randrange(1, 1 << 128) for _ in range((d.n_tau_g1 - 1) + 3 * (d.n_tau - 1))]
    rep = cc.check_srs(srs, rho=rho, lib=lib)
    assert rep.ok, rep.describe()
    fresh = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib)
    want = cc.trapdoor_setup(*csrs, n_vars, n_pub, _prod(s1, s2) + [1, 1], lib=lib)
    for name in ("beta_g1", "delta_g1"):
        assert bytes(getattr(fresh, name)) == bytes(getattr(want, name)), name
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert bytes(getattr(fresh.vk, name)) == bytes(getattr(want.vk, name)), name
    assert np.array_equal(np.asarray(fresh.vk.gamma_abc_g1), np.asarray(want.vk.gamma_abc_g1))
    for q in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query"):
        assert np.array_equal(np.asarray(getattr(fresh, q)), np.asarray(getattr(want, q))), q
    key1 = cc.contribute_key(fresh, D1, lib=lib)
    rep = cc.check_key_circuit(key1, *csrs, srs, lib=lib)
    assert rep.ok, rep.describe()
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    pr = cc.Prover(key1, H.matrices_from_rows(a_rows, b_rows, 2, n_vars, lib), lib=lib)
    proof = pr.prove(1234567, 7654321, w)
    pr.close()
    assert cc.verify_batch(key1.vk, [proof], [w[1:2]], lib=lib) == [True]


# ---- 6. drawn secrets ------------------------------------------------------------------------------------------
def test_drawn_secrets_2_3(lib):
    import circom_compat_amd as cc
    srs = _trapdoor(cc, lib, 3, _secrets(306))
    before = _copy_srs(cc, srs)
    x, y = cc.contribute_srs(srs, lib=lib), cc.contribute_srs(srs, None, lib=lib)
    for name in ("tau_g2", "alpha_tau_g1", "beta_tau_g1"):
        assert not np.array_equal(getattr(x, name), getattr(y, name)), name
        assert not np.array_equal(getattr(x, name), getattr(srs, name)), name
    assert not np.array_equal(x.tau_g1[1:], y.tau_g1[1:]) and x.beta_g2 != y.beta_g2
    assert cc.check_srs(x, lib=lib).ok and cc.check_srs(y, lib=lib).ok
    _same_srs(srs, before)


# ---- 7. in place, through the C ABI ----------------------------------------------------------------------------
def test_in_place_2_5(lib, monkeypatch):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    monkeypatch.setenv(CHUNK_ENV, "24")
    tox, sec = _secrets(503), _secrets(504)
    want = cc.contribute_srs(_trapdoor(cc, lib, 5, tox), sec, lib=lib)
    work = _copy_srs(cc, _trapdoor(cc, lib, 5, tox))
    d = work.to_c()
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
    st = lib.g16_srs_contribute(0, C.byref(d), ptr(H.fr_mont_arr(sec)), ptr(work.tau_g1), ptr(work.tau_g2),
                                ptr(work.alpha_tau_g1), ptr(work.beta_tau_g1), d.beta_g2)
    assert st == B.G16_OK
    work.beta_g2 = bytes(d.beta_g2)
    _same_srs(work, want)


# ---- 8. .ptau round trip ---------------------------------------------------------------------------------------
def test_ptau_round_trip_2_3(lib, tmp_path):
    import circom_compat_amd as cc
    got = cc.contribute_srs(cc.new_srs(3, lib=lib), _secrets(307), lib=lib)
    path = tmp_path / "contributed.ptau"
    cc.write_ptau(path, got, lib=lib)
    back = cc.read_ptau(path, lib=lib)
    assert back.power == 3
    _same_srs(back, got)
    # power / ceremony_power of a string that was read from a file are carried over
    again = cc.contribute_srs(back, _secrets(308), lib=lib)
    assert (again.power, again.ceremony_power) == (back.power, back.ceremony_power)


# ---- 9. arguments ------------------------------------------------------------------------------------------------
def test_arguments_2_3(lib):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    srs = _trapdoor(cc, lib, 3, _secrets(309))
    good = H.fr_mont_arr(_secrets(310))
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
    FILL = 0xA5
    outs = [np.full(getattr(srs, n).shape, FILL, dtype=np.uint8) for n in ARRAYS]
    bg2 = (C.c_uint8 * 128)(*([FILL] * 128))

    def call(desc=None, secrets=good, drop=None):
        d = srs.to_c() if desc is None else desc
        args = [ptr(x) for x in outs] + [bg2]
        if drop is not None:
            args[drop] = None
        st = lib.g16_srs_contribute(0, C.byref(d), ptr(secrets) if secrets is not None else None, *args)
        untouched = all((x == FILL).all() for x in outs) and all(v == FILL for v in bg2)
        return st, untouched

    r_words = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint64)
    for which in range(3):
        zero = good.copy()
        zero[which] = 0
        assert call(secrets=zero) == (B.G16_ERR_INVALID, True), which
        big = good.copy()
        big[which] = r_words                                                 # the words of r itself: not below r
        assert call(secrets=big) == (B.G16_ERR_INVALID, True), which
        big[which] = 0xFFFFFFFFFFFFFFFF
        assert call(secrets=big) == (B.G16_ERR_INVALID, True), which
    for drop in range(5):
        assert call(drop=drop) == (B.G16_ERR_INVALID, True), drop
    for field in ("n_tau_g1", "n_tau"):
        d = srs.to_c()
        setattr(d, field, 0)
        assert call(desc=d) == (B.G16_ERR_INVALID, True), field
    for field in ARRAYS:
        d = srs.to_c()
        setattr(d, field, None)
        assert call(desc=d) == (B.G16_ERR_INVALID, True), field
    assert lib.g16_srs_contribute(0, None, ptr(good), *[ptr(x) for x in outs], bg2) == B.G16_ERR_INVALID
    # the binding refuses the same before it calls: the values, and the number of them
    for bad in ((0, 1, 1), (1, R, 1), (1, 1, R + 5), (1, 1, -1), (2, 3), (2, 3, 4, 5), ()):
        with pytest.raises(cc.G16Error) as e:
            cc.contribute_srs(srs, bad, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID, bad
    empty = cc.Srs(srs.tau_g1, srs.tau_g2[:0], srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2)
    with pytest.raises(cc.G16Error) as e:
        cc.contribute_srs(empty, (2, 3, 4), lib=lib)
    assert e.value.status == B.G16_ERR_INVALID
    # and the good call goes through with the same arguments
    assert call() == (B.G16_OK, False)


# ---- 10. repeatability -------------------------------------------------------------------------------------------
def test_repeatable_2_5(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv(CHUNK_ENV, "24")
    srs, sec = _trapdoor(cc, lib, 5, _secrets(505)), _secrets(506)
    _same_srs(cc.contribute_srs(srs, sec, lib=lib), cc.contribute_srs(srs, sec, lib=lib))


# ---- 11. GPU only ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,chunk", [(12, None), (16, 5000)])
def test_trapdoor_equivalence_gpu(gpulib, monkeypatch, k, chunk):
    """2^12 at the default chunk (one chunk per array); 2^16 in chunks of 5000 (27 / 14 chunks, ragged ends, and
    groups of the shared inversion cut by every seam)"""
    import circom_compat_amd as cc
    if chunk is None:
        monkeypatch.delenv(CHUNK_ENV, raising=False)
    else:
        monkeypatch.setenv(CHUNK_ENV, str(chunk))
    tox, sec = _secrets(1100 + k), _secrets(1200 + k)
    got = cc.contribute_srs(cc.trapdoor_srs(k, tox, lib=gpulib), sec, lib=gpulib)
    print(f"contribute_srs 2^{k}: device ms per phase {cc.contribute_srs_times(gpulib)}")
    _same_srs(got, cc.trapdoor_srs(k, _prod(tox, sec), lib=gpulib))


@pytest.mark.gpu
def test_live_prover_is_untouched_gpu(gpulib):
    """a Prover alive on the device proves the same bytes before and after contribute_srs calls on that device"""
    import circom_compat_amd as cc
    sys.path.insert(0, ROOT)
    import bench
    mats, (A, Bm, Cm), w, n_vars = bench.chain_circuit(cc, 12)
    rng = random.Random(1212)
    pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, R) for _ in range(5)])
    pr = cc.Prover(pk, mats, lib=gpulib)
    r, s = 1234567, 7654321
    before = pr.prove(r, s, w)
    srs = cc.contribute_srs(cc.new_srs(12, lib=gpulib), lib=gpulib)
    assert pr.prove(r, s, w).raw == before.raw
    assert cc.check_srs(cc.contribute_srs(srs, _secrets(1213), lib=gpulib), lib=gpulib).ok
    assert pr.prove(r, s, w).raw == before.raw
    pr.close()
