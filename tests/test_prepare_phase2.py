"""Prepared powers of tau: cc.prepare_phase2 (g16_srs_prepare), cc.check_lagrange (g16_srs_lagrange_check) and
cc.setup_from_srs / cc.check_key_circuit with lagrange= (g16_setup_from_prepared).

Expected points never come from the library: every level is o.G1.mul / o.G2.mul of o.lagrange_at_tau(2^p, tau) (the
padded top level of tau_g1: the inverse transform of the powers with the last set to 0), scaled by alpha / beta.
Verdicts of check_lagrange follow from the arithmetic: a Lagrange point replaced by another element of its prime-order
group differs from the right one by d G, d != 0, and breaks exactly its own array's relation (probability 1 - 2^-127
over rho); structural reasons are the kind of fault that was planted.

Time limits of the GPU cases: prepare_phase2 at 2^16 is about 2^16 * 16 butterflies of a 255-step ladder per array,
twice over for the levels below (~10^11 field multiplications, a few seconds of kernel time at most); the check is a
tenth of that.  The limits below are hang guards, not performance gates."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_setup_srs import _csrs, _mixed_circuit, _same_key, _wide_circuit
from test_srs_check import _plus_q, _y_plus_1
from test_verify import _twist_point_outside_g2

R = o.R_MOD
NONCANON, OFF_CURVE, SUBGROUP = 1, 2, 4
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
BIT = {name: 1 << i for i, name in enumerate(ARRAYS)}
QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")
D1 = 0x1D0C0FFEE0DDBA11F00D5EED0FACADE5C0DEC0DE1234567890ABCDEF13579BDF % R
GUARD_S = 120.0


def _tox3(seed):
    rng = random.Random(seed)
    return [rng.randrange(2, R) for _ in range(3)]


def _tops(power):
    return dict(tau_g1=power + 1, tau_g2=power, alpha_tau_g1=power, beta_tau_g1=power)


def _n_rho(power):
    return ((4 << power) - 1) + 3 * ((2 << power) - 1)


def _rho(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


def _rho_at(power, name, p, j):
    """index into rho of entry j of level p of the array"""
    at = 0
    for a in ARRAYS:
        if a == name:
            return at + (1 << p) - 1 + j
        at += (2 << _tops(power)[a]) - 1
    raise KeyError(name)


# ---- expected levels from the oracle, computed once ------------------------------------------------------
_scalar_cache, _level_cache, _set_cache = {}, {}, {}


def _level_scalars(power, tau, p):
    """L_j(tau) of the domain of size 2^p; p = power + 1: the transform of the powers with the last set to 0"""
    key = (power, tau, p)
    if key not in _scalar_cache:
        n = 1 << p
        if p <= power:
            _scalar_cache[key] = o.lagrange_at_tau(n, tau)
        else:
            pw = [pow(tau, i, R) for i in range(n)]
            pw[-1] = 0
            _scalar_cache[key] = o.ntt(pw, inverse=True)
    return _scalar_cache[key]


def _oracle_level(power, tox, name, p):
    key = (power, tuple(tox), name, p)
    if key not in _level_cache:
        tau, alpha, beta = tox
        scale = dict(tau_g1=1, tau_g2=1, alpha_tau_g1=alpha, beta_tau_g1=beta)[name]
        sc = [s * scale % R for s in _level_scalars(power, tau, p)]
        if name == "tau_g2":
            raw = b"".join(o.g2_to_bytes(o.G2.mul(o.G2_GEN, s)) for s in sc)
        else:
            raw = b"".join(o.g1_to_bytes(o.G1.mul(o.G1_GEN, s)) for s in sc)
        _level_cache[key] = np.frombuffer(raw, dtype=np.uint8).reshape(1 << p, -1)
    return _level_cache[key]


def _prepared(cc, lib, power, tox, log2=None):
    """(srs, LagrangeSrs) of the trapdoor string, once per library; treat as read-only (see _copy)"""
    key = (id(lib), power, tuple(tox), log2)
    if key not in _set_cache:
        srs = cc.trapdoor_srs(log2 if log2 is not None else power, tox, lib=lib)
        _set_cache[key] = (srs, cc.prepare_phase2(srs, power=power, lib=lib))
    return _set_cache[key]


def _copy(cc, lag):
    return cc.LagrangeSrs(lag.power, *(np.array(getattr(lag, a), dtype=np.uint8, copy=True) for a in ARRAYS))


def _same_set(a, b):
    assert a.power == b.power
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape, name
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8])


def _assert_levels(lag, power, tox, skip=()):
    for name in ARRAYS:
        assert lag.levels(name) == _tops(power)[name] + 1
        for p in range(lag.levels(name)):
            if (name, p) in skip:
                continue
            got, want = lag.level(name, p), _oracle_level(power, tox, name, p)
            assert got.shape == want.shape, (name, p)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (name, p, bad[:8])


# ---- 1. levels against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("power,seed", [(3, 61), (5, 62)])
def test_levels_vs_oracle(lib, power, seed):
    import circom_compat_amd as cc
    tox = _tox3(seed)
    srs, lag = _prepared(cc, lib, power, tox)
    assert lag.power == power
    assert lag.tau_g1.shape == ((4 << power) - 1, 64) and lag.tau_g2.shape == ((2 << power) - 1, 128)
    assert lag.alpha_tau_g1.shape == lag.beta_tau_g1.shape == ((2 << power) - 1, 64)
    _assert_levels(lag, power, tox)
    for name in ARRAYS:                                           # level 0 is M[0]
        assert np.array_equal(lag.level(name, 0)[0], getattr(srs, name)[0]), name
    assert cc.LagrangeSrs.locate(0) == (0, 0) and cc.LagrangeSrs.locate((1 << power) - 1 + 3) == (power, 3)
    ms = cc.prepare_phase2_times(lib)
    assert set(ms) == set(cc.SETUP_SRS_PHASES) and ms["ntt_g1"] > 0 and ms["ntt_g2"] > 0 and ms["combine"] == 0


# ---- 2. tau on the domain --------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 8])
def test_tau_on_the_domain(lib, order):
    """tau a root of unity of order 1 / 8: on every domain that contains it L_j(tau) is 1 at one j and 0 elsewhere --
    one proper point and all-zero records, through butterflies whose difference is infinity and affine runs whose
    shared inversion skips the infinities"""
    import circom_compat_amd as cc
    power = 4
    tau = 1 if order == 1 else o.root_of_unity(8)
    assert pow(tau, order, R) == 1 and (order == 1 or pow(tau, 4, R) != 1)
    tox = [tau, 0xA11CE, 0xB0B]
    srs, lag = _prepared(cc, lib, power, tox)
    first = 0 if order == 1 else 3                                # the smallest level whose domain holds tau
    for name in ARRAYS:
        for p in range(first, power + 1):                          # the padded level P+1 is not such a transform
            lvl = lag.level(name, p)
            nz = np.nonzero(lvl.any(axis=1))[0]
            assert nz.size == 1, (name, p, nz)
            j = int(nz[0])
            assert pow(o.root_of_unity(1 << p), j, R) == tau, (name, p, j)
            assert np.array_equal(lvl[j], getattr(srs, name)[0]), (name, p)      # 1 * M[0]
    _assert_levels(lag, power, tox)                               # every level, the other ones included
    rep = cc.check_lagrange(srs, lag, lib=lib)
    assert rep.ok, rep
    assert rep.n_infinity["tau_g2"] == sum((1 << p) - 1 for p in range(first, power + 1))


# ---- 3. longer strings are cut ---------------------------------------------------------------------------
def test_longer_strings_are_cut(lib):
    import circom_compat_amd as cc
    tox = _tox3(63)
    _srs4, want = _prepared(cc, lib, 4, tox)
    longer = cc.trapdoor_srs(6, tox, lib=lib)
    got = cc.prepare_phase2(longer, power=4, lib=lib)
    _same_set(got, want)
    assert cc.check_lagrange(longer, got, lib=lib).ok             # the check cuts the string the same way
    assert cc.prepare_phase2(longer, lib=lib).power == 6          # default: all the string covers


# ---- 4. check_lagrange -----------------------------------------------------------------------------------
@pytest.mark.parametrize("power,chunk", [(3, 1), (3, 5), (5, 16), (5, 1 << 20)])
def test_honest_sets_pass(lib, monkeypatch, power, chunk):
    """chunks of 1, 5 and 16 points: levels start at 2^p - 1, so every level above the chunk straddles seams"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", str(chunk))
    srs, lag = _prepared(cc, lib, power, _tox3(61 if power == 3 else 62))
    rep = cc.check_lagrange(srs, lag, lib=lib)
    assert rep.ok and rep.relations_checked and rep.relations_failed == 0 and rep.failed_arrays == []
    assert rep.n_points == dict(tau_g1=(4 << power) - 1, tau_g2=(2 << power) - 1, alpha_tau_g1=(2 << power) - 1,
                                beta_tau_g1=(2 << power) - 1)
    assert not any(rep.n_bad.values()) and not any(rep.n_infinity.values()) and rep.bad_points == []
    assert rep.describe() == "ok"
    rho = _rho(5, _n_rho(power))
    assert cc.check_lagrange(srs, lag, rho=rho, lib=lib).ok


def _other_point(name, salt):
    if name == "tau_g2":
        return np.frombuffer(o.g2_to_bytes(o.G2.mul(o.G2_GEN, 0xC0FFEE + salt)), dtype=np.uint8)
    return np.frombuffer(o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE + salt)), dtype=np.uint8)


def _wrong_cases():
    P = 3
    cases = []
    for name in ARRAYS:
        top = _tops(P)[name]
        # level 0; the first and the last entry of a level; the last point of the section
        cases += [(name, 0, 0), (name, 2, 0), (name, 2, 3), (name, top, (1 << top) - 1)]
    cases += [("tau_g1", P + 1, 0), ("tau_g1", P + 1, 5)]      # more of the padded level; its last is the section's last
    return cases


@pytest.mark.parametrize("name,p,j", _wrong_cases())
def test_one_wrong_point_fails_its_array(lib, monkeypatch, name, p, j):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "5")
    srs, lag = _prepared(cc, lib, 3, _tox3(61))
    bad = _copy(cc, lag)
    bad.level(name, p)[j] = _other_point(name, p * 100 + j)
    rep = cc.check_lagrange(srs, bad, lib=lib)
    assert not rep.ok and rep.relations_checked and rep.relations_failed == BIT[name], rep
    assert rep.failed_arrays == [name] and name in rep.describe()
    assert not any(rep.n_bad.values()) and rep.bad_points == []


def test_swapped_entries_and_another_string_fail(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "5")
    srs, lag = _prepared(cc, lib, 3, _tox3(61))
    bad = _copy(cc, lag)
    lvl = bad.level("alpha_tau_g1", 3)
    lvl[[2, 6]] = lvl[[6, 2]]
    assert not np.array_equal(bad.alpha_tau_g1, lag.alpha_tau_g1)
    assert cc.check_lagrange(srs, bad, lib=lib).relations_failed == BIT["alpha_tau_g1"]
    # a correct set, of another string: every array fails
    other_srs, other = _prepared(cc, lib, 3, _tox3(64))
    assert cc.check_lagrange(other_srs, other, lib=lib).ok
    rep = cc.check_lagrange(srs, other, lib=lib)
    assert not rep.ok and rep.relations_failed == 15 and rep.failed_arrays == list(ARRAYS)


def _plant(lag, name, p, j, kind, salt=0):
    """overwrite an entry with a structural fault; returns the list entry the report must have"""
    raw = bytes(lag.level(name, p)[j])
    assert any(raw)
    if kind == "noncanon":
        new, why = _plus_q(raw, (j + salt) % (len(raw) // 32)), NONCANON
    elif kind == "offcurve":
        new, why = _y_plus_1(raw), OFF_CURVE
    else:
        assert kind == "cofactor" and name == "tau_g2"
        new, why = o.g2_to_bytes(_twist_point_outside_g2(1 + salt)), SUBGROUP
    lag.level(name, p)[j] = np.frombuffer(new, dtype=np.uint8)
    return (name, p, j, why)


STRUCT_CASES = [("tau_g1", 0, 0, "noncanon"), ("tau_g1", 6, 63, "offcurve"), ("tau_g1", 4, 0, "noncanon"),
                ("tau_g2", 4, 1, "noncanon"), ("tau_g2", 4, 0, "offcurve"), ("tau_g2", 5, 31, "cofactor"),
                ("tau_g2", 0, 0, "cofactor"), ("alpha_tau_g1", 0, 0, "offcurve"), ("alpha_tau_g1", 5, 31, "noncanon"),
                ("beta_tau_g1", 4, 2, "offcurve"), ("beta_tau_g1", 3, 7, "noncanon")]


@pytest.mark.parametrize("name,p,j,kind", STRUCT_CASES)
def test_structural_faults_are_located(lib, monkeypatch, name, p, j, kind):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "16")                # level 4 starts at 15, level 5 at 31
    srs, lag = _prepared(cc, lib, 5, _tox3(62))
    bad = _copy(cc, lag)
    planted = _plant(bad, name, p, j, kind)
    rep = cc.check_lagrange(srs, bad, lib=lib)
    assert rep.bad_points == [planted], (rep.bad_points, planted)
    assert not rep.ok and not rep.relations_checked and rep.relations_failed == 0
    assert sum(rep.n_bad.values()) == 1 and rep.n_bad[name] == 1
    assert f"{name} level {p} entry {j}" in rep.describe()


def test_faults_in_several_arrays_come_sorted(lib, monkeypatch):
    """counts per array and one list in ascending (array, position) order, whatever the chunking; the list is cut at
    max_listed, the counts are not"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "16")
    srs, lag = _prepared(cc, lib, 5, _tox3(62))
    bad = _copy(cc, lag)
    planted = [_plant(bad, "beta_tau_g1", 5, 9, "offcurve"), _plant(bad, "tau_g2", 5, 30, "cofactor"),
               _plant(bad, "tau_g1", 6, 1, "noncanon"), _plant(bad, "tau_g2", 2, 1, "offcurve"),
               _plant(bad, "tau_g1", 4, 1, "offcurve"), _plant(bad, "alpha_tau_g1", 4, 0, "noncanon"),
               _plant(bad, "tau_g1", 4, 0, "noncanon")]
    want = sorted(planted, key=lambda e: (ARRAYS.index(e[0]), e[1], e[2]))
    rep = cc.check_lagrange(srs, bad, lib=lib)
    assert rep.bad_points == want
    assert rep.n_bad == dict(tau_g1=3, tau_g2=2, alpha_tau_g1=1, beta_tau_g1=1) and not rep.relations_checked
    cut = cc.check_lagrange(srs, bad, max_listed=4, lib=lib)
    assert cut.bad_points == want[:4] and cut.n_bad == rep.n_bad
    assert cc.check_lagrange(srs, bad, max_listed=0, lib=lib).bad_points == []


def test_coefficients_are_used(lib, monkeypatch):
    """whoever knows rho cancels two entries: Lambda[a] += rho_b D and Lambda[b] -= rho_a D change the combination by
    rho_a rho_b D - rho_b rho_a D = 0.  The check passes with that rho and fails with any other."""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "5")
    power = 3
    srs, lag = _prepared(cc, lib, power, _tox3(61))
    rho = _rho(77, _n_rho(power))
    (pa, ja), (pb, jb) = (2, 1), (4, 11)                          # two levels of tau_g1, the padded one among them
    ra, rb = rho[_rho_at(power, "tau_g1", pa, ja)], rho[_rho_at(power, "tau_g1", pb, jb)]
    D = o.G1.mul(o.G1_GEN, 0xD1FF)
    bad = _copy(cc, lag)
    A = o.g1_from_bytes(bytes(bad.level("tau_g1", pa)[ja]))
    Bp = o.g1_from_bytes(bytes(bad.level("tau_g1", pb)[jb]))
    bad.level("tau_g1", pa)[ja] = np.frombuffer(o.g1_to_bytes(o.G1.add(A, o.G1.mul(D, rb))), dtype=np.uint8)
    bad.level("tau_g1", pb)[jb] = np.frombuffer(o.g1_to_bytes(o.G1.add(Bp, o.G1.mul(D, R - ra))), dtype=np.uint8)
    rep = cc.check_lagrange(srs, bad, rho=rho, lib=lib)
    assert rep.ok and rep.relations_failed == 0
    rep = cc.check_lagrange(srs, bad, rho=_rho(78, _n_rho(power)), lib=lib)
    assert not rep.ok and rep.relations_failed == BIT["tau_g1"]
    assert cc.check_lagrange(srs, bad, lib=lib).relations_failed == BIT["tau_g1"]        # drawn coefficients


# ---- 5. setup --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
@pytest.mark.parametrize("which", ["domain8", "wide"])
def test_setup_at_the_power_is_setup_from_srs(lib, which, reduction):
    import circom_compat_amd as cc
    if which == "domain8":
        cons, _w, n_vars, n_pub = H.squaring_chain(3)
        power, seed = 3, 61
    else:
        cons, n_vars, n_pub = _wide_circuit()
        power, seed = 5, 62
    srs, lag = _prepared(cc, lib, power, _tox3(seed))
    csrs = _csrs(cc, cons, lib)
    want = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib, reduction=reduction)
    got = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib, reduction=reduction, lagrange=lag)
    assert got.domain_size == 1 << power
    _same_key(got, want)


_below = {}


def _below_keys(cc, lib):
    """the domain-8 squaring chain under a power-5 string: plain and prepared-path keys, both reductions"""
    if id(lib) not in _below:
        cons, w, n_vars, n_pub = H.squaring_chain(3)
        tox = _tox3(62)
        srs, lag = _prepared(cc, lib, 5, tox)
        csrs = _csrs(cc, cons, lib)
        keys = {(red, how): cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib, reduction=red,
                                              lagrange=lag if how == "prepared" else None)
                for red in ("circom", "libsnark") for how in ("plain", "prepared")}
        _below[id(lib)] = (cons, w, n_vars, n_pub, tox, srs, lag, csrs, keys)
    return _below[id(lib)]


def test_setup_below_the_power(lib):
    """every field but the circom h_query is setup_from_srs's; h_query is the odd half of level k+1 as it stands"""
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub, tox, srs, lag, csrs, keys = _below_keys(cc, lib)
    plain, prep = keys["circom", "plain"], keys["circom", "prepared"]
    assert prep.domain_size == 8
    _same_key(keys["libsnark", "prepared"], keys["libsnark", "plain"])
    assert not np.array_equal(prep.h_query, plain.h_query)
    h = np.array(plain.h_query, copy=True)
    same_but_h = cc.ProvingKey(prep.n_vars, prep.n_public, prep.domain_size, prep.vk, bytes(prep.beta_g1),
                               bytes(prep.delta_g1), prep.a_query, prep.b_g1_query, prep.b_g2_query, prep.l_query, h)
    _same_key(same_but_h, plain)
    want = b"".join(o.g1_to_bytes(o.G1.mul(o.G1_GEN, s)) for s in o.lagrange_at_tau(16, tox[0])[1::2])
    assert np.asarray(prep.h_query).tobytes() == want
    assert np.array_equal(np.asarray(prep.h_query), lag.level("tau_g1", 4)[1::2])


def test_proofs_below_the_power_are_the_same(lib):
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub, tox, srs, lag, csrs, keys = _below_keys(cc, lib)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    proofs = []
    for how in ("plain", "prepared"):
        key = keys["circom", how]
        pr = cc.Prover(key, H.matrices_from_rows(a_rows, b_rows, 2, n_vars, lib), lib=lib)
        proofs.append(pr.prove(1234567, 7654321, w))
        pr.close()
        assert cc.verify_batch(key.vk, [proofs[-1]], [w[1:2]], lib=lib) == [True]
    assert len(proofs[0].raw) == 256 and proofs[0].raw == proofs[1].raw


def test_check_key_circuit_needs_the_files_level(lib):
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub, tox, srs, lag, csrs, keys = _below_keys(cc, lib)
    prep = keys["circom", "prepared"]                              # the key `snarkjs zkey new` would write
    rep = cc.check_key_circuit(prep, *csrs, srs, lib=lib)          # today's behaviour: the reason for lagrange=
    assert not rep.ok and rep.failed == "contribution"
    rep = cc.check_key_circuit(prep, *csrs, srs, lib=lib, lagrange=lag)
    assert rep.ok and rep.failed is None
    key1 = cc.contribute_key(prep, D1, lib=lib)
    assert cc.check_key_circuit(key1, *csrs, srs, lib=lib, lagrange=lag).ok
    assert cc.check_key_circuit(key1, *csrs, srs, lib=lib).failed == "contribution"
    assert cc.check_key_circuit(keys["libsnark", "prepared"], *csrs, srs, lib=lib, reduction="libsnark").ok


# ---- 6. arguments and repeatability ----------------------------------------------------------------------
def test_arguments(lib):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    srs, lag = _prepared(cc, lib, 3, _tox3(61))
    d, dl = srs.to_c(), lag.to_c()
    outs = [np.zeros((m, w), dtype=np.uint8) for m, w in ((31, 64), (15, 128), (15, 64), (15, 64))]
    ptrs = [x.ctypes.data_as(C.c_void_p) for x in outs]
    prep = lambda dev, desc, power, *p: lib.g16_srs_prepare(dev, desc, power, *p)
    assert prep(0, None, 3, *ptrs) == B.G16_ERR_INVALID
    for i in range(4):
        assert prep(0, C.byref(d), 3, *[None if k == i else p for k, p in enumerate(ptrs)]) == B.G16_ERR_INVALID
    assert prep(0, C.byref(d), 28, *ptrs) == B.G16_ERR_DOMAIN_TOO_LARGE
    assert prep(0, C.byref(d), 4, *ptrs) == B.G16_ERR_INVALID          # the string covers power 3 only
    short_srs = cc.Srs(srs.tau_g1[:-1], srs.tau_g2, srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2)
    short = short_srs.to_c()
    assert prep(0, C.byref(short), 3, *ptrs) == B.G16_ERR_INVALID
    short2_srs = cc.Srs(srs.tau_g1, srs.tau_g2, srs.alpha_tau_g1[:-1], srs.beta_tau_g1, srs.beta_g2)
    short2 = short2_srs.to_c()
    assert prep(0, C.byref(short2), 3, *ptrs) == B.G16_ERR_INVALID
    nul = srs.to_c()
    nul.tau_g2 = None
    assert prep(0, C.byref(nul), 3, *ptrs) == B.G16_ERR_INVALID
    assert prep(99, C.byref(d), 3, *ptrs) == B.G16_ERR_INVALID
    assert prep(-1, C.byref(d), 3, *ptrs) == B.G16_ERR_INVALID
    assert not any(x.any() for x in outs)                               # nothing was written
    assert lib.g16_srs_prepare_times(None, 7) == B.G16_ERR_INVALID
    with pytest.raises(cc.SynthesisError):
        cc.prepare_phase2(srs, power=28, lib=lib)
    with pytest.raises(cc.G16Error):
        cc.prepare_phase2(srs, power=4, lib=lib)
    with pytest.raises(cc.G16Error):
        cc.LagrangeSrs(3, lag.tau_g1[:-1], lag.tau_g2, lag.alpha_tau_g1, lag.beta_tau_g1)
    with pytest.raises(cc.G16Error):
        lag.level("tau_g2", 4)

    # the check
    rep = B.SrsLagrangeReportC()
    bad = (B.KeyBadPoint * 4)()
    chk = lambda dev, a, b, rho, lst, cap, r: lib.g16_srs_lagrange_check(dev, a, b, rho, lst, cap, r)
    assert chk(0, None, C.byref(dl), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert chk(0, C.byref(d), None, None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert chk(0, C.byref(d), C.byref(dl), None, bad, 4, None) == B.G16_ERR_INVALID
    assert chk(0, C.byref(d), C.byref(dl), None, None, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert chk(0, C.byref(short), C.byref(dl), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert chk(0, C.byref(nul), C.byref(dl), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    nul_l = lag.to_c()
    nul_l.beta_tau_g1 = None
    assert chk(0, C.byref(d), C.byref(nul_l), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    big = lag.to_c()
    big.power = 28
    assert chk(0, C.byref(d), C.byref(big), None, bad, 4, C.byref(rep)) == B.G16_ERR_DOMAIN_TOO_LARGE
    assert chk(99, C.byref(d), C.byref(dl), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    rho = _rho(9, _n_rho(3))
    for at in (0, 30, 31, len(rho) - 1):
        zero = list(rho)
        zero[at] = 0
        with pytest.raises(cc.G16Error) as e:
            cc.check_lagrange(srs, lag, rho=zero, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    with pytest.raises(cc.G16Error):
        cc.check_lagrange(srs, lag, rho=rho[:-1], lib=lib)

    # the setup: a Lagrange set below the circuit's domain, NULLs, the device
    cons, n_vars, n_pub = _wide_circuit()                               # domain 32
    with pytest.raises(cc.G16Error) as e:
        cc.setup_from_srs(*_csrs(cc, cons, lib), n_vars, n_pub, cc.trapdoor_srs(5, _tox3(61), lib=lib), lib=lib,
                          lagrange=lag)
    assert e.value.status == B.G16_ERR_INVALID
    cons, _w, n_vars, n_pub = H.squaring_chain(3)
    csrs = _csrs(cc, cons, lib)
    cat, cbt, cct = (m.to_c() for m in cc._setup_matrices(*csrs, n_vars, n_pub, lib))
    h = C.c_void_p()
    call = lambda dev, s, l, red: lib.g16_setup_from_prepared(dev, C.byref(cat), C.byref(cbt), C.byref(cct), n_vars,
                                                              n_pub, len(cons), s, l, red, C.byref(h))
    assert call(0, C.byref(d), None, 0) == B.G16_ERR_INVALID
    assert call(0, None, C.byref(dl), 0) == B.G16_ERR_INVALID
    assert call(0, C.byref(d), C.byref(nul_l), 0) == B.G16_ERR_INVALID
    assert call(0, C.byref(d), C.byref(dl), 7) == B.G16_ERR_INVALID
    assert call(99, C.byref(d), C.byref(dl), 0) == B.G16_ERR_INVALID
    assert call(0, C.byref(d), C.byref(big), 0) == B.G16_ERR_DOMAIN_TOO_LARGE


def test_repeatable(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "7")
    srs, lag = _prepared(cc, lib, 4, _tox3(63))
    _same_set(cc.prepare_phase2(srs, lib=lib), lag)
    bad = _copy(cc, lag)
    _plant(bad, "tau_g2", 3, 2, "offcurve")
    _plant(bad, "tau_g1", 5, 31, "noncanon")
    a, b = cc.check_lagrange(srs, bad, lib=lib), cc.check_lagrange(srs, bad, lib=lib)
    assert a == b and len(a.bad_points) == 2
    wrong = _copy(cc, lag)
    wrong.level("beta_tau_g1", 4)[15] = _other_point("beta_tau_g1", 1)
    rho = _rho(3, _n_rho(4))
    a, b = cc.check_lagrange(srs, wrong, rho=rho, lib=lib), cc.check_lagrange(srs, wrong, rho=rho, lib=lib)
    assert a == b and a.relations_failed == BIT["beta_tau_g1"]


# ---- 7. at size, on the GPU ------------------------------------------------------------------------------
def _gpu_round(cc, lib, power, cons, n_vars, n_pub, seams):
    tox = _tox3(70 + power)
    srs = cc.trapdoor_srs(power, tox, lib=lib)
    t0 = time.perf_counter()
    lag = cc.prepare_phase2(srs, lib=lib)
    t1 = time.perf_counter()
    rep = cc.check_lagrange(srs, lag, lib=lib)
    t2 = time.perf_counter()
    print(f"prepare_phase2 2^{power}: {t1 - t0:.3f} s {cc.prepare_phase2_times(lib)}; check_lagrange {t2 - t1:.3f} s")
    assert rep.ok, rep
    assert lag.level("tau_g1", 0).tobytes() == srs.tau_g1[0].tobytes()
    for name, index in seams:
        bad = _copy(cc, lag)
        p, j = cc.LagrangeSrs.locate(index)
        bad.level(name, p)[j] = _other_point(name, index)
        rep = cc.check_lagrange(srs, bad, lib=lib)
        assert not rep.ok and rep.relations_failed == BIT[name], (name, index, rep)
    csrs = _csrs(cc, cons, lib)
    want = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib)
    got = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib, lagrange=lag)
    assert got.domain_size == 1 << power
    _same_key(got, want)
    return time.perf_counter() - t0


@pytest.mark.gpu
def test_power_12_gpu(gpulib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_LAGCHECK_CHUNK", "1000")               # seams at multiples of 1000 in every section
    cons, n_vars, n_pub = _mixed_circuit(12)
    seams = [("tau_g1", 999), ("tau_g1", 1000), ("tau_g1", (4 << 12) - 2), ("tau_g2", 7999), ("alpha_tau_g1", 8000),
             ("beta_tau_g1", 0)]
    assert _gpu_round(cc, gpulib, 12, cons, n_vars, n_pub, seams) < GUARD_S
    # structural faults on either side of a seam, sorted
    srs = cc.trapdoor_srs(12, _tox3(82), lib=gpulib)
    bad = _copy(cc, cc.prepare_phase2(srs, lib=gpulib))
    planted = []
    for name, index, kind in (("tau_g1", 999, "offcurve"), ("tau_g1", 1000, "noncanon"), ("tau_g2", 3000, "cofactor"),
                              ("beta_tau_g1", 8190, "offcurve")):
        p, j = cc.LagrangeSrs.locate(index)
        planted.append(_plant(bad, name, p, j, kind))
    rep = cc.check_lagrange(srs, bad, lib=gpulib)
    assert rep.bad_points == planted and not rep.relations_checked


@pytest.mark.gpu
def test_power_16_gpu(gpulib):
    import circom_compat_amd as cc
    cons, _w, n_vars, n_pub = H.squaring_chain(16)
    assert _gpu_round(cc, gpulib, 16, cons, n_vars, n_pub, []) < GUARD_S


@pytest.mark.gpu
def test_live_prover_is_untouched_gpu(gpulib):
    import circom_compat_amd as cc
    lib = gpulib
    cons, w, n_vars, n_pub = H.squaring_chain(6)
    csrs = _csrs(cc, cons, lib)
    srs = cc.trapdoor_srs(6, _tox3(55), lib=lib)
    key = cc.contribute_key(cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib), D1, lib=lib)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    pr = cc.Prover(key, H.matrices_from_rows(a_rows, b_rows, 2, n_vars, lib), lib=lib)
    before = pr.prove(1234567, 7654321, w).raw
    lag = cc.prepare_phase2(srs, lib=lib)
    assert cc.check_lagrange(srs, lag, lib=lib).ok
    after = pr.prove(1234567, 7654321, w).raw
    pr.close()
    assert before == after
