"""Validation of a powers-of-tau string on the GPU: cc.check_srs (g16_srs_check).

Expected verdicts never come from the library.  An honest string is built from (tau, alpha, beta) with the oracle's
scalar multiplications and must pass by construction.  The relation mask of a tampered 2^3 string is computed HERE
(_oracle_mask) from oracle/bn254_ref.py -- its scalar multiplication for Lo / Hi and its pairing for the six pairs --
with the same explicit rho the library is given.  At sizes where Python pairings over many cases take too long the
expected bit follows from the arithmetic: one entry of an array replaced by another element of its (prime-order) group
breaks exactly that array's ratio relation (probability 1 - 2^-127 over rho) and, unless it is entry 1 of tau_g1 /
tau_g2 or entry 0 of beta_tau_g1, nothing else.  Structural reasons are the kind of fault that was planted.

Time limits of the GPU cases at 2^16 (n = 65536): 4n - 1 G1 points at 128 doublings + ~128 additions (~3 10^3 field
multiplications each) and n G2 points at a 254-step subgroup test plus the same chain over Fq2 (~3 10^4 each): about
3 10^9 field multiplications per call, well under a second of kernel time, plus a 21 MB upload.  The 60 s per call
below is a hang guard two orders of magnitude above that, not a performance gate."""
import os
import random
import sys
import time

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_verify import _twist_point_outside_g2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R_MOD
NONCANON, OFF_CURVE, SUBGROUP = 1, 2, 4
BASE, DEGENERATE, PAIR_TAU, PAIR_TAU_G1, PAIR_TAU_G2, PAIR_ALPHA, PAIR_BETA, PAIR_BETA_G2 = 1, 2, 4, 8, 16, 32, 64, 128
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
ARRAY_BIT = dict(tau_g1=PAIR_TAU_G1, tau_g2=PAIR_TAU_G2, alpha_tau_g1=PAIR_ALPHA, beta_tau_g1=PAIR_BETA)
CHUNK = 16
GUARD_S = 60.0


# ---- strings as lists of oracle points ---------------------------------------------------------------------
def _tox3(seed):
    rng = random.Random(seed)
    return [rng.randrange(2, R) for _ in range(3)]


def _points(k, tox, extra=0):
    """the string of (tau, alpha, beta) for domain 2^k (+ extra entries per array) as oracle points"""
    tau, alpha, beta = tox
    n = (1 << k) + extra
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    return dict(tau_g1=[o.G1.mul(o.G1_GEN, p) for p in pw], tau_g2=[o.G2.mul(o.G2_GEN, p) for p in pw[:n]],
                alpha_tau_g1=[o.G1.mul(o.G1_GEN, alpha * p % R) for p in pw[:n]],
                beta_tau_g1=[o.G1.mul(o.G1_GEN, beta * p % R) for p in pw[:n]], beta_g2=o.G2.mul(o.G2_GEN, beta))


_pts_cache = {}


def _honest(k, seed, extra=0):
    key = (k, seed, extra)
    if key not in _pts_cache:
        _pts_cache[key] = _points(k, _tox3(seed), extra)
    S = _pts_cache[key]
    return {name: (list(v) if isinstance(v, list) else v) for name, v in S.items()}


def _srs(cc, S):
    arr = lambda pts, enc, w: np.frombuffer(b"".join(enc(p) for p in pts), dtype=np.uint8).reshape(-1, w).copy()
    return cc.Srs(arr(S["tau_g1"], o.g1_to_bytes, 64), arr(S["tau_g2"], o.g2_to_bytes, 128),
                  arr(S["alpha_tau_g1"], o.g1_to_bytes, 64), arr(S["beta_tau_g1"], o.g1_to_bytes, 64),
                  o.g2_to_bytes(S["beta_g2"]))


def _copy_srs(cc, srs):
    return cc.Srs(*(np.array(getattr(srs, a), dtype=np.uint8, copy=True) for a in ARRAYS), srs.beta_g2)


def _n_rho(S):
    return (len(S["tau_g1"]) - 1) + 3 * (len(S["tau_g2"]) - 1)


def _rho(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


def _segments(S, rho):
    out, at = {}, 0
    for name in ARRAYS:
        out[name] = rho[at:at + len(S[name]) - 1]
        at += len(S[name]) - 1
    assert at == len(rho)
    return out


# ---- the oracle's verdict -----------------------------------------------------------------------------------
_pair_cache = {}


def _pairs_equal(P1, Q1, P2, Q2):
    """e(P1, Q1) == e(P2, Q2) on the CPU (P in G1, Q in G2, None = infinity)"""
    key = (P1, Q1, P2, Q2)
    if key not in _pair_cache:
        f = o._f12_mul(o.miller_loop(Q1, P1), o.miller_loop(Q2, None if P2 is None else o.G1.neg(P2)))
        _pair_cache[key] = o.final_exponentiation(f) == o.miller_loop(None, None)
    return _pair_cache[key]


def _lo_hi(curve, P, rho):
    assert len(rho) == len(P) - 1
    terms = lambda pts: curve.sum([curve.mul(p, k) for p, k in zip(pts, rho) if p is not None])
    return terms(P[:-1]), terms(P[1:])


def _oracle_mask(S, rho):
    seg = _segments(S, rho)
    g1, g2 = o.G1_GEN, o.G2_GEN
    t1, t2 = S["tau_g1"][1], S["tau_g2"][1]
    mask = 0
    if S["tau_g1"][0] != g1 or S["tau_g2"][0] != g2:
        mask |= BASE
    if None in (t1, t2, S["alpha_tau_g1"][0], S["beta_tau_g1"][0], S["beta_g2"]):
        mask |= DEGENERATE
    if not _pairs_equal(t1, g2, g1, t2):
        mask |= PAIR_TAU
    for name in ("tau_g1", "alpha_tau_g1", "beta_tau_g1"):
        lo, hi = _lo_hi(o.G1, S[name], seg[name])
        if not _pairs_equal(hi, g2, lo, t2):
            mask |= ARRAY_BIT[name]
    lo, hi = _lo_hi(o.G2, S["tau_g2"], seg["tau_g2"])
    if not _pairs_equal(t1, lo, g1, hi):
        mask |= PAIR_TAU_G2
    if not _pairs_equal(S["beta_tau_g1"][0], g2, g1, S["beta_g2"]):
        mask |= PAIR_BETA_G2
    return mask


def _clean(rep, S=None):
    assert rep.ok and rep.relations_checked and rep.relations_failed == 0 and rep.bad_points == [], rep
    assert all(v == 0 for v in rep.n_bad.values()) and all(v == 0 for v in rep.n_infinity.values()), rep
    assert rep.describe() == "ok"
    if S is not None:
        assert rep.n_points == dict(tau_g1=len(S["tau_g1"]), tau_g2=len(S["tau_g2"]),
                                    alpha_tau_g1=len(S["alpha_tau_g1"]), beta_tau_g1=len(S["beta_tau_g1"]), singles=1)


# ---- 1. honest strings pass -------------------------------------------------------------------------------
@pytest.mark.parametrize("k,seed", [(3, 41), (5, 42)])
def test_honest_strings_pass(lib, monkeypatch, k, seed):
    """oracle-built strings, with the default chunk (one chunk per array) and in chunks of 16 (2^5: every array
    crosses seams), with drawn and with explicit coefficients"""
    import circom_compat_amd as cc
    S = _honest(k, seed)
    srs = _srs(cc, S)
    _clean(cc.check_srs(srs, lib=lib), S)
    _clean(cc.check_srs(srs, rho=_rho(seed, _n_rho(S)), lib=lib), S)
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(CHUNK))
    _clean(cc.check_srs(srs, lib=lib), S)
    _clean(cc.check_srs(srs, rho=_rho(seed + 1, _n_rho(S)), lib=lib), S)
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", "5")                      # seams inside every array at 2^3 too
    _clean(cc.check_srs(srs, rho=_rho(seed + 2, _n_rho(S)), lib=lib), S)
    _clean(cc.check_srs(srs, lib=lib), S)


def test_trapdoor_srs_and_longer_strings_pass(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(CHUNK))
    srs = cc.trapdoor_srs(6, _tox3(43), lib=lib)
    rep = cc.check_srs(srs, lib=lib)
    assert rep.ok and rep.n_points == dict(tau_g1=127, tau_g2=64, alpha_tau_g1=64, beta_tau_g1=64, singles=1), rep
    # longer than any power of two needs: 2^3 + 3 entries per array, 21 of tau_g1 -- every one is checked
    S = _honest(3, 44, extra=3)
    _clean(cc.check_srs(_srs(cc, S), lib=lib), S)
    assert len(S["tau_g1"]) == 21 and len(S["tau_g2"]) == 11
    S["tau_g1"][20] = o.G1.mul(o.G1_GEN, 5)                                # beyond what a domain of 8 reads
    rep = cc.check_srs(_srs(cc, S), lib=lib)
    assert not rep.ok and rep.relations_failed == PAIR_TAU_G1


# ---- 2. relation masks, bit for bit ---------------------------------------------------------------------
OTHER1 = o.G1.mul(o.G1_GEN, 0xC0FFEE)
OTHER2 = o.G2.mul(o.G2_GEN, 0xBADC0DE)


def _tampered(case):
    """(points, the mask the case is stated to give or None) of a planted case on the 2^3 string of seed 45"""
    S = _honest(3, 45)
    tau, alpha, beta = _tox3(45)
    kind = case[0]
    if kind == "replace":
        _, name, i = case
        S[name][i] = OTHER2 if name == "tau_g2" else OTHER1
        return S, (ARRAY_BIT[name] if i > 1 else None)
    if kind == "swap":
        S["tau_g1"][4], S["tau_g1"][5] = S["tau_g1"][5], S["tau_g1"][4]
        return S, PAIR_TAU_G1
    if kind == "other_tau_g2":
        S["tau_g2"] = _points(3, [tau + 1, alpha, beta])["tau_g2"]
        return S, None
    if kind == "other_beta_g2":
        S["beta_g2"] = o.G2.mul(o.G2_GEN, beta + 1)
        return S, PAIR_BETA_G2
    if kind == "other_alpha":                                              # a valid string of (tau, alpha + 1, beta)
        S["alpha_tau_g1"] = _points(3, [tau, alpha + 1, beta])["alpha_tau_g1"]
        return S, 0
    if kind == "scaled":                                                   # tau_g1[i] = 2 tau^i G: every ratio holds
        S["tau_g1"] = [o.G1.mul(p, 2) for p in S["tau_g1"]]
        return S, None
    if kind == "tau_zero":
        for name in ARRAYS:
            S[name] = S[name][:1] + [None] * (len(S[name]) - 1)
        return S, DEGENERATE
    assert kind == "alpha_zero"
    S["alpha_tau_g1"] = [None] * len(S["alpha_tau_g1"])
    return S, DEGENERATE


MASK_CASES = [("replace", "tau_g1", i) for i in range(1, 15)] + \
    [("replace", "tau_g2", 5), ("replace", "tau_g2", 1), ("replace", "alpha_tau_g1", 3), ("replace", "alpha_tau_g1", 0),
     ("replace", "beta_tau_g1", 6), ("replace", "beta_tau_g1", 0), ("swap",), ("other_tau_g2",), ("other_beta_g2",),
     ("other_alpha",), ("scaled",), ("tau_zero",), ("alpha_zero",)]


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_relation_masks_equal_the_oracle(lib, case):
    """fixed rho at 2^3: relations_failed is the oracle's mask, bit for bit.  ("scaled": tau_g1 = 2 x the honest array
    keeps every neighbour ratio, so PAIR_TAU_G1 holds, but BASE is not the only bit: PAIR_TAU and PAIR_TAU_G2 pair
    tau_g1[1] = 2 tau G against the unscaled tau_g2 and fail too -- the oracle says so.)"""
    import circom_compat_amd as cc
    S, stated = _tampered(case)
    rho = _rho(4545, _n_rho(S))
    want = _oracle_mask(S, rho)
    if stated is not None:
        assert want == stated, (case, want, stated)
    if case == ("scaled",):
        assert want & BASE and not want & PAIR_TAU_G1
    rep = cc.check_srs(_srs(cc, S), rho=rho, lib=lib)
    assert rep.relations_checked and rep.bad_points == [] and all(v == 0 for v in rep.n_bad.values())
    assert rep.relations_failed == want, (case, rep.relations_failed, want)
    assert rep.ok == (want == 0)
    if case == ("tau_zero",):
        assert rep.n_infinity == dict(tau_g1=14, tau_g2=7, alpha_tau_g1=7, beta_tau_g1=7, singles=0)
    if want:
        assert rep.describe() != "ok" and "bad point" not in rep.describe()


# ---- 3. seams ---------------------------------------------------------------------------------------------
SEAM_CASES = [("tau_g1", 15), ("tau_g1", 16), ("tau_g1", 17), ("tau_g1", 31), ("tau_g1", 32), ("tau_g1", 62),
              ("tau_g2", 15), ("tau_g2", 16), ("tau_g2", 17), ("tau_g2", 31), ("alpha_tau_g1", 15),
              ("alpha_tau_g1", 16), ("alpha_tau_g1", 31), ("beta_tau_g1", 16), ("beta_tau_g1", 17), ("beta_tau_g1", 31)]


@pytest.mark.parametrize("name,i", SEAM_CASES)
def test_seams(lib, monkeypatch, name, i):
    """2^5 in chunks of 16: a replaced point on either side of a chunk seam and at the last index of every array is
    detected, with drawn coefficients, and breaks that array's relation alone"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(CHUNK))
    srs = _copy_srs(cc, _srs(cc, _honest(5, 42)))
    enc = o.g2_to_bytes(OTHER2) if name == "tau_g2" else o.g1_to_bytes(OTHER1)
    getattr(srs, name)[i] = np.frombuffer(enc, dtype=np.uint8)
    rep = cc.check_srs(srs, lib=lib)
    assert not rep.ok and rep.relations_checked and rep.relations_failed == ARRAY_BIT[name], (name, i, rep)
    monkeypatch.delenv("G16_SRSCHECK_CHUNK")
    assert cc.check_srs(srs, lib=lib).relations_failed == ARRAY_BIT[name]          # one chunk per array


# ---- 4. the coefficients are used -------------------------------------------------------------------------
def test_coefficients_are_used(lib, monkeypatch):
    """whoever knows rho cancels two entries: with rho_{j-1} = rho_j and rho_{k-1} = rho_k, tau_g1[j] += rho_k D and
    tau_g1[k] -= rho_j D leave both Lo (rho_j rho_k D - rho_k rho_j D) and Hi (the same with the equal neighbours)
    unchanged.  The check passes with that rho and fails with any other."""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", "5")
    S = _honest(3, 45)
    j, k = 3, 9
    rho = _rho(77, _n_rho(S))
    rho[j - 1], rho[k - 1] = rho[j], rho[k]                                  # the tau_g1 segment comes first
    D = o.G1.mul(o.G1_GEN, 0xD1FF)
    S["tau_g1"][j] = o.G1.add(S["tau_g1"][j], o.G1.mul(D, rho[k]))
    S["tau_g1"][k] = o.G1.add(S["tau_g1"][k], o.G1.mul(D, R - rho[j]))
    srs = _srs(cc, S)
    assert _oracle_mask(S, rho) == 0
    rep = cc.check_srs(srs, rho=rho, lib=lib)
    assert rep.ok and rep.relations_failed == 0
    other = _rho(78, _n_rho(S))
    assert _oracle_mask(S, other) == PAIR_TAU_G1
    rep = cc.check_srs(srs, rho=other, lib=lib)
    assert not rep.ok and rep.relations_failed == PAIR_TAU_G1
    assert cc.check_srs(srs, lib=lib).relations_failed == PAIR_TAU_G1        # drawn coefficients


# ---- 5. structural faults -----------------------------------------------------------------------------------
def _plus_q(raw, word):
    off = 32 * word
    v = int.from_bytes(raw[off:off + 32], "little") + o.Q_MOD
    assert v < 1 << 256
    return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]


def _y_plus_1(raw):
    off = len(raw) // 2
    v = int.from_bytes(raw[off:off + 32], "little") + 1
    assert v < o.Q_MOD
    return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]


def _plant(srs, name, i, kind, salt=0):
    """overwrite an entry with a structural fault; returns (query name, index, reason) as the report lists it"""
    raw = srs.beta_g2 if name == "beta_g2" else bytes(getattr(srs, name)[i])
    assert any(raw)
    if kind == "noncanon":
        new, why = _plus_q(raw, (i + salt) % (len(raw) // 32)), NONCANON
    elif kind == "offcurve":
        new, why = _y_plus_1(raw), OFF_CURVE
    elif kind == "cofactor":
        new, why = o.g2_to_bytes(_twist_point_outside_g2(1 + salt)), SUBGROUP
    else:
        assert kind == "order10069"
        T = _twist_point_outside_g2(7)
        P = o.G2.mul(T, R * ((2 * o.Q_MOD - R) // 10069))
        assert P is not None and o.G2.mul(P, 10069) is None and o.G2.mul(P, R) is not None and o.G2.on_curve(P)
        new, why = o.g2_to_bytes(P), SUBGROUP
    if name == "beta_g2":
        srs.beta_g2 = new
        return ("singles", 0, why)
    getattr(srs, name)[i] = np.frombuffer(new, dtype=np.uint8)
    return (name, i, why)


STRUCT_CASES = [("tau_g1", 0, "noncanon"), ("tau_g1", 16, "offcurve"), ("tau_g1", 62, "noncanon"),
                ("tau_g2", 15, "noncanon"), ("tau_g2", 16, "offcurve"), ("tau_g2", 31, "cofactor"),
                ("tau_g2", 3, "order10069"), ("alpha_tau_g1", 0, "offcurve"), ("alpha_tau_g1", 31, "noncanon"),
                ("beta_tau_g1", 17, "offcurve"), ("beta_tau_g1", 30, "noncanon"), ("beta_g2", 0, "noncanon"),
                ("beta_g2", 0, "offcurve"), ("beta_g2", 0, "cofactor")]


@pytest.mark.parametrize("name,i,kind", STRUCT_CASES)
def test_structural_faults_are_located(lib, monkeypatch, name, i, kind):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(CHUNK))
    srs = _copy_srs(cc, _srs(cc, _honest(5, 42)))
    planted = _plant(srs, name, i, kind)
    rep = cc.check_srs(srs, lib=lib)
    assert rep.bad_points == [planted], (rep.bad_points, planted)
    assert not rep.ok and not rep.relations_checked and rep.relations_failed == 0
    assert sum(rep.n_bad.values()) == 1 and rep.n_bad[planted[0]] == 1
    assert ("beta_g2" if name == "beta_g2" else f"{name}[{i}]") in rep.describe()


def test_faults_in_several_arrays_come_sorted(lib, monkeypatch):
    """counts per array and one list in ascending (array, index) order, whatever the chunking; the list is cut at
    max_listed, the counts are not"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(CHUNK))
    srs = _copy_srs(cc, _srs(cc, _honest(5, 42)))
    plan = [("beta_tau_g1", 31, "offcurve"), ("tau_g2", 16, "cofactor"), ("tau_g1", 47, "noncanon"),
            ("beta_g2", 0, "order10069"), ("tau_g1", 15, "offcurve"), ("alpha_tau_g1", 1, "noncanon"),
            ("tau_g2", 2, "noncanon"), ("tau_g1", 16, "noncanon"), ("beta_tau_g1", 0, "noncanon")]
    planted = [_plant(srs, name, i, kind, salt=s) for s, (name, i, kind) in enumerate(plan)]
    order = {q: n for n, q in enumerate(ARRAYS + ("singles",))}
    planted.sort(key=lambda b: (order[b[0]], b[1]))
    rep = cc.check_srs(srs, lib=lib)
    assert rep.bad_points == planted and not rep.ok and not rep.relations_checked and rep.relations_failed == 0
    assert rep.n_bad == dict(tau_g1=3, tau_g2=2, alpha_tau_g1=1, beta_tau_g1=2, singles=1)
    short = cc.check_srs(srs, max_listed=4, lib=lib)
    assert short.bad_points == planted[:4] and short.n_bad == rep.n_bad
    monkeypatch.delenv("G16_SRSCHECK_CHUNK")
    assert cc.check_srs(srs, lib=lib) == rep


# ---- 6. arguments and repeatability ---------------------------------------------------------------------
def test_arguments(lib):
    import ctypes as C
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    S = _honest(3, 41)
    srs = _srs(cc, S)
    d = srs.to_c()
    rep, bad = B.SrsReportC(), (B.KeyBadPoint * 4)()
    assert lib.g16_srs_check(0, None, None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert lib.g16_srs_check(0, C.byref(d), None, bad, 4, None) == B.G16_ERR_INVALID
    assert lib.g16_srs_check(0, C.byref(d), None, None, 4, C.byref(rep)) == B.G16_ERR_INVALID
    for field in ARRAYS:
        e = srs.to_c()
        setattr(e, field, None)
        assert lib.g16_srs_check(0, C.byref(e), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID, field
    for field in ("n_tau", "n_tau_g1"):
        for short in (0, 1):
            e = srs.to_c()
            setattr(e, field, short)
            assert lib.g16_srs_check(0, C.byref(e), None, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID, (field, short)
    # a zero coefficient anywhere: the last entry of the last segment here
    rho = _rho(1, _n_rho(S))
    arr = np.array([[x & 0xFFFFFFFFFFFFFFFF, x >> 64] for x in rho], dtype=np.uint64)
    arr[-1] = 0
    assert lib.g16_srs_check(0, C.byref(d), arr.ctypes.data, bad, 4, C.byref(rep)) == B.G16_ERR_INVALID
    with pytest.raises(cc.G16Error):
        cc.check_srs(srs, rho=rho[:-1], lib=lib)
    # bad_cap = 0: nothing listed, everything counted
    assert lib.g16_srs_check(0, C.byref(d), None, None, 0, C.byref(rep)) == B.G16_OK and rep.ok == 1
    faulty = _copy_srs(cc, srs)
    _plant(faulty, "tau_g1", 9, "offcurve")
    r0 = cc.check_srs(faulty, max_listed=0, lib=lib)
    assert r0.bad_points == [] and r0.n_bad["tau_g1"] == 1 and not r0.ok and not r0.relations_checked
    # the smallest string there is: two entries per array
    two = cc.Srs(srs.tau_g1[:2], srs.tau_g2[:2], srs.alpha_tau_g1[:2], srs.beta_tau_g1[:2], srs.beta_g2)
    assert cc.check_srs(two, lib=lib).ok


def test_repeatable(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(CHUNK))
    srs = _copy_srs(cc, _srs(cc, _honest(5, 42)))
    planted = sorted([_plant(srs, "tau_g1", 40, "offcurve"), _plant(srs, "tau_g1", 3, "noncanon")], key=lambda b: b[1])
    rho = _rho(9, 62 + 3 * 31)
    a, b = cc.check_srs(srs, rho=rho, lib=lib), cc.check_srs(srs, rho=rho, lib=lib)
    assert a == b and a.bad_points == planted
    S, _ = _tampered(("swap",))
    t = _srs(cc, S)
    assert cc.check_srs(t, rho=_rho(4545, _n_rho(S)), lib=lib) == cc.check_srs(t, rho=_rho(4545, _n_rho(S)), lib=lib)


# ---- 7. at size, on the GPU ---------------------------------------------------------------------------------
_gpu = {}


def _srs16(cc, lib):
    if "srs" not in _gpu:
        _gpu["srs"] = cc.trapdoor_srs(16, _tox3(1616), lib=lib)
    return _gpu["srs"]


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    print(f"check_srs: {dt:.3f} s")
    assert dt < GUARD_S, f"check_srs took {dt:.1f} s: hang guard {GUARD_S} s (not a performance gate)"
    return out


@pytest.mark.gpu
def test_srs_2_16_passes_gpu(gpulib):
    import circom_compat_amd as cc
    srs = _srs16(cc, gpulib)
    cc.check_srs(cc.trapdoor_srs(4, _tox3(4), lib=gpulib), lib=gpulib)                    # warm-up: module load
    rep = _timed(lambda: cc.check_srs(srs, lib=gpulib))
    assert rep.ok and rep.relations_checked and rep.bad_points == [], rep
    assert rep.n_points == dict(tau_g1=(1 << 17) - 1, tau_g2=1 << 16, alpha_tau_g1=1 << 16, beta_tau_g1=1 << 16, singles=1)
    assert all(v == 0 for v in rep.n_infinity.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", [("tau_g1", (1 << 17) - 2), ("tau_g1", 1 << 14), ("tau_g1", (1 << 14) - 1),
                                    ("tau_g2", (1 << 16) - 1), ("tau_g2", 3 << 14), ("alpha_tau_g1", (1 << 16) - 1),
                                    ("alpha_tau_g1", (1 << 15) - 1), ("beta_tau_g1", (1 << 16) - 1),
                                    ("beta_tau_g1", 1 << 15)])
def test_srs_2_16_planted_faults_gpu(gpulib, monkeypatch, name, i):
    """one entry replaced by another element of its group (entry i - 2 of the same array): that array's relation
    fails alone, in chunks of 2^14 (the index sits on a seam or at the end of its array) and in one chunk; then the
    same entry made malformed is located.  The arrays are shorter than 2^18: no seam of the default chunk exists."""
    import circom_compat_amd as cc
    srs = _copy_srs(cc, _srs16(cc, gpulib))
    getattr(srs, name)[i] = getattr(srs, name)[i - 2]
    monkeypatch.setenv("G16_SRSCHECK_CHUNK", str(1 << 14))
    rep = _timed(lambda: cc.check_srs(srs, lib=gpulib))
    assert not rep.ok and rep.relations_checked and rep.relations_failed == ARRAY_BIT[name], rep
    monkeypatch.delenv("G16_SRSCHECK_CHUNK")
    assert _timed(lambda: cc.check_srs(srs, lib=gpulib)).relations_failed == ARRAY_BIT[name]
    planted = _plant(srs, name, i, "cofactor" if name == "tau_g2" else "offcurve")
    rep = _timed(lambda: cc.check_srs(srs, lib=gpulib))
    assert rep.bad_points == [planted] and not rep.relations_checked and sum(rep.n_bad.values()) == 1


@pytest.mark.gpu
def test_live_prover_is_untouched_gpu(gpulib):
    """a Prover alive on the device proves the same bytes before and after check_srs calls on that device"""
    import circom_compat_amd as cc
    sys.path.insert(0, ROOT)
    import bench
    mats, (A, Bm, Cm), w, n_vars = bench.chain_circuit(cc, 12)
    rng = random.Random(1212)
    pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, R) for _ in range(5)])
    pr = cc.Prover(pk, mats, lib=gpulib)
    r, s = 1234567, 7654321
    before = pr.prove(r, s, w)
    srs = cc.trapdoor_srs(12, _tox3(12), lib=gpulib)
    assert _timed(lambda: cc.check_srs(srs, lib=gpulib)).ok
    bad = _copy_srs(cc, srs)
    _plant(bad, "tau_g2", 77, "offcurve")
    assert not cc.check_srs(bad, lib=gpulib).ok
    assert pr.prove(r, s, w).raw == before.raw
    pr.close()
