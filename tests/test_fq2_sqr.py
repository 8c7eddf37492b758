"""F29x2::sqr -- the complex squaring (c0 + c1)(c0 - c1) | 2 c0 c1 over the lazy 29-bit limbs (field29.h).

Directly, on raw limb patterns through the emulator build (tests/emu/emu_f29_exports.cpp; its F29_CHECK asserts
abort the process on a column or value overflow): sqr(a) == a * a == the integers' (v0 + v1 i)^2 / 2^261 mod p.
The product library exports no such hook, so the GPU legs reach the squaring through the G2 operations that use
it: a 64-point G2 MSM (madd in the accumulation; add and dbl_in_place in the bucket reduction and k_horner)."""
import ctypes as C
import random

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

P = o.Q_MOD
RINV = pow(1 << 261, -1, P)
LIMB = 1 << 29
EDGE = LIMB + 8                      # |limb| bound of a carried value / of a difference of two products (ec29.h)


def _value(limbs):
    return sum(int(l) << (29 * i) for i, l in enumerate(limbs))


def _canonical_limbs(v):
    return [(v >> (29 * i)) & (LIMB - 1) for i in range(9)]


def _edge_limbs(sign_of, target):
    """limbs 0..7 at +-EDGE (sign_of(i)), the top limb chosen so that the value is about `target`"""
    low = [sign_of(i) * EDGE for i in range(8)]
    top = (target - _value(low)) >> 232
    return low + [top]


def _cases():
    rng = random.Random(2907)
    cases = []
    for _ in range(24):                                           # canonical operands
        cases.append((_canonical_limbs(rng.randrange(P)), _canonical_limbs(rng.randrange(P))))
    plus, minus, alt = (lambda i: 1), (lambda i: -1), (lambda i: 1 if i % 2 == 0 else -1)
    for s0 in (plus, minus, alt):                                 # every limb at +-(2^29 + 8), values about +-8 p
        for s1 in (plus, minus, alt):
            for t0, t1 in ((8 * P, 8 * P), (8 * P, -8 * P), (-8 * P, 3 * P), (0, 8 * P), (-8 * P, 0), (P // 3, -5 * P)):
                cases.append((_edge_limbs(s0, t0), _edge_limbs(s1, t1)))
    top = 8 * P >> 232                                            # the top limb at its bound, the others zero / maximal
    cases.append(([0] * 8 + [top], [0] * 8 + [-top]))
    cases.append(([LIMB - 1] * 8 + [top], [LIMB - 1] * 8 + [top]))
    for _ in range(6):                                            # c0 = +-c1: one factor is zero
        a = _canonical_limbs(rng.randrange(P))
        cases.append((a, list(a)))
        cases.append((a, [-x for x in a]))
    e = _edge_limbs(alt, -7 * P)
    cases.append((e, list(e)))
    cases.append((e, [-x for x in e]))
    cases.append(([0] * 9, [0] * 9))
    return cases


def _words_to_int(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def test_fq2_sqr_on_limb_patterns_vs_integers(emu):
    cases = _cases()
    for c0, c1 in cases:                     # what the call sites can produce, and within the contract of `*`
        assert all(abs(x) <= EDGE for x in c0[:8] + c1[:8])
        assert max(abs(_value(c0)), abs(_value(c1))) < 9 * P
    n = len(cases)
    limbs = np.array([c0 + c1 for c0, c1 in cases], dtype=np.int32)
    got_sqr = np.zeros((n, 16), dtype=np.uint32)
    got_mul = np.zeros((n, 16), dtype=np.uint32)
    fn = emu.L.emu_fq2x29_sqr
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn(limbs.ctypes.data, got_sqr.ctypes.data, got_mul.ctypes.data, n)
    for i, (c0, c1) in enumerate(cases):
        v0, v1 = _value(c0), _value(c1)
        want = ((v0 * v0 - v1 * v1) * RINV % P, 2 * v0 * v1 * RINV % P)
        assert (_words_to_int(got_sqr[i, :8]), _words_to_int(got_sqr[i, 8:])) == want, i
        assert (_words_to_int(got_mul[i, :8]), _words_to_int(got_mul[i, 8:])) == want, i


@pytest.fixture(scope="module")
def g2_case():
    """64 G2 points (distinct multiples, one at infinity) and scalars with repeated, zero and extreme entries; the
    expected sum is computed once"""
    rng = random.Random(64)
    base = H.rand_g2(rng, 4)
    n = 64
    B2 = [None] + [o.G2.mul(base[i % 4], i + 2) if i != 17 else None for i in range(n)]
    g1 = H.rand_g1(rng, 3)
    scal = H.rand_fr(rng, n)
    scal[0], scal[1], scal[2] = 0, 1, o.R_MOD - 1
    scal[3] = scal[4] = scal[5]                       # equal scalars: the points meet in one bucket
    B2[5], B2[6] = B2[4], o.G2.neg(B2[4])   # P + P (dbl) and P - P in a bucket
    want = o.g2_to_bytes(o.G2.msm(B2[1:], scal))
    return dict(B2=B2, g1=g1, g2=base, scal=scal, want=want, n=n)


@pytest.mark.parametrize("wb,planes", [(8, 0), (8, 2), (4, 1)])
def test_g2_msm_64_points_vs_oracle(lib, g2_case, wb, planes):
    """madd (accumulation), add / dbl_in_place (bucket reduction at window_bits = 8; with fewer planes than
    windows k_horner doubles between the folded bucket sets)"""
    import circom_compat_amd as cc
    c = g2_case
    N = c["n"] + 1
    A = [c["g1"][i % 3] for i in range(N)]
    pk = dict(n_vars=N, n_public=1, domain_size=4, alpha_g1=c["g1"][0], beta_g1=c["g1"][1], beta_g2=c["g2"][0],
              gamma_g2=c["g2"][1], delta_g1=c["g1"][2], delta_g2=c["g2"][2], ic=c["g1"][:2], a_query=A, b_g1_query=A,
              b_g2_query=c["B2"], l_query=A[2:], h_query=A[:4])
    mats = H.matrices_from_rows([[(1, 1)]], [[(1, 0)]], 2, N, lib)
    pr = cc.Prover(H.pk_from_oracle(pk), mats, lib=lib, window_bits=wb, planes=planes)
    assert pr.msm_g2(c["scal"]) == c["want"]
    pr.close()
