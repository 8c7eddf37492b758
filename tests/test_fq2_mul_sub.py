"""F29x2::mul_sub(a, b, c, d) = a b - c d over the lazy 29-bit limbs (field29.h) -- the Y3 of every G2 addition and
doubling -- with ONE Montgomery reduction per component: four limb products per column, their left operands
re-centred so that the 64-bit column holds (F29::recentre, F29::mul4).

Directly, on raw limb patterns through the emulator build (tests/emu/emu_fq2_mul_sub_exports.cpp; its F29_CHECK
asserts abort the process on a column or value overflow): the result == the integers' (a b - c d) / 2^261 mod p,
lies in the class ec29.h stores a y in, and == the split form (a * b - c * d).carry() wherever that form's own,
narrower, contract admits the operands.  The product library exports no such hook, so the GPU legs reach the routine
through the G2 operations that call it: a 64-point G2 MSM (madd in the accumulation; add and dbl_in_place in the
bucket reduction and k_horner)."""
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
# field29.h, F29x2::mul_sub: |a0 b0| + |a1 b1| + |c0 d0| + |c1 d1| < 337 p^2, and the same for the crossed pairs
VALUE_BOUND = 337
# ec29.h, the five call sites: a = R (madd, add: |v| < 10 p) or Mm (doublings: < 6 p); b = Q - X3 (< 9 p) or S - X3;
# c = the stored y (< 3 p), S1 or W (products: in (-p, 2p)); d = PPP (a product) or the stored y
A_MAX, B_MAX, C_MAX, D_MAX = 10 * P, 9 * P, 3 * P, 3 * P


def _value(limbs):
    return sum(int(l) << (29 * i) for i, l in enumerate(limbs))


def _canonical_limbs(v):
    return [(v >> (29 * i)) & (LIMB - 1) for i in range(9)]


def _edge_limbs(sign_of, target):
    """limbs 0..7 at +-EDGE (sign_of(i)), the top limb chosen so that the value is `target` rounded towards zero to
    a multiple of 2^232 (so a target AT a bound stays inside it)"""
    low = [sign_of(i) * EDGE for i in range(8)]
    rest = target - _value(low)
    top = rest >> 232 if target >= 0 else -((-rest) >> 232)
    return low + [top]


PLUS, MINUS, ALT = (lambda i: 1), (lambda i: -1), (lambda i: 1 if i % 2 == 0 else -1)


def _fq2(sign0, sign1, t0, t1):
    return _edge_limbs(sign0, t0) + _edge_limbs(sign1, t1)


def _canon2(rng):
    return _canonical_limbs(rng.randrange(P)) + _canonical_limbs(rng.randrange(P))


def _cases():
    """each case: (a, b, c, d), every operand 18 limbs (c0 | c1)"""
    rng = random.Random(2908)
    cases = []
    for _ in range(24):                                           # canonical operands
        cases.append(tuple(_canon2(rng) for _ in range(4)))
    # every limb 0..7 of every operand at +-(2^29 + 8), in the sign patterns +, -, alternating (the same pattern on
    # both sides of a product puts every term of a column on one side of zero), values at the call sites' extremes:
    # both components of a at +-10 p, of b at +-9 p, of c and d at +-3 p
    for sa in (PLUS, MINUS, ALT):
        for sb in (PLUS, MINUS, ALT):
            for va, vb, vc, vd in ((1, 1, 1, 1), (1, 1, -1, 1), (-1, 1, 1, 1), (1, -1, -1, -1), (-1, -1, 1, -1)):
                cases.append((_fq2(sa, sa, va * A_MAX, va * A_MAX), _fq2(sb, sb, vb * B_MAX, vb * B_MAX),
                              _fq2(sa, sb, vc * C_MAX, -vc * C_MAX), _fq2(sb, sa, vd * D_MAX, vd * D_MAX)))
    # the same limb patterns at the values a madd really holds (R = S2 - y: below 5 p), which the split form admits
    for sa in (PLUS, MINUS, ALT):
        for sb in (PLUS, MINUS, ALT):
            for va, vc in ((1, 1), (-1, 1)):
                cases.append((_fq2(sa, sa, va * 5 * P, 5 * P), _fq2(sb, sb, B_MAX, -B_MAX),
                              _fq2(sa, sb, vc * C_MAX, C_MAX), _fq2(sb, sa, 2 * P, -2 * P)))
    # components of opposite extremes: c0 = a0 b0 - a1 b1 - ... adds where the case above cancels, and conversely
    for sa in (PLUS, MINUS, ALT):
        cases.append((_fq2(sa, sa, A_MAX, -A_MAX), _fq2(sa, sa, B_MAX, -B_MAX),
                      _fq2(sa, sa, -C_MAX, C_MAX), _fq2(sa, sa, D_MAX, -D_MAX)))
        cases.append((_fq2(sa, sa, A_MAX, A_MAX), _fq2(sa, sa, B_MAX, -B_MAX),
                      _fq2(sa, sa, C_MAX, C_MAX), _fq2(sa, sa, -D_MAX, D_MAX)))
    # what the call sites hold at their value extremes with ordinary limbs: a canonical value + k p
    def shifted(k0, k1):
        return _lift(rng.randrange(P), k0) + _lift(rng.randrange(P), k1)
    for ka, kb, kc, kd in ((9, 8, 2, 2), (-10, 8, -3, 2), (9, -9, 2, -3), (-10, -9, -3, -3), (5, 6, 1, 2)):
        cases.append((shifted(ka, ka), shifted(kb, kb), shifted(kc, kc), shifted(kd, kd)))
    for _ in range(6):                                            # a b = c d exactly: the difference is zero
        a, b = _canon2(rng), _canon2(rng)
        cases.append((a, b, list(a), list(b)))
        cases.append((a, b, list(b), list(a)))
    e, f = _fq2(ALT, MINUS, -3 * P, 2 * P), _fq2(PLUS, ALT, 3 * P, -2 * P)
    cases.append((e, f, list(e), list(f)))
    cases.append((e, f, [-x for x in e], [-x for x in f]))
    top = A_MAX >> 232                                            # the top limbs at their bounds, the others zero / maximal
    z = [0] * 8
    cases.append((z + [top] + z + [-top], z + [B_MAX >> 232] + z + [B_MAX >> 232],
                  z + [C_MAX >> 232] + z + [C_MAX >> 232], z + [-(D_MAX >> 232)] + z + [D_MAX >> 232]))
    cases.append(tuple(([LIMB - 1] * 8 + [(C_MAX >> 232) - 1]) * 2 for _ in range(4)))
    cases.append(tuple([0] * 18 for _ in range(4)))               # all-zero operands
    cases.append(([0] * 18, _canon2(rng), _canon2(rng), [0] * 18))
    return cases


def _lift(v, k):
    """v + k p with limbs 0..7 normalised, the top limb taking the rest"""
    v += k * P
    low = [(v >> (29 * i)) & (LIMB - 1) for i in range(8)]
    return low + [(v - _value(low)) >> 232]


def _words_to_int(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def _run(emu, cases, split):
    n = len(cases)
    limbs = np.array([a + b + c + d for a, b, c, d in cases], dtype=np.int32).reshape(n, 72)
    out = np.zeros((n, 16), dtype=np.uint32)
    raw = np.zeros((n, 18), dtype=np.int32)
    fn = emu.L.emu_fq2x29_mul_sub
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn(limbs.ctypes.data, out.ctypes.data, raw.ctypes.data, n, 1 if split else 0)
    return out, raw


def _halves(x):
    return _value(x[:9]), _value(x[9:])


def _value_sums(a, b, c, d):
    """the two sums of |value products| that mul_sub's contract bounds, in units of p^2"""
    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = _halves(a), _halves(b), _halves(c), _halves(d)
    s0 = abs(a0 * b0) + abs(a1 * b1) + abs(c0 * d0) + abs(c1 * d1)
    s1 = abs(a0 * b1) + abs(a1 * b0) + abs(c0 * d1) + abs(c1 * d0)
    return s0 / (P * P), s1 / (P * P)


def _want(a, b, c, d):
    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = _halves(a), _halves(b), _halves(c), _halves(d)
    return ((a0 * b0 - a1 * b1 - c0 * d0 + c1 * d1) * RINV % P, (a0 * b1 + a1 * b0 - c0 * d1 - c1 * d0) * RINV % P)


def test_fq2_mul_sub_on_limb_patterns_vs_integers_and_the_split_form(emu):
    cases = _cases()
    for a, b, c, d in cases:                 # every case inside the documented contract of mul_sub
        for x in (a, b, c, d):
            assert len(x) == 18 and all(abs(l) <= EDGE for l in x[:8] + x[9:17])
        for x, bound in ((a, A_MAX), (b, B_MAX), (c, C_MAX), (d, D_MAX)):
            assert max(abs(v) for v in _halves(x)) <= bound
        assert max(_value_sums(a, b, c, d)) < VALUE_BOUND
    assert max(max(_value_sums(*k)) for k in cases) > 190          # ... and the call sites' worst (192 p^2) is reached
    got, raw = _run(emu, cases, split=False)
    for i, (a, b, c, d) in enumerate(cases):
        assert (_words_to_int(got[i, :8]), _words_to_int(got[i, 8:])) == _want(a, b, c, d), i
        for comp in (raw[i, :9], raw[i, 9:]):                      # the class of a stored y (ec29.h), and tighter
            assert all(0 <= int(l) < LIMB for l in comp[:8]), i
            assert abs(int(comp[8])) < 1 << 24, i
            assert -2 * P < _value(comp) < 3 * P, i
    # the split form multiplies a by b and c by d as two Fq2 products of their own: |a0 b0| + |a1 b1| < 168.9 p^2 each
    old = [k for k in cases if max(_value_sums(k[0], k[1], [0] * 18, [0] * 18)) < 168 and
           max(_value_sums([0] * 18, [0] * 18, k[2], k[3])) < 168]
    assert sum(1 for k in old if all(abs(l) == EDGE for x in k for l in x[:8] + x[9:17])) >= 18   # edge limbs too
    got_old, _ = _run(emu, old, split=True)
    for i, k in enumerate(old):
        assert (_words_to_int(got_old[i, :8]), _words_to_int(got_old[i, 8:])) == _want(*k), i


def test_recentred_limbs_keep_the_column_inside_64_bits():
    """the bound field29.h states, from the integers: 36 products of a re-centred limb (|l| <= 2^28 + 1) with a limb
    within +-(2^29 + 2^4), the reduction's 9 m_i p_j < 2^58 and the carry of the column before stay below 2^63"""
    col = 36 * ((1 << 28) + 1) * ((1 << 29) + 16) + 9 * (1 << 58)
    assert col + (col >> 29) + 1 < 1 << 63
    for l in (-EDGE - 8, -EDGE, -(1 << 28) - 1, -(1 << 28), -1, 0, 1, (1 << 28) - 1, 1 << 28, LIMB - 1, LIMB, EDGE, EDGE + 8):
        lo = ((l + (1 << 28)) % LIMB) - (1 << 28)                  # the sign-extended 29-bit field
        hi = (l - lo) >> 29
        assert -(1 << 28) <= lo < 1 << 28 and hi in (-1, 0, 1) and lo + (hi << 29) == l


@pytest.fixture(scope="module")
def g2_case():
    """64 G2 points (distinct multiples, one at infinity, repeated points) and scalars with repeated, zero and
    extreme entries; the expected sum is computed once"""
    rng = random.Random(65)
    base = H.rand_g2(rng, 4)
    n = 64
    B2 = [None] + [o.G2.mul(base[i % 4], i + 3) if i != 23 else None for i in range(n)]
    g1 = H.rand_g1(rng, 3)
    scal = H.rand_fr(rng, n)
    scal[0], scal[1], scal[2] = 0, 1, o.R_MOD - 1
    scal[7] = scal[8] = scal[9] = scal[10]            # equal scalars: the points meet in one bucket
    B2[9], B2[10], B2[11] = B2[8], B2[8], o.G2.neg(B2[8])   # P + P (the doubling branch of add / madd) and P - P in a bucket
    scal[40] = scal[41] = 1
    B2[42] = B2[41]                                   # a doubling in bucket 1 as well
    want = o.g2_to_bytes(o.G2.msm(B2[1:], scal))
    return dict(B2=B2, g1=g1, g2=base, scal=scal, want=want, n=n)


@pytest.mark.parametrize("wb,planes", [(8, 0), (8, 2), (4, 1)])
def test_g2_msm_64_points_vs_oracle(lib, g2_case, wb, planes):
    """madd (accumulation), add / dbl_in_place (bucket reduction at window_bits = 8; with fewer planes than
    windows k_horner doubles between the folded bucket sets): every one forms its Y3 with mul_sub"""
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
