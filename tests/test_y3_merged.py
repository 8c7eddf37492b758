"""mul_sub_y3(a, b, c, d) = a b - c d (field29.h), the name under which ec29.h forms every Y3: for Fq2 the merged form
(one reduction per component, F29x2::mul_sub_merged), for Fq mul_sub itself.  tests/test_fq2_mul_sub.py drives the
merged form at the operand shapes of madd; here the shapes of the two formula sites it does not drive:

  add           a = R = S2 - S1 (|v| < 3p), b = Q - X3 in (-6p, 9p), c = S1 and d = PPP products in (-p, 2p)
  dbl_in_place  a = Mm = 3 X^2 carried, in (-3p, 6p), b = S - X3 in (-5p, 7p), c = W a product, d = the stored y (< 3p)

with limbs 0..7 of every operand at the extremes +-(2^29 + 8) in the sign patterns that put all terms of a column on
one side of zero, and with ordinary limbs at the value extremes.  Through the emulator build
(tests/emu/emu_y3_exports.cpp; F29_CHECK aborts on a column or value overflow): the result == the integers'
(a b - c d) / 2^261 mod p == the split form's, and lies in (-2p, 3p) with limbs 0..7 in [0, 2^29) -- the class ec29.h
stores a y in.  (The two sites themselves keep the split mul_sub for the registers of k_bucket_reduce<Fq2>, ec29.h; the
bounds hold either way.)  The product library exports no such hook: there (and on the emulator) a G2 MSM with fewer planes than
windows runs add in the bucket reduction and dbl_in_place in k_horner on real operands."""
import ctypes as C
import random

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_fq2_mul_sub import (ALT, EDGE, LIMB, MINUS, P, PLUS, _fq2, _halves, _lift, _value, _value_sums, _want,
                              _words_to_int)

# (|a|, b below, b above, |c| as a product or a stored y, |d|) in units of p, per component
SHAPES = {
    "add": dict(a=3, b_lo=-6, b_hi=9, c=2, d=2),
    "dbl_in_place": dict(a=6, b_lo=-5, b_hi=7, c=2, d=3),
}
# the split form multiplies a by b and c by d as Fq2 products of their own: |x0 y0| + |x1 y1| < 168.9 p^2 each
SPLIT_BOUND = 168


def _cases(shape):
    s = SHAPES[shape]
    rng = random.Random(2909 + len(shape))
    cases = []
    for sa in (PLUS, MINUS, ALT):
        for sb in (PLUS, MINUS, ALT):
            for va, vb, vc, vd in ((1, 1, 1, 1), (1, 1, -1, 1), (-1, 1, 1, 1), (1, -1, -1, -1), (-1, -1, 1, -1)):
                b = (s["b_hi"] if vb > 0 else s["b_lo"]) * P
                cases.append((_fq2(sa, sa, va * s["a"] * P, va * s["a"] * P), _fq2(sb, sb, b, b),
                              _fq2(sa, sb, vc * s["c"] * P, -vc * s["c"] * P), _fq2(sb, sa, vd * s["d"] * P, vd * s["d"] * P)))
        # components of opposite extremes: c0 adds where the case above cancels, and conversely
        cases.append((_fq2(sa, sa, s["a"] * P, -s["a"] * P), _fq2(sa, sa, s["b_hi"] * P, s["b_lo"] * P),
                      _fq2(sa, sa, -s["c"] * P, s["c"] * P), _fq2(sa, sa, s["d"] * P, -s["d"] * P)))

    def shifted(k0, k1):                                          # a canonical value + k p, ordinary limbs
        return _lift(rng.randrange(P), k0) + _lift(rng.randrange(P), k1)
    for _ in range(12):
        ka, kc, kd = (rng.randrange(-s[x], s[x]) for x in ("a", "c", "d"))
        kb = rng.randrange(s["b_lo"], s["b_hi"])
        cases.append((shifted(ka, -ka - 1), shifted(kb, kb), shifted(kc, kc), shifted(kd, -kd - 1)))
    cases.append(tuple([0] * 18 for _ in range(4)))
    return cases


def _run2(emu, cases):
    n = len(cases)
    limbs = np.array([a + b + c + d for a, b, c, d in cases], dtype=np.int32).reshape(n, 72)
    out, split = np.zeros((n, 16), dtype=np.uint32), np.zeros((n, 16), dtype=np.uint32)
    raw = np.zeros((n, 18), dtype=np.int32)
    fn = emu.L.emu_fq2x29_mul_sub_y3
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn(limbs.ctypes.data, out.ctypes.data, raw.ctypes.data, split.ctypes.data, n)
    return out, raw, split


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fq2_y3_vs_integers_and_the_split_form(emu, shape):
    s = SHAPES[shape]
    cases = _cases(shape)
    for a, b, c, d in cases:                                      # every case inside the site's own bounds
        for x in (a, b, c, d):
            assert len(x) == 18 and all(abs(l) <= EDGE for l in x[:8] + x[9:17])
        assert max(abs(v) for v in _halves(a)) <= s["a"] * P
        assert all(s["b_lo"] * P <= v <= s["b_hi"] * P for v in _halves(b))
        assert max(abs(v) for v in _halves(c)) <= s["c"] * P and max(abs(v) for v in _halves(d)) <= s["d"] * P
        zero = [0] * 18
        assert max(_value_sums(a, b, zero, zero)) < SPLIT_BOUND and max(_value_sums(zero, zero, c, d)) < SPLIT_BOUND
    assert sum(1 for k in cases if all(abs(l) == EDGE for x in k for l in x[:8] + x[9:17])) >= 45
    got, raw, split = _run2(emu, cases)
    for i, k in enumerate(cases):
        want = _want(*k)
        assert (_words_to_int(got[i, :8]), _words_to_int(got[i, 8:])) == want, (shape, i)
        assert (_words_to_int(split[i, :8]), _words_to_int(split[i, 8:])) == want, (shape, i, "split")
        for comp in (raw[i, :9], raw[i, 9:]):
            assert all(0 <= int(l) < LIMB for l in comp[:8]), (shape, i)
            assert abs(int(comp[8])) < 1 << 24, (shape, i)
            assert -2 * P < _value(comp) < 3 * P, (shape, i)


def test_fq_y3_is_mul_sub(emu):
    """G1: one reduction already -- the same limbs as mul_sub, the integers' value, the M class"""
    rng = random.Random(77)
    rinv = pow(1 << 261, -1, P)
    cases = []
    for shape in sorted(SHAPES):
        for a, b, c, d in _cases(shape):
            cases.append((a[:9], b[:9], c[:9], d[:9]))
    cases += [tuple(_lift(rng.randrange(P), 0) for _ in range(4)) for _ in range(8)]
    n = len(cases)
    limbs = np.array([a + b + c + d for a, b, c, d in cases], dtype=np.int32).reshape(n, 36)
    out, sub = np.zeros((n, 8), dtype=np.uint32), np.zeros((n, 8), dtype=np.uint32)
    raw = np.zeros((n, 9), dtype=np.int32)
    fn = emu.L.emu_fq29_mul_sub_y3
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn(limbs.ctypes.data, out.ctypes.data, raw.ctypes.data, sub.ctypes.data, n)
    for i, (a, b, c, d) in enumerate(cases):
        want = (_value(a) * _value(b) - _value(c) * _value(d)) * rinv % P
        assert _words_to_int(out[i]) == want == _words_to_int(sub[i]), i
        assert all(0 <= int(l) < LIMB for l in raw[i, :8]) and -P < _value(raw[i]) < 2 * P, i


@pytest.fixture(scope="module")
def g2_case():
    """48 G2 points, one at infinity, a repeated and a negated one under equal scalars; the expected sum once"""
    import cpu_ref
    rng = random.Random(4809)
    n = 48
    B2 = cpu_ref.g2_mul_batch(o.g2_to_bytes(o.G2_GEN), [rng.randrange(1, o.R_MOD) for _ in range(n + 1)])
    B2[6] = 0
    B2[13] = B2[12]
    B2[15] = np.frombuffer(o.g2_to_bytes(o.G2.neg(o.g2_from_bytes(bytes(B2[14])))), dtype=np.uint8)
    scal = H.rand_fr(rng, n)
    scal[0], scal[1], scal[2] = 0, 1, o.R_MOD - 1
    scal[11] = scal[12] = scal[13] = scal[14]         # wires 12 .. 15 (B2[1:] holds wire 1 first): P, P, Q, -Q
    want = cpu_ref.msm_g2(np.ascontiguousarray(B2[1:]), H.fr_mont_arr(scal))
    return dict(B2=B2, scal=scal, want=want, n=n)


@pytest.mark.parametrize("wb,planes", [(4, 1), (8, 2)])
def test_g2_msm_through_add_and_dbl_in_place(lib, g2_case, wb, planes):
    import circom_compat_amd as cc
    import cpu_ref
    c = g2_case
    N = c["n"] + 1
    g1 = cpu_ref.g1_mul_batch(o.g1_to_bytes(o.G1_GEN), list(range(2, N + 6)))
    g2 = cpu_ref.g2_mul_batch(o.g2_to_bytes(o.G2_GEN), [3, 5, 7])
    vk = cc.VerifyingKey(g1[0].tobytes(), g2[0].tobytes(), g2[1].tobytes(), g2[2].tobytes(), g1[:2].copy())
    pk = cc.ProvingKey(N, 1, 4, vk, g1[1].tobytes(), g1[2].tobytes(), g1[:N].copy(), g1[:N].copy(), c["B2"],
                       g1[2:N].copy(), g1[:4].copy())
    mats = H.matrices_from_rows([[(1, 1)]], [[(1, 0)]], 2, N, lib)
    pr = cc.Prover(pk, mats, lib=lib, window_bits=wb, planes=planes)
    assert pr.msm_g2(c["scal"]) == c["want"]
    pr.close()
