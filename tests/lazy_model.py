"""Exact integer model of field29.h / ec29.h and the ctypes side of tests/arith/arith_hooks.hip.

Test infrastructure shared by test_lazy_field.py and test_lazy_ec.py.  Everything here is plain Python
integers: value(limbs) = sum l_i 2^(29 i), the Montgomery product's EXACT result (T + m p) / 2^261, and the
limb / value classes the two headers document."""
import ctypes as C
import os

import numpy as np

import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_HOOKS = os.path.join(ROOT, "tests", "arith", "libg16_arith_gpu.so")

LIMB = 1 << 29
RP = 1 << 261                                   # the internal Montgomery radix
# what a 64-bit column can take (F29_CHECK asserts exactly this): the m p terms add up to 9 * 2^58, the carry 2^36
COL_MAX = (1 << 63) - (9 << 58) - (1 << 36)
assert COL_MAX < 2 ** 62.9                      # inside the bound the header states
INT32 = 1 << 31

FIELDS = {"fq": (0, o.Q_MOD, 9), "fr": (1, o.R_MOD, 9), "fq2": (2, o.Q_MOD, 18)}
(F_MUL, F_SQR, F_MUL2, F_MUL_SUB, F_CARRY, F_CANONICAL, F_IS_ZERO, F_MAYBE_ZERO, F_PACK, F_UNPACK, F_FROM_MONT,
 F_TO_MONT, F_PACK_INTERNAL, F_LOAD_PACKED, F_STORE_PACKED, F_INV, F_INV_VARTIME) = range(17)
(E_MADD, E_MADD_SELECT, E_MADD_RARE, E_ADD, E_DBL, E_DBL_AFFINE, E_NEG, E_FROM_AFFINE, E_TO_AFFINE,
 E_TO_AFFINE_VARTIME, E_AFFINE_FROM_MONT, E_XYZZ_TO_MONT, E_STORE_PACKED_AFFINE, E_LOAD_PACKED_AFFINE,
 E_CHAIN) = range(15)
CHAIN_STEPS = 32


# ---- limbs <-> integers ------------------------------------------------------------------------------------------
def value(limbs):
    return sum(int(l) << (29 * i) for i, l in enumerate(limbs))


def norm(v):
    """limbs 0..7 in [0, 2^29), the (signed) top limb takes the rest"""
    return [(v >> (29 * i)) & (LIMB - 1) for i in range(8)] + [v >> 232]


def edge(sign_of, mag, target):
    """limbs 0..7 at sign_of(i) * mag, the top limb chosen so that the value is `target` to within 2^232"""
    low = [sign_of(i) * mag for i in range(8)]
    return low + [(target - value(low)) >> 232]


PLUS, MINUS, ALT = (lambda i: 1), (lambda i: -1), (lambda i: 1 if i % 2 == 0 else -1)
SIGNS = (PLUS, MINUS, ALT)


def words(v, n=8):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def from_words(w):
    return sum((int(x) & 0xffffffff) << (32 * i) for i, x in enumerate(w))


def carry(l):
    """F29::carry on Python integers (arithmetic shifts, as on int32)"""
    r = [l[0] & (LIMB - 1)]
    for i in range(1, 8):
        r.append((l[i] & (LIMB - 1)) + (l[i - 1] >> 29))
    r.append(l[8] + (l[7] >> 29))
    return r


# ---- the Montgomery product ---------------------------------------------------------------------------------------
def mont_exact(T, p):
    """(T + m p) / 2^261 with m = -T / p mod 2^261: the exact integer a reduction returns"""
    m = (-T * pow(p, -1, RP)) % RP
    assert (T + m * p) % RP == 0
    return (T + m * p) >> 261


def in_contract(products, p):
    """products: [(a, b), ...] limb vectors whose products ONE reduction sums (1 for *, 2 for mul2 / mul_sub)"""
    for a, b in products:
        if any(abs(x) >= INT32 for x in list(a) + list(b)):
            return False
    for k in range(17):
        s = 0
        for a, b in products:
            s += sum(abs(a[i]) * abs(b[k - i]) for i in range(9) if 0 <= k - i < 9)
        if s >= COL_MAX:
            return False
    return 10 * sum(abs(value(a) * value(b)) for a, b in products) < 1688 * p * p       # < 168.8 p^2


def is_m_class(l, p):
    return all(0 <= x < LIMB for x in l[:8]) and abs(l[8]) < (1 << 24) and -p < value(l) < 2 * p


def in_class(l, p, lo, hi, slack):
    """limbs 0..7 in [-slack, 2^29 + slack), value in (lo p, hi p)"""
    return all(-slack <= x < LIMB + slack for x in l[:8]) and lo * p < value(l) < hi * p


# ---- the hook library ---------------------------------------------------------------------------------------------
class Hooks:
    def __init__(self, cdll):
        self.L = cdll
        ip = C.c_void_p
        for name in ("arith_f29_op", "arith_ec29_op"):
            fn = getattr(cdll, name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_int, C.c_int, ip, ip, ip, C.c_size_t]

    def field(self, fname, op, cases):
        """cases: per case up to 4 operands of W limbs (or words).  Returns (n x W int64 array, flags)"""
        fid, _, W = FIELDS[fname]
        n = len(cases)
        buf = np.zeros((n, 4, W), dtype=np.int64)
        for i, ops in enumerate(cases):
            for j, x in enumerate(ops):
                buf[i, j, :len(x)] = x
        assert np.all(buf < (1 << 32)) and np.all(buf >= -INT32)
        arr = np.ascontiguousarray(buf.astype(np.uint32).view(np.int32))      # limbs and 32-bit words alike
        out = np.full((n, W), 0x5a5a5a5a, dtype=np.int32)
        flag = np.full(n, -1, dtype=np.int32)
        st = self.L.arith_f29_op(fid, op, arr.ctypes.data, out.ctypes.data, flag.ctypes.data, n)
        assert st == 0, f"arith_f29_op({fname}, {op}) returned {st}"
        return out.astype(np.int64), flag

    def ec(self, g2, op, cases):
        """cases: dicts with acc / q (4 x W limbs), p (2 x W limbs or words), inf.  Returns (out, flags)"""
        W = 18 if g2 else 9
        n = len(cases)
        buf = np.zeros((n, 10 * W + 1), dtype=np.int64)
        for i, c in enumerate(cases):
            for key, off in (("acc", 0), ("q", 4 * W), ("p", 8 * W)):
                flat = [x for part in c.get(key, ()) for x in part]
                buf[i, off:off + len(flat)] = flat
            buf[i, 10 * W] = 1 if c.get("inf") else 0
        assert np.all(buf < (1 << 32)) and np.all(buf >= -INT32)
        arr = np.ascontiguousarray(buf.astype(np.uint32).view(np.int32))      # limbs and 32-bit words alike
        per = 4 * W * (CHAIN_STEPS if op == E_CHAIN else 1)
        out = np.full((n, per), 0x5a5a5a5a, dtype=np.int32)
        flag = np.full(n, -1, dtype=np.int32)
        st = self.L.arith_ec29_op(int(g2), op, arr.ctypes.data, out.ctypes.data, flag.ctypes.data, n)
        assert st == 0, f"arith_ec29_op({g2}, {op}) returned {st}"
        return out.astype(np.int64), flag


def load_hooks(request):
    """the module fixtures' body: "emu" = the hooks inside the emulator library (F29_CHECK on), "gpu" = the hipcc
    build, which build() leaves next to the source -- missing there is a failure, never a skip or a compile"""
    if request.param == "emu":
        return Hooks(request.getfixturevalue("emu").L)
    import pytest
    if not os.path.exists(GPU_HOOKS):
        pytest.fail(f"{GPU_HOOKS} is not built (make -C circom_compat_amd/csrc)")
    return Hooks(C.CDLL(GPU_HOOKS))
