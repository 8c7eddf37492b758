"""toaffine.h's launcher and kernel, directly (tests/arith/arith_hooks.hip: arith_to_affine), on the emulator and on the
GPU: XYZZ -> canonical affine with one inversion per run of 8 points, contiguous and into record-strided slots.

Every input is built here from a known affine point (X, Y) and a nonzero z as (X z^2, Y z^3, z^2, z^3); the output
must be the storage form of (X, Y) as the oracle writes it, a point at infinity must come out as zero bytes, and
every byte between the slots must keep the guard pattern.

Lane t of block g owns the points g * 512 + k * 64 + t, k < 8 (toaffine.h); the totals sit around one wavefront of
lanes (63, 64, 65), around one full block of runs (511, 512, 513) and in a grid of three blocks with a ragged end
(1025)."""
import ctypes as C

import numpy as np
import pytest

import bn254_ref as o
import lazy_model as M

TOTALS = (0, 1, 63, 64, 65, 511, 512, 513, 1025)
MOST = max(TOTALS)
BLOCK, RUN = 64, 8
GUARD = 0xA5
REC = 256
OFFSETS = ((0, 192), (0, 128))   # G1: A and C of a proof record; G2: the two halves of a record


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks(request):
    h = M.load_hooks(request)
    h.L.arith_to_affine.restype = C.c_int
    h.L.arith_to_affine.argtypes = [C.c_int, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_size_t]
    return h


def _fq_words(v):
    return o.fq_to_mont_bytes(v)


def _build(g2):
    """MOST known affine points, their XYZZ forms with a z of their own, and their storage bytes; once per field"""
    curve, gen = (o.G2, o.G2_GEN) if g2 else (o.G1, o.G1_GEN)
    pt = 128 if g2 else 64
    P = curve.mul(gen, 0x1234567)
    xyzz = np.zeros((MOST, 4 * pt // 2), dtype=np.uint8)
    want = np.zeros((MOST, pt), dtype=np.uint8)
    z = 3 + (1 << 200)
    for j in range(MOST):
        z = (z * z + 5 * j + 1) % o.Q_MOD or 7          # nonzero, different for every point
        if g2:
            zc = (z, (z * 7 + j) % o.Q_MOD)
            zz = o.f2_sqr(zc)
            zzz = o.f2_mul(zz, zc)
            parts = (o.f2_mul(P[0], zz), o.f2_mul(P[1], zzz), zz, zzz)
            raw = b"".join(_fq_words(c) for part in parts for c in part)
            want[j] = np.frombuffer(o.g2_to_bytes(P), dtype=np.uint8)
        else:
            zz = z * z % o.Q_MOD
            zzz = zz * z % o.Q_MOD
            raw = b"".join(_fq_words(v) for v in (P[0] * zz, P[1] * zzz, zz, zzz))
            want[j] = np.frombuffer(o.g1_to_bytes(P), dtype=np.uint8)
        xyzz[j] = np.frombuffer(raw, dtype=np.uint8)
        P = curve.add(P, gen)
    xyzz.setflags(write=False)
    want.setflags(write=False)
    return xyzz, want


_built = {}


def built(g2):
    if g2 not in _built:
        _built[g2] = _build(g2)
    return _built[g2]


def infinite(pattern, total):
    """which of the `total` points are at infinity"""
    j = np.arange(total)
    lane, k = j % BLOCK, (j % (BLOCK * RUN)) // BLOCK
    if pattern == "edges":    # the first slot of lane 3's run, the last of lane 5's, both of lane 7's; and the last point
        inf = ((lane == 3) & (k == 0)) | ((lane == 5) & (k == RUN - 1)) | ((lane == 7) & ((k == 0) | (k == RUN - 1)))
        inf |= j == total - 1
        return inf
    if pattern == "run":      # the whole run of lane 9, in every block
        return lane == 9
    assert pattern == "all"
    return np.ones(total, dtype=bool)


@pytest.mark.parametrize("pattern", ["edges", "run", "all"])
@pytest.mark.parametrize("addressing", ["contiguous", "records"])
@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("g2", [0, 1], ids=["fq", "fq2"])
def test_to_affine(hooks, g2, total, addressing, pattern):
    xyzz, want = built(g2)
    pt = want.shape[1]
    inf = infinite(pattern, total)
    work = xyzz[:total].copy()
    work[inf, pt:] = 0                                   # zz = zzz = 0; x and y stay: only zzz decides
    expect_pts = want[:total].copy()
    expect_pts[inf] = 0
    if addressing == "contiguous":
        n, off0, off1, stride = total, 0, 0, pt
        size = total * pt + 48                           # a guard behind the last point
    else:
        n, stride = total // 2, REC
        off0, off1 = OFFSETS[g2]
        size = max(n, total - n) * REC + 48
    expected = np.full(size, GUARD, dtype=np.uint8)
    for j in range(total):
        at = (j if j < n else j - n) * stride + (off0 if j < n else off1)
        expected[at:at + pt] = expect_pts[j]
    out = np.full(size, GUARD, dtype=np.uint8)
    work = np.ascontiguousarray(work)
    st = hooks.L.arith_to_affine(g2, work.ctypes.data, total, n, off0, off1, stride, out.ctypes.data, size)
    assert st == 0, f"arith_to_affine returned {st}"
    bad = np.flatnonzero(out != expected)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]} of {size}"
