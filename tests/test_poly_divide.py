"""g16_poly_divide_linear: p(X) = q(X) (X - z) + y against Python's synthetic division, byte for byte (field elements
have one canonical value), on the emulator and on the GPU.  The sizes follow the kernel's own constants: its run
length (coefficients per lane), run x block (coefficients per block) and two blocks, one below, at and one above."""
import os
import random
import re

import numpy as np
import pytest

import circom_compat_amd as cc

R = cc.FR_MODULUS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "g16_amd.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))


RUN = _header_constant("G16_POLY_RUN")        # coefficients per lane
BLOCK = _header_constant("G16_POLY_BLOCK")    # lanes per block
TILE = RUN * BLOCK                            # coefficients per block
SIZES = sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, 1025,
                RUN - 1, RUN, RUN + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1} - {0})


def synthetic_division(coeffs, z):
    s, out = 0, []
    for a in reversed(coeffs):
        s = (a + z * s) % R
        out.append(s)
    out.reverse()
    return out[1:], out[0]


def evaluate(coeffs, t):
    s = 0
    for a in reversed(coeffs):
        s = (a + t * s) % R
    return s


def test_python_binding_matches_the_header():
    assert (cc.POLY_RUN, cc.POLY_BLOCK) == (RUN, BLOCK)


@pytest.mark.parametrize("n", SIZES)
def test_quotient_and_remainder(lib, n):
    """z in {0, 1, r - 1, random, a root of p}: five polynomials in one call, each with its own point"""
    rng = random.Random(1000 + n)
    p = [rng.randrange(R) for _ in range(n)]
    if n > 1:
        p[-1] = rng.randrange(1, R)
    z_root = rng.randrange(R)
    with_root = list(p)
    with_root[0] = (p[0] - evaluate(p, z_root)) % R
    zs = [0, 1, R - 1, rng.randrange(R), z_root]
    polys = [p, p, p, p, with_root]
    got = cc.poly_divide_linear(polys, zs, lib=lib)
    assert len(got) == 5
    for (q, y), poly, z in zip(got, polys, zs):
        assert (q, y) == synthetic_division(poly, z), (n, z)
        assert len(q) == n - 1
    assert got[4][1] == 0                      # at the root the remainder is 0
    assert got[0][1] == p[0] and got[0][0] == p[1:]   # z = 0: the quotient is the polynomial shifted down


def test_three_polynomials_three_points(lib):
    rng = random.Random(7)
    n = TILE + 37
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [rng.randrange(R) for _ in range(3)]
    batch = cc.poly_divide_linear(polys, zs, lib=lib)
    for k in range(3):
        assert batch[k] == synthetic_division(polys[k], zs[k])
        assert batch[k] == cc.poly_divide_linear(polys[k], zs[k], lib=lib)   # a single call gives the same


def test_montgomery_and_canonical_inputs_agree(lib):
    rng = random.Random(8)
    p = [rng.randrange(R) for _ in range(RUN * 3 + 1)]
    z = rng.randrange(R)
    mont = cc.fr_from_ints(p, lib)
    assert cc.poly_divide_linear(mont, cc.fr_from_ints([z], lib), lib=lib) == cc.poly_divide_linear(p, z, lib=lib)


def test_refusals(lib):
    with pytest.raises(cc.G16Error) as e:
        cc.poly_divide_linear([1, R, 3], 5, lib=lib)          # a canonical coefficient equal to r
    assert e.value.status == 1 and "coefficient 1 " in str(e.value)
    with pytest.raises(cc.G16Error) as e:
        cc.poly_divide_linear([1, 2, 3], R, lib=lib)          # the point equal to r
    assert e.value.status == 1 and "point 0 " in str(e.value)
    z = np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros((1, 4), dtype=np.uint64)
    assert lib.g16_poly_divide_linear(0, None, 4, 1, z.ctypes.data, 0, out.ctypes.data, out.ctypes.data) == 1
    assert lib.g16_poly_divide_linear(0, z.ctypes.data, 0, 1, z.ctypes.data, 0, out.ctypes.data, out.ctypes.data) == 1
    assert lib.g16_poly_divide_linear(0, z.ctypes.data, (1 << 27) + 1, 1, z.ctypes.data, 0, out.ctypes.data,
                                      out.ctypes.data) == 1


@pytest.mark.gpu
def test_large_division_identity(gpulib):
    """n = 2^20: p(t) = q(t) (t - z) + y at a random t, in Python integers"""
    n = 1 << 20
    rs = np.random.RandomState(20)
    raw = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x1f                                          # below 2^253 < r
    rng = random.Random(21)
    z, t = rng.randrange(R), rng.randrange(R)
    q, y = cc.poly_divide_linear(raw, z, lib=gpulib)
    b = raw.tobytes()
    p = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    assert len(q) == n - 1
    assert y == evaluate(p, z)
    assert evaluate(p, t) == (evaluate(q, t) * (t - z) + y) % R
