"""KZG commit / open / verify on a powers-of-tau string.  With a trapdoor string tau is known, so a commitment is
p(tau) G and a proof q(tau) G: one oracle scalar multiplication each, compared byte for byte."""
import random

import numpy as np
import pytest

import bn254_ref as o
import circom_compat_amd as cc

R = o.R_MOD
TAU = 0x2b5a9d1c3e7f00112233445566778899aabbccddeeff0123456789abcdef % R


def _eval(p, t):
    s = 0
    for a in reversed(p):
        s = (a + t * s) % R
    return s


def _quotient(p, z):
    s, out = 0, []
    for a in reversed(p):
        s = (a + z * s) % R
        out.append(s)
    out.reverse()
    return out[1:], out[0]


def _g(k):
    return o.g1_to_bytes(o.G1.mul(o.G1_GEN, k % R))


_SRS = {}


def _srs(lib):
    if lib.path not in _SRS:
        _SRS[lib.path] = cc.trapdoor_srs(5, (TAU, 3, 5), lib=lib)     # 63 powers in G1
    return _SRS[lib.path]


def test_commit_open_verify(lib):
    srs = _srs(lib)
    L = 40
    key = cc.KzgKey(srs, max_len=L, lib=lib)
    assert key.info()["n"] == L and key.tau_g2 == srs.tau_g2[1].tobytes()
    rng = random.Random(1)
    p = [rng.randrange(R) for _ in range(L)]
    z = rng.randrange(R)
    c = key.commit(p)
    assert c == _g(_eval(p, TAU))
    y, pi = key.open(p, z)
    q, rem = _quotient(p, z)
    assert y == rem == _eval(p, z)
    assert pi == _g(_eval(q, TAU))
    assert key.verify(c, z, y, pi) is True
    assert key.verify(c, z, (y + 1) % R, pi) is False
    assert key.open(cc.fr_from_ints(p, lib), z) == (y, pi)          # Montgomery coefficients: the same bytes
    # a key of max_len L refuses L + 1 coefficients
    for call in (lambda: key.commit(p + [1]), lambda: key.open(p + [1], z)):
        with pytest.raises(cc.G16Error) as e:
            call()
        assert e.value.status == 1
    with pytest.raises(cc.G16Error):
        cc.KzgKey(srs, max_len=srs.tau_g1.shape[0] + 1, lib=lib)
    # one coefficient: the quotient is empty, the proof is the point at infinity
    assert key.open([7], z) == (7, bytes(64))
    assert key.verify(key.commit([7]), z, 7, bytes(64)) is True
    # a canonical coefficient equal to r is refused with its index
    with pytest.raises(cc.G16Error) as e:
        key.open([1, 2, R, 4], z)
    assert e.value.status == 1 and "coefficient 2 " in str(e.value)


def test_batch_of_64_and_its_forgeries(lib):
    srs = _srs(lib)
    key = cc.KzgKey(srs, max_len=8, max_batch=24, lib=lib)          # 64 = 24 + 24 + 16: three chunks
    rng = random.Random(2)
    n = 64
    polys = [[rng.randrange(R) for _ in range(6)] for _ in range(n)]
    zs = [rng.randrange(R) for _ in range(n)]
    cms = key.commit(polys)
    opened = key.open(polys, zs)
    ys, pis = [y for y, _ in opened], [pi for _, pi in opened]
    for k in (0, 23, 24, 63):
        q, rem = _quotient(polys[k], zs[k])
        assert cms[k] == _g(_eval(polys[k], TAU)) and ys[k] == rem and pis[k] == _g(_eval(q, TAU)), k
    rho = [rng.randrange(1, 1 << 128) for _ in range(n)]
    assert key.verify(cms, zs, ys, pis, rho=rho) is True
    assert key.verify(cms, zs, ys, pis, rho=rho) is True           # a given rho: the same verdict again
    assert key.verify(cms, zs, ys, pis) is True                     # rho drawn by the library
    assert cc.kzg_verify(srs.tau_g2[1].tobytes(), cms, zs, ys, pis, rho=rho, lib=lib) is True

    def tampered(what, k, value):
        parts = {"c": list(cms), "z": list(zs), "y": list(ys), "pi": list(pis)}
        parts[what][k] = value
        return key.verify(parts["c"], parts["z"], parts["y"], parts["pi"], rho=rho)

    assert tampered("y", 17, (ys[17] + 1) % R) is False             # one wrong value
    assert tampered("z", 40, (zs[40] + 1) % R) is False             # one wrong point
    assert tampered("pi", 5, _g(12345)) is False                    # a proof replaced by another valid point
    off = bytearray(cms[63])
    off[32] ^= 1
    assert tampered("c", 63, bytes(off)) is False                   # a commitment off the curve
    with pytest.raises(cc.G16Error) as e:
        key.verify(cms, zs, ys, pis, rho=[0] + rho[1:])             # a zero coefficient is refused
    assert e.value.status == 1
    # the wrong tau_g2 fails everything
    assert cc.kzg_verify(srs.tau_g2[2].tobytes(), cms, zs, ys, pis, rho=rho, lib=lib) is False


def test_empty_batch_is_true(lib):
    assert cc.kzg_verify(o.g2_to_bytes(o.G2_GEN), [], [], [], [], lib=lib) is True
    ok = cc.C.c_uint8(0)
    assert lib.g16_kzg_verify(0, None, None, None, None, None, 0, None, cc.C.byref(ok)) == 0 and ok.value == 1
    assert lib.g16_kzg_verify(0, None, None, None, None, None, 1, None, cc.C.byref(ok)) == 1
    assert lib.g16_kzg_verify(0, None, None, None, None, None, 0, None, None) == 1


@pytest.mark.gpu
def test_degree_2_16_on_a_string_nobody_knows_tau_of(gpulib):
    """open and verify against cc.contribute_srs(cc.new_srs(..)): the check is verify alone"""
    srs = cc.contribute_srs(cc.new_srs(16, lib=gpulib), lib=gpulib)
    n = (1 << 16) + 1
    assert srs.tau_g1.shape[0] >= n
    key = cc.KzgKey(srs, max_len=n, lib=gpulib)
    rs = np.random.RandomState(4)
    raw = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x1f
    raw[n - 1, 0] |= 1                                              # degree exactly 2^16
    z = random.Random(5).randrange(R)
    c = key.commit(raw)
    y, pi = key.open(raw, z)
    b = raw.tobytes()
    assert y == _eval([int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)], z)
    assert key.verify(c, z, y, pi) is True
    assert key.verify(c, z, (y + 1) % R, pi) is False
    assert key.verify(c, (z + 1) % R, y, pi) is False
