"""g16_points_from_ark / g16_points_to_ark against an encoder and a decoder written HERE, in Python, from the
description of ark-serialize's canonical form in include/g16_amd.h -- independent of the product -- and against
known arkworks encodings of single points (the pins)."""
import numpy as np
import pytest

import bn254_ref as o
import circom_compat_amd as cc
from circom_compat_amd import _binding as B

Q = o.Q_MOD
HALF = (Q - 1) // 2
INV2 = pow(2, Q - 2, Q)
NEG, INF = 0x80, 0x40
ENC, NONCANON, OFF, SUB = B.KEY_BAD_ENCODING, B.KEY_BAD_NONCANONICAL, B.KEY_BAD_OFF_CURVE, B.KEY_BAD_SUBGROUP
GROUPS = ("g1", "g2")
MODES = (True, False)                                       # compressed, uncompressed


# ---- the format, restated ------------------------------------------------------------------------------------------
def _coords(group, v):
    """a coordinate as a list of Fq integers"""
    return [v] if group == "g1" else list(v)


def _negative(group, y):
    if group == "g1":
        return y > HALF
    return y[1] > HALF or (y[1] == 0 and y[0] > HALF)


def py_encode(group, P, compressed):
    w = 1 if group == "g1" else 2
    if P is None:
        b = bytearray(32 * w * (1 if compressed else 2))
        b[-1] |= INF
        return bytes(b)
    x, y = P
    vals = _coords(group, x) + ([] if compressed else _coords(group, y))
    b = bytearray(b"".join(v.to_bytes(32, "little") for v in vals))
    if _negative(group, y):
        b[-1] |= NEG
    return bytes(b)


def _fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a else None


def _f2_sqrt(a):
    """the textbook complex method, with its inversion"""
    a0, a1 = a
    if a1 == 0:
        r = _fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        return (0, _fq_sqrt(Q - a0))
    s = _fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if s is None:
        return None
    t = (a0 + s) * INV2 % Q
    y0 = _fq_sqrt(t)
    if y0 is None:
        y0 = _fq_sqrt((a0 - s) * INV2 % Q)
    y = (y0, a1 * pow(2 * y0, Q - 2, Q) % Q)
    assert o.f2_sqr(y) == a
    return y


def _rhs(group, x):
    if group == "g1":
        return (x * x * x + 3) % Q
    return o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.G2_B)


def _neg(group, y):
    return (Q - y) % Q if group == "g1" else o.f2_neg(y)


def py_decode(group, rec, compressed, validate=True):
    """(point | None, reason): the first test that fails"""
    w = 1 if group == "g1" else 2
    assert len(rec) == 32 * w * (1 if compressed else 2)
    fl = rec[-1] & 0xC0
    body = bytearray(rec)
    body[-1] &= 0x3F
    vals = [int.from_bytes(body[i:i + 32], "little") for i in range(0, len(body), 32)]
    if fl == 0xC0:
        return None, ENC
    if fl & INF:
        return None, (ENC if any(vals) else 0)
    if any(v >= Q for v in vals):
        return None, NONCANON
    x = vals[0] if group == "g1" else tuple(vals[:2])
    rhs = _rhs(group, x)
    if compressed:
        y = _fq_sqrt(rhs) if group == "g1" else _f2_sqrt(rhs)
        if y is None:
            return None, OFF
        if _negative(group, y) != bool(fl & NEG):
            y = _neg(group, y)
    else:
        y = vals[1] if group == "g1" else tuple(vals[2:])
        if (y * y % Q if group == "g1" else o.f2_sqr(y)) != rhs:
            return None, OFF
    if group == "g2" and validate and o.G2.mul((x, y), o.R_MOD) is not None:
        return None, SUB
    return (x, y), 0


def packed(group, P):
    return o.g1_to_bytes(P) if group == "g1" else o.g2_to_bytes(P)


def packed_size(group):
    return 64 if group == "g1" else 128


# ---- shared points: multiples of the generators, computed once ---------------------------------------------------
_CACHE = {}


def multiples(group, n):
    """[G, 2G, ..., nG]"""
    got = _CACHE.setdefault(group, [])
    crv, gen = (o.G1, o.G1_GEN) if group == "g1" else (o.G2, o.G2_GEN)
    while len(got) < n:
        got.append(gen if not got else crv.add(got[-1], gen))
    return got[:n]


def with_infinities(group, n):
    """n points, every fifth (and the first of a longer list's second block) at infinity; negatives mixed in so that
    both values of the sign flag occur"""
    crv = o.G1 if group == "g1" else o.G2
    pts = []
    for i, P in enumerate(multiples(group, n)):
        if i % 5 == 2 or i == 64:
            pts.append(None)
        else:
            pts.append(crv.neg(P) if i % 3 == 1 else P)
    return pts


def decode(lib, group, blob, compressed, validate=True, **kw):
    return cc.points_from_ark(blob, group, compressed=compressed, validate=validate, lib=lib, **kw)


# ---- pins: known arkworks byte strings ---------------------------------------------------------------------------
G2_GEN_ARK = bytes.fromhex("edf692d95cbdde46ddda5ef7d422436779445c5e66006a42761e1f12efde0018"
                           "c212f3aeb785e49712e7a9353349aaf1255dfb31b7bf60723a480d9293938e19")


def _flag(b, bit):
    b = bytearray(b)
    b[-1] |= bit
    return bytes(b)


def test_pins(lib):
    g1, g2 = o.G1_GEN, o.G2_GEN
    x2 = b"".join(v.to_bytes(32, "little") for v in g2[0])
    y2 = b"".join(v.to_bytes(32, "little") for v in g2[1])
    assert x2 == G2_GEN_ARK and not _negative("g2", g2[1])             # the vector's x is the oracle's generator
    one, two = (1).to_bytes(32, "little"), (2).to_bytes(32, "little")
    ny1 = (Q - 2).to_bytes(32, "little")
    ny2 = b"".join(v.to_bytes(32, "little") for v in o.f2_neg(g2[1]))
    pins = [
        ("g1", True, g1, one),
        ("g1", True, o.G1.neg(g1), _flag(one, NEG)),
        ("g1", True, None, _flag(bytes(32), INF)),
        ("g2", True, None, _flag(bytes(64), INF)),
        ("g2", True, g2, G2_GEN_ARK),
        ("g2", True, o.G2.neg(g2), _flag(G2_GEN_ARK, NEG)),
        ("g1", False, g1, one + two),
        ("g1", False, o.G1.neg(g1), one + _flag(ny1, NEG)),
        ("g1", False, None, _flag(bytes(64), INF)),
        ("g2", False, None, _flag(bytes(128), INF)),
        ("g2", False, g2, G2_GEN_ARK + y2),
        ("g2", False, o.G2.neg(g2), G2_GEN_ARK + _flag(ny2, NEG)),
    ]
    assert one == bytes([1]) + bytes(31) and _flag(one, NEG)[31] == 0x80
    for group, comp, P, ark in pins:
        assert py_encode(group, P, comp) == ark                       # the restatement agrees with the pins
        pts, why, bad = decode(lib, group, ark, comp)
        assert bad == 0 and list(why) == [0], (group, comp, P)
        assert pts.tobytes() == packed(group, P), (group, comp, P)
        back = cc.points_to_ark(packed(group, P), group, compressed=comp, lib=lib)
        assert back.tobytes() == ark, (group, comp, P)


# ---- round trips -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9])
@pytest.mark.parametrize("compressed", MODES)
@pytest.mark.parametrize("group", GROUPS)
def test_round_trip(lib, group, compressed, n):
    pts = with_infinities(group, n)
    ark = b"".join(py_encode(group, P, compressed) for P in pts)
    want = b"".join(packed(group, P) for P in pts)
    got, why, bad = decode(lib, group, ark, compressed)
    assert bad == 0 and not why.any() and why.shape == (n,)
    assert got.tobytes() == want
    back = cc.points_to_ark(np.frombuffer(want, dtype=np.uint8), group, compressed=compressed, lib=lib)
    assert back.tobytes() == ark
    rec = len(ark) // n if n else 0
    for i, P in enumerate(pts):                                        # and the library's bytes through the test's decoder
        assert py_decode(group, back.tobytes()[i * rec:(i + 1) * rec], compressed, validate=False) == (P, 0)


@pytest.mark.parametrize("compressed", MODES)
@pytest.mark.parametrize("group", GROUPS)
def test_round_trip_chunked(lib, group, compressed, monkeypatch):
    monkeypatch.setenv("G16_ARKSER_CHUNK", "64")                      # 133 = two full chunks and a ragged third
    pts = with_infinities(group, 133)
    ark = b"".join(py_encode(group, P, compressed) for P in pts)
    want = b"".join(packed(group, P) for P in pts)
    got, why, bad = decode(lib, group, ark, compressed)
    assert bad == 0 and not why.any()
    assert got.tobytes() == want
    assert cc.points_to_ark(got, group, compressed=compressed, lib=lib).tobytes() == ark
    # a bad point in each chunk: counted, located, neighbours untouched
    rec = len(ark) // 133
    broken = bytearray(ark)
    for i in (5, 64 + 63, 132):
        broken[(i + 1) * rec - 1] |= 0xC0
    got2, why2, bad2 = decode(lib, group, bytes(broken), compressed)
    assert bad2 == 3 and [i for i in range(133) if why2[i]] == [5, 127, 132]
    w = packed_size(group)
    for i in range(133):
        assert got2[i].tobytes() == (bytes(w) if i in (5, 127, 132) else want[i * w:(i + 1) * w])


@pytest.mark.parametrize("compressed", MODES)
def test_proof_layout_strides(lib, compressed):
    """A | B | C records of 128 / 256 bytes <-> packed proofs of 256 bytes: three strided calls"""
    n = 5
    g1s, g2s = with_infinities("g1", 2 * n), with_infinities("g2", n)
    s1, s2 = (32, 64) if compressed else (64, 128)
    rec = 2 * s1 + s2
    ark = b"".join(py_encode("g1", g1s[2 * i], compressed) + py_encode("g2", g2s[i], compressed) +
                   py_encode("g1", g1s[2 * i + 1], compressed) for i in range(n))
    want = b"".join(packed("g1", g1s[2 * i]) + packed("g2", g2s[i]) + packed("g1", g1s[2 * i + 1]) for i in range(n))
    src = np.frombuffer(ark, dtype=np.uint8)
    out = np.full(n * 256, 0xAA, dtype=np.uint8)
    for group, off_in, off_out in (("g1", 0, 0), ("g2", s1, 64), ("g1", s1 + s2, 192)):
        _, why, bad = decode(lib, group, src[off_in:], compressed, n=n, in_stride=rec, out_stride=256, out=out[off_out:])
        assert bad == 0 and not why.any()
    assert out.tobytes() == want
    back = np.full(n * rec, 0x55, dtype=np.uint8)
    for group, off_in, off_out in (("g1", 0, 0), ("g2", 64, s1), ("g1", 192, s1 + s2)):
        cc.points_to_ark(out[off_in:], group, n=n, compressed=compressed, in_stride=256, out_stride=rec,
                         out=back[off_out:], lib=lib)
    assert back.tobytes() == ark
    # a strided call writes its own records only
    lone = np.full(n * 256, 0xAA, dtype=np.uint8)
    decode(lib, "g1", src, compressed, n=n, in_stride=rec, out_stride=256, out=lone)
    for i in range(n):
        assert lone[i * 256:i * 256 + 64].tobytes() == want[i * 256:i * 256 + 64]
        assert (lone[i * 256 + 64:(i + 1) * 256] == 0xAA).all()


# ---- rejections --------------------------------------------------------------------------------------------------
def _le(*vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _reject(lib, group, compressed, bad_rec, reason, validate=True):
    """the bad record at index 3 of 9: its exact reason, a zeroed output record, untouched neighbours"""
    pts = with_infinities(group, 9)
    recs = [py_encode(group, P, compressed) for P in pts]
    assert len(bad_rec) == len(recs[3])
    recs[3] = bad_rec
    got, why, bad = decode(lib, group, b"".join(recs), compressed, validate=validate)
    assert list(why) == [0, 0, 0, reason, 0, 0, 0, 0, 0], (group, compressed, reason, list(why))
    assert bad == 1
    w = packed_size(group)
    for i, P in enumerate(pts):
        assert got[i].tobytes() == (bytes(w) if i == 3 else packed(group, P)), i
    assert py_decode(group, bad_rec, compressed, validate)[1] == reason   # the restatement gives the same verdict


@pytest.mark.parametrize("compressed", MODES)
@pytest.mark.parametrize("group", GROUPS)
def test_reject_flags_and_range(lib, group, compressed):
    w = 1 if group == "g1" else 2
    P = multiples(group, 4)[3]
    good = py_encode(group, P, compressed)
    size = len(good)
    _reject(lib, group, compressed, _flag(good, 0xC0), ENC)                               # both flags
    stray = bytearray(_flag(bytes(size), INF))
    stray[0] = 1
    _reject(lib, group, compressed, bytes(stray), ENC)                                    # infinity + a stray bit
    stray = bytearray(_flag(bytes(size), INF))
    stray[-1] |= 0x01
    _reject(lib, group, compressed, bytes(stray), ENC)
    # x = q (in the last word of x: where the flags live in compressed form), with and without a flag
    tail = good[32 * w:]
    xq = _le(*([0] * (w - 1) + [Q]))
    _reject(lib, group, compressed, xq + tail, NONCANON)
    _reject(lib, group, compressed, _flag(xq + tail, NEG), NONCANON)
    if group == "g2":
        _reject(lib, group, compressed, _le(Q, 5) + tail, NONCANON)                       # x.c0 = q
    # first failure: x = q + 4 is non-canonical AND (as 4) off the curve
    _reject(lib, group, compressed, _le(*([0] * (w - 1) + [Q + 4])) + tail, NONCANON)
    if not compressed:
        head = good[:32 * w]
        _reject(lib, group, compressed, head + _le(*([0] * (w - 1) + [Q])), NONCANON)     # y >= q
        _reject(lib, group, compressed, head + _le(*([Q] + [1] * (w - 1))), NONCANON)
        y = _coords(group, P[1])
        y[0] = (y[0] + 1) % Q
        _reject(lib, group, compressed, head + _le(*y), OFF)                              # y + 1
        # an x beyond 254 bits in uncompressed form is just a value >= q
        _reject(lib, group, compressed, _flag(head, NEG) + good[32 * w:], NONCANON)


def test_reject_g1_no_root(lib):
    for x in (0, 4):
        assert pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == Q - 1                            # a non-residue
        _reject(lib, "g1", True, _le(x), OFF)
        _reject(lib, "g1", True, _flag(_le(x), NEG), OFF)
    _reject(lib, "g1", False, _le(0, 0), OFF)                                             # (0, 0) without the flag


def test_reject_g2_no_root(lib):
    x = next((k, 1) for k in range(1, 50) if _f2_sqrt(_rhs("g2", (k, 1))) is None)
    _reject(lib, "g2", True, _le(*x), OFF)


def _twist_points_outside_g2():
    """points of the twist with Im(x^3 + b') = 0, so that y^2 is REAL: y is real when it is a residue, purely
    imaginary otherwise.  x = (x0, x1) with 3 x0^2 x1 - x1^3 = -Im(b')."""
    b1 = o.G2_B[1]
    found = {}
    tries = 0
    for x1 in range(1, 200):
        tries += 1
        x0 = _fq_sqrt((x1 ** 3 - b1) * pow(3 * x1, Q - 2, Q) % Q)
        if x0 is None:
            continue
        x = (x0, x1)
        rhs = _rhs("g2", x)
        assert rhs[1] == 0
        y = _f2_sqrt(rhs)
        cls = "real" if y[1] == 0 else "imaginary"
        assert y[0] == 0 or y[1] == 0
        found.setdefault(cls, (x, y))
        if len(found) == 2:
            break
    return found, tries


def test_g2_outside_the_subgroup(lib):
    found, tries = _twist_points_outside_g2()
    assert set(found) == {"real", "imaginary"}, (found, tries)                            # neither branch is skipped
    for cls, P in found.items():
        assert o.G2.on_curve(P) and o.G2.mul(P, o.R_MOD) is not None, cls
        for compressed in MODES:
            for Pt in (P, o.G2.neg(P)):
                rec = py_encode("g2", Pt, compressed)
                _reject(lib, "g2", compressed, rec, SUB, validate=True)
                got, why, bad = decode(lib, "g2", rec, compressed, validate=False)        # accepted without VALIDATE
                assert bad == 0 and list(why) == [0]
                assert got.tobytes() == o.g2_to_bytes(Pt), (cls, compressed)


def test_n_bad_counts_every_bad_point(lib):
    pts = with_infinities("g1", 9)
    recs = [py_encode("g1", P, True) for P in pts]
    recs[0] = _le(0)                    # no root
    recs[3] = _le(Q)                    # non-canonical
    recs[8] = _flag(recs[8], 0xC0)      # both flags
    got, why, bad = decode(lib, "g1", b"".join(recs), True)
    assert bad == 3 and list(why) == [OFF, 0, 0, NONCANON, 0, 0, 0, 0, ENC]
    assert not got[0].any() and not got[3].any() and not got[8].any()
    _, _, bad_only = cc.points_from_ark(b"".join(recs), "g1", lib=lib)
    assert bad_only == 3


@pytest.mark.parametrize("group", GROUPS)
def test_encode_rejects_a_word_not_below_q(lib, group):
    pts = with_infinities(group, 9)
    raw = bytearray(b"".join(packed(group, P) for P in pts))
    w = packed_size(group)
    raw[3 * w + w - 32:3 * w + w] = Q.to_bytes(32, "little")                              # the last word of point 3
    with pytest.raises(cc.G16Error) as e:
        cc.points_to_ark(bytes(raw), group, lib=lib)
    assert e.value.status == B.G16_ERR_INVALID
    out = np.zeros(9 * cc.ark_point_bytes(group), dtype=np.uint8)
    n_bad = B.C.c_uint64()
    src = np.frombuffer(bytes(raw), dtype=np.uint8)
    st = lib.g16_points_to_ark(0, B.POINT_G1 if group == "g1" else B.POINT_G2, B.ARK_COMPRESSED, src.ctypes.data, 0, 9,
                               out.ctypes.data, 0, B.C.byref(n_bad))
    assert st == B.G16_ERR_INVALID and n_bad.value == 1
    rec = cc.ark_point_bytes(group)
    for i, P in enumerate(pts):
        assert out[i * rec:(i + 1) * rec].tobytes() == (bytes(rec) if i == 3 else py_encode(group, P, True))


def test_bad_arguments(lib):
    one = np.zeros(64, dtype=np.uint8)
    bad = B.C.c_uint64()
    assert lib.g16_points_from_ark(0, 2, 1, one.ctypes.data, 0, 1, one.ctypes.data, 0, None, B.C.byref(bad)) == B.G16_ERR_INVALID
    assert lib.g16_points_from_ark(0, 0, 4, one.ctypes.data, 0, 1, one.ctypes.data, 0, None, B.C.byref(bad)) == B.G16_ERR_INVALID
    assert lib.g16_points_from_ark(0, 0, 1, one.ctypes.data, 16, 1, one.ctypes.data, 0, None, B.C.byref(bad)) == B.G16_ERR_INVALID
    assert lib.g16_points_from_ark(0, 0, 1, None, 0, 0, None, 0, None, None) == B.G16_OK  # n == 0


def test_same_bytes_and_reasons_twice(lib, monkeypatch):
    monkeypatch.setenv("G16_ARKSER_CHUNK", "16")
    pts = with_infinities("g2", 40)
    recs = [py_encode("g2", P, True) for P in pts]
    recs[7] = _le(Q, 1)
    recs[33] = _flag(recs[33], 0xC0)
    blob = b"".join(recs)
    a = decode(lib, "g2", blob, True)
    b = decode(lib, "g2", blob, True)
    assert a[0].tobytes() == b[0].tobytes() and list(a[1]) == list(b[1]) and a[2] == b[2] == 2
    assert list(np.nonzero(a[1])[0]) == [7, 33]
