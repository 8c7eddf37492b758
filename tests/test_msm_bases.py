"""The MSM engine over caller-supplied bases (g16_msm_bases_create / g16_msm / g16_msm_once) against the oracle's
Curve.msm and closed forms.  A group element has one affine encoding: every comparison is byte equality."""
import os
import random

import numpy as np
import pytest

import bn254_ref as o
import circom_compat_amd as cc

R = o.R_MOD


def _bases(curve, gen, n, seed):
    """n points with the awkward ones first: infinity, a point, its negation (equal x), the point again, then
    distinct multiples of the generator"""
    rng = random.Random(seed)
    P = curve.mul(gen, rng.randrange(1, R))
    pts = [None, P, curve.neg(P), P]
    Q = curve.mul(gen, rng.randrange(1, R))
    while len(pts) < n:
        pts.append(Q)
        Q = curve.add(Q, gen)
    return pts[:n]


def _scalars(n, seed):
    rng = random.Random(seed)
    s = [0, 1, R - 1, rng.randrange(1 << 253, R), 5, 5, R - 5, 2]
    s += [rng.randrange(R) for _ in range(max(0, n - len(s)))]
    rng.shuffle(s)
    return s[:n]


_G1 = {}
_G2 = {}


def g1_case(n):
    if n not in _G1:
        pts = _bases(o.G1, o.G1_GEN, n, 11)
        s = _scalars(n, 12 + n)
        _G1[n] = (pts, b"".join(o.g1_to_bytes(p) for p in pts), s, o.g1_to_bytes(o.G1.msm(pts, s)))
    return _G1[n]


def g2_case(n):
    if n not in _G2:
        pts = _bases(o.G2, o.G2_GEN, n, 21)
        s = _scalars(n, 22 + n)
        _G2[n] = (pts, b"".join(o.g2_to_bytes(p) for p in pts), s, o.g2_to_bytes(o.G2.msm(pts, s)))
    return _G2[n]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300])
def test_g1_against_the_oracle(lib, n):
    pts, raw, s, want = g1_case(n)
    h = cc.MsmBases(raw, "g1", lib=lib)
    assert h.info()["n"] == n
    got = h.msm(s)                                        # canonical scalars
    assert got == want
    if n:
        assert h.msm(cc.fr_from_ints(s, lib)) == want     # Montgomery scalars: the same bytes
    assert cc.msm(raw, s, "g1", lib=lib) == want          # the one-shot call
    h.close()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64])
def test_g2_against_the_oracle(lib, n):
    pts, raw, s, want = g2_case(n)
    h = cc.MsmBases(raw, "g2", lib=lib)
    assert h.msm(s) == want
    if n:
        assert h.msm(cc.fr_from_ints(s, lib)) == want
    assert cc.msm(raw, s, "g2", lib=lib) == want
    h.close()


def test_fewer_scalars_than_bases(lib):
    pts, raw, s, _ = g1_case(65)
    h = cc.MsmBases(raw, "g1", lib=lib)
    for ln in (0, 1, 40):
        assert h.msm(s[:ln]) == o.g1_to_bytes(o.G1.msm(pts[:ln], s[:ln])), ln
    with pytest.raises(cc.G16Error) as e:
        h.msm(s + [1])
    assert e.value.status == 1
    pts2, raw2, s2, _ = g2_case(64)
    h2 = cc.MsmBases(raw2, "g2", lib=lib)
    assert h2.msm(s2[:17]) == o.g2_to_bytes(o.G2.msm(pts2[:17], s2[:17]))


def _is_emu(lib):
    return "emu" in os.path.basename(lib.path)


def _fix_cap(lib):
    """MSM_FIX_CAP of the build under test: 512 on the emulator, 2048 on the GPU"""
    return 512 if _is_emu(lib) else 2048


def test_equal_bases_take_the_exact_kernel(lib):
    """every base the same point, scalars 1..n, n above the fix-up list: the optimistic accumulation sets every
    addition aside, the list overflows and the exact kernel redoes the launch.  A key never looks like this; a
    caller's bases easily do."""
    n = 513 if _is_emu(lib) else 4096
    assert n > _fix_cap(lib)
    raw = o.g1_to_bytes(o.G1_GEN) * n
    h = cc.MsmBases(raw, "g1", max_batch=3, lib=lib)
    up = list(range(1, n + 1))
    want = o.g1_to_bytes(o.G1.mul(o.G1_GEN, n * (n + 1) // 2))
    assert h.msm(up) == want
    batch = h.msm([up, [1] * n, up[::-1]])
    assert batch == [want, o.g1_to_bytes(o.G1.mul(o.G1_GEN, n)), want]


def test_planes_and_one_shot_give_the_same_bytes(lib):
    pts, raw, s, want = g1_case(65)
    seen = {}
    for planes in (1, 2, None):
        h = cc.MsmBases(raw, "g1", planes=planes, lib=lib)
        info = h.info()
        seen[planes] = info["planes"]
        assert info["planes"] * info["bucket_sets"] >= info["windows"]
        assert h.msm(s) == want, planes
        h.close()
    assert seen[1] == 1 and seen[2] == 2 and seen[None] > 2
    assert cc.msm(raw, s, "g1", lib=lib) == want
    pts2, raw2, s2, want2 = g2_case(2)
    for planes in (1, 2, None):
        assert cc.MsmBases(raw2, "g2", planes=planes, lib=lib).msm(s2) == want2


def test_chunks_and_stride(lib):
    """count in {1, B, B + 1, 2 B + 1} vectors at a stride above len: every vector gets what a single call gives"""
    n, ln, stride, B = 20, 17, 23, 2
    pts, raw, _, _ = g1_case(63)
    raw = raw[:64 * n]
    h = cc.MsmBases(raw, "g1", max_batch=B, lib=lib)
    assert h.info()["batch"] == B
    rng = random.Random(5)
    for count in (1, B, B + 1, 2 * B + 1):
        vecs = [[rng.randrange(R) for _ in range(ln)] for _ in range(count)]
        buf = np.zeros((count, stride, 4), dtype=np.uint64)
        for k, v in enumerate(vecs):
            buf[k, :ln] = cc.fr_from_ints(v, lib)
            buf[k, ln:] = 0xFFFFFFFFFFFFFFFF               # what lies between the vectors is never read as a scalar
        out = np.zeros((count, 64), dtype=np.uint8)
        lib.check(lib.g16_msm(h._h.ptr, buf.ctypes.data, ln, count, stride, 0, out.ctypes.data))
        for k, v in enumerate(vecs):
            single = h.msm(v)
            assert out[k].tobytes() == single, (count, k)
            assert single == o.g1_to_bytes(o.G1.msm(pts[:ln], v))
        assert h.msm(vecs) == [out[k].tobytes() for k in range(count)]


def _twist_point_outside_g2(seed):
    """a point of E'(Fq2) outside the r-torsion (the twist's cofactor is 2q - r: a random point is)"""
    q = o.Q_MOD
    rng = random.Random(seed)

    def fq_sqrt(a):
        s = pow(a, (q + 1) // 4, q)
        return s if s * s % q == a % q else None

    while True:
        x = (rng.randrange(q), rng.randrange(q))
        rhs = o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.G2_B)
        a0, a1 = rhs
        nrm = fq_sqrt((a0 * a0 + a1 * a1) % q)
        if nrm is None:
            continue
        for sgn in (nrm, q - nrm):
            y0 = fq_sqrt((a0 + sgn) * pow(2, q - 2, q) % q)
            if not y0:
                continue
            y = (y0, a1 * pow(2 * y0, q - 2, q) % q)
            if o.f2_sqr(y) == (rhs[0] % q, rhs[1] % q):
                P = (x, y)
                assert o.G2.on_curve(P) and o.G2.mul(P, R) is not None
                return P


def test_refusals(lib):
    pts, raw, s, want = g1_case(63)
    h = cc.MsmBases(raw, "g1", validate=True, lib=lib)     # a well-formed set passes the predicates
    assert h.info()["validated"] == 1 and h.msm(s) == want
    bad = list(s)
    bad[41] = R                                            # a canonical scalar equal to r
    with pytest.raises(cc.G16Error) as e:
        h.msm(bad)
    assert e.value.status == 1 and "scalar 41 " in str(e.value)
    with pytest.raises(cc.G16Error) as e:
        h.msm([s, bad])                                    # ... and inside a batch: vector 1, element 41
    assert e.value.status == 1 and "vector 1, element 41" in str(e.value)
    # a point off the curve
    off = bytearray(raw)
    off[64 * 7 + 32] ^= 1
    with pytest.raises(cc.G16Error) as e:
        cc.MsmBases(bytes(off), "g1", validate=True, lib=lib)
    assert e.value.status == 1 and "point 7:" in str(e.value) and "curve" in str(e.value)
    assert cc.MsmBases(bytes(off), "g1", lib=lib).info()["validated"] == 0   # without validate: taken as it comes
    # a non-canonical coordinate
    nc = bytearray(raw)
    nc[64 * 3:64 * 3 + 32] = b"\xff" * 32
    with pytest.raises(cc.G16Error) as e:
        cc.MsmBases(bytes(nc), "g1", validate=True, lib=lib)
    assert "point 3:" in str(e.value) and "canonical" in str(e.value)
    # a G2 point on the twist outside the subgroup
    pts2, raw2, _, _ = g2_case(2)
    out = raw2 + o.g2_to_bytes(_twist_point_outside_g2(3))
    with pytest.raises(cc.G16Error) as e:
        cc.MsmBases(out, "g2", validate=True, lib=lib)
    assert e.value.status == 1 and "point 2:" in str(e.value) and "subgroup" in str(e.value)
    assert cc.MsmBases(raw2, "g2", validate=True, lib=lib).info()["validated"] == 1
    # NULL pointers; n above 2^27 is refused before anything is dereferenced
    hp, one = cc.C.c_void_p(), np.zeros(64, dtype=np.uint8)
    assert lib.g16_msm_bases_create(0, 0, None, 4, 0, None, cc.C.byref(hp)) == 1
    assert lib.g16_msm_bases_create(0, 0, one.ctypes.data, 1, 0, None, None) == 1
    assert lib.g16_msm_bases_create(0, 2, one.ctypes.data, 1, 0, None, cc.C.byref(hp)) == 1
    assert lib.g16_msm_bases_create(0, 0, 1, (1 << 27) + 1, 0, None, cc.C.byref(hp)) == 1
    assert lib.g16_msm_once(0, 0, 1, 1, (1 << 27) + 1, 0, one.ctypes.data) == 1
    assert lib.g16_msm_once(0, 0, None, None, 3, 0, one.ctypes.data) == 1
    assert lib.g16_msm(None, one.ctypes.data, 1, 1, 1, 0, one.ctypes.data) == 1
    assert lib.g16_msm(h._h.ptr, None, 1, 1, 1, 0, one.ctypes.data) == 1
    assert lib.g16_msm(h._h.ptr, one.ctypes.data, 1, 1, 1, 0, None) == 1


@pytest.mark.gpu
def test_large_against_a_trapdoor_srs(gpulib):
    """n = 2^16 + 1 bases tau^i G of a trapdoor SRS: the MSM is p(tau) G, one oracle scalar multiplication"""
    n = (1 << 16) + 1
    tau = 0x1234567890abcdef1234567890abcdef % R
    srs = cc.trapdoor_srs(16, (tau, 3, 5), lib=gpulib)
    assert srs.tau_g1.shape[0] >= n
    rs = np.random.RandomState(16)
    raw = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x1f
    b = raw.tobytes()
    acc = 0
    for i in range(n - 1, -1, -1):
        acc = (acc * tau + int.from_bytes(b[32 * i:32 * i + 32], "little")) % R
    want = o.g1_to_bytes(o.G1.mul(o.G1_GEN, acc))
    h = cc.MsmBases(srs.tau_g1[:n], "g1", max_batch=2, lib=gpulib)
    assert h.msm(raw) == want
    assert h.msm(np.stack([raw, raw])) == [want, want]
    assert cc.msm(srs.tau_g1[:n], raw, "g1", lib=gpulib) == want


@pytest.mark.gpu
def test_same_result_as_the_resident_key_msm(gpulib):
    """the engine on the A query of a small generated key equals g16_msm_g1(ctx, G16_QUERY_A, ..) on the same scalars"""
    import helpers as H
    m, n_pub = 300, 2
    base = 1 + n_pub
    n_vars = base + m + 1
    cons = [([(base + i, 1)], [(base + i, 1)], [(base + i + 1, 1)]) for i in range(m)]
    rng = random.Random(3)
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *[rng.randrange(1, R) for _ in range(5)])
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, gpulib)
    pk = H.pk_from_oracle(opk)
    pr = cc.Prover(pk, mats, lib=gpulib)
    s = [rng.randrange(R) for _ in range(n_vars - 1)]
    want = pr.msm_g1(cc.B.QUERY_A, s)
    a = np.ascontiguousarray(pk.a_query, dtype=np.uint8).reshape(-1, 64)
    assert cc.MsmBases(a[1:], "g1", lib=gpulib).msm(s) == bytes(want)
    assert cc.msm(a[1:], s, "g1", lib=gpulib) == bytes(want)
