"""ec29.h -- the XYZZ group law over the lazy limbs -- operation by operation against the oracle's G1 / G2.

Accumulators are built in Python for known points, (X z^2, Y z^3, z^2, z^3) in the internal form, and then moved
about INSIDE the classes the header of ec29.h documents (x across (-8p, 8p) with limbs 0..7 down to -8 and up to
2^29 + 7, y across (-3p, 3p), zz / zzz across (-p, 2p)).  The raw limbs that come back are mapped to affine points
and compared with bn254_ref, and checked against the same classes, so that the classes are shown to be invariants.
The P = +-Q branch, which whole proofs reach about 2^-23 of the time, is entered on purpose: with the exact product
model of lazy_model the stored x is set to U2 - j p, so that Pp = U2 - x is exactly j p, for every admissible j.

The limbs of y cannot be driven to -8 / 2^29 + 7 the way those of x are: once x is chosen, z and with it the
residue of y are fixed (and q = 1 mod 9 leaves no cheap cube root to start from y instead); y moves by multiples
of p only."""
import random

import pytest

import bn254_ref as o
import lazy_model as M
from lazy_model import LIMB, RP, norm, value

P = o.Q_MOD
RPI = pow(RP, -1, P)


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks(request):
    return M.load_hooks(request)


# ---- Fq / Fq2 elements as tuples of components --------------------------------------------------------------------
def fmul(a, b):
    return ((a[0] * b[0]) % P,) if len(a) == 1 else o.f2_mul(a, b)


def finv(a):
    return (pow(a[0], -1, P),) if len(a) == 1 else o.f2_inv(a)


def fsub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def fq_sqrt(a):
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def fsqrt(a):
    if len(a) == 1:
        r = fq_sqrt(a[0])
        return None if r is None else (r,)
    a0, a1 = a
    if a1 == 0:
        r = fq_sqrt(a0)
        return (r, 0) if r is not None else (0, fq_sqrt(-a0 % P))
    n = fq_sqrt((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None
    for half in ((a0 + n) * pow(2, -1, P) % P, (a0 - n) * pow(2, -1, P) % P):
        y0 = fq_sqrt(half)
        if y0:
            r = (y0, a1 * pow(2 * y0, -1, P) % P)
            if o.f2_mul(r, r) == (a0 % P, a1 % P):
                return r
    return None


class Curve:
    def __init__(self, g2):
        self.g2, self.k, self.W = g2, 2 if g2 else 1, 18 if g2 else 9
        self.C = o.G2 if g2 else o.G1
        rng = random.Random(290 + g2)
        gen = o.G2_GEN if g2 else o.G1_GEN
        self.pts = [self.C.mul(gen, rng.randrange(1, 1 << 64)) for _ in range(40)]

    def elt(self, c):                       # oracle coordinate -> tuple
        return tuple(c) if self.g2 else (c,)

    def coord(self, t):                     # tuple -> oracle coordinate
        return tuple(t) if self.g2 else t[0]

    def rand_elt(self, rng):
        return tuple(rng.randrange(1, P) for _ in range(self.k))

    # lazy elements are lists of k * 9 limbs
    def vals(self, l):
        return tuple(value(l[9 * i:9 * i + 9]) for i in range(self.k))

    def limbs(self, vals):
        return [x for v in vals for x in norm(v)]

    def internal(self, t):                  # canonical internal values of a field element
        return tuple(c * RP % P for c in t)

    def true(self, l):                      # the field element a lazy register stands for
        return tuple(v * RPI % P for v in self.vals(l))

    def lmul(self, a, b):
        """the exact values of the lazy product a * b"""
        va, vb = self.vals(a), self.vals(b)
        if not self.g2:
            return (M.mont_exact(va[0] * vb[0], P),)
        return (M.mont_exact(va[0] * vb[0] - va[1] * vb[1], P), M.mont_exact(va[0] * vb[1] + va[1] * vb[0], P))

    def affine(self, pt):
        """Aff29 as loaded: canonical internal limbs"""
        if pt is None:
            return dict(p=[[0] * self.W, [0] * self.W], inf=1)
        return dict(p=[self.limbs(self.internal(self.elt(pt[0]))), self.limbs(self.internal(self.elt(pt[1])))], inf=0)

    def acc(self, pt, z, kx=None, ky=None, kzz=None, kzzz=None):
        """(X z^2, Y z^3, z^2, z^3) with component values shifted by the given multiples of p"""
        if pt is None:
            return [[0] * self.W] * 4
        zz = fmul(z, z)
        zzz = fmul(zz, z)
        els = (fmul(self.elt(pt[0]), zz), fmul(self.elt(pt[1]), zzz), zz, zzz)
        out = []
        for e, ks in zip(els, (kx, ky, kzz, kzzz)):
            ks = ks or (0,) * self.k
            out.append(self.limbs(tuple(v + k * P for v, k in zip(self.internal(e), ks))))
        return out

    def point(self, a):
        """raw XYZZ29 limbs -> the oracle's affine point; infinity is exactly the all-zero zz"""
        x, y, zz, zzz = a
        if not any(zz):
            return None
        tzz, tzzz = self.true(zz), self.true(zzz)
        assert any(tzz), "zz = 0 mod p with non-zero limbs"
        assert fmul(fmul(tzz, tzz), tzz) == fmul(tzzz, tzzz)
        return (self.coord(fmul(self.true(x), finv(tzz))), self.coord(fmul(self.true(y), finv(tzzz))))

    def split(self, row):
        W = self.W
        return [list(map(int, row[i * W:(i + 1) * W])) for i in range(len(row) // W)]

    def in_classes(self, a):
        """the header of ec29.h, per component"""
        x, y, zz, zzz = a
        ok = True
        for i in range(self.k):
            s = slice(9 * i, 9 * i + 9)
            ok &= M.in_class(x[s], P, -8, 8, 8) and M.in_class(y[s], P, -3, 3, 8)
            ok &= M.is_m_class(zz[s], P) and M.is_m_class(zzz[s], P)
        return bool(ok)

    def check(self, row, want, what):
        a = self.split(row)[:4]
        assert self.point(a) == want, what
        if want is None:
            return a
        assert self.in_classes(a), (what, a)
        return a

    def extreme_x_acc(self, pt, rng, ky=None):
        """an accumulator for pt whose x limbs 0..7 sit at the ends of [-8, 2^29 + 8): x is chosen first, z = the
        square root of x / X follows (retried until there is one)"""
        X = self.elt(pt[0])
        for _ in range(200):
            xl = []
            for _c in range(self.k):
                low = [rng.choice((-8, -1, LIMB, LIMB + 7, -8, LIMB + 7, rng.randrange(LIMB))) for _ in range(8)]
                t = rng.choice((-8, -5, 0, 4, 7)) * P + rng.randrange(P)
                l = low + [(t - value(low)) >> 232]
                if not -8 * P < value(l) < 8 * P:
                    l[8] += 1 if value(l) < 0 else -1
                xl += l
            z = fsqrt(fmul(self.true(xl), finv(X)))
            if z is None or not any(z):
                continue
            a = self.acc(pt, z, ky=ky)
            assert self.true(a[0]) == self.true(xl)
            a[0] = xl
            assert self.in_classes(a) and self.point(a) == pt
            return a
        raise AssertionError("no square root found")

    def varied_acc(self, pt, rng, i):
        """class-extreme shifts in turn, every fourth one with extreme x limbs"""
        k = self.k
        ky = tuple(rng.choice((-3, 2, -1, 0)) for _ in range(k))
        if i % 4 == 3:
            return self.extreme_x_acc(pt, rng, ky)
        kx = tuple((-8, 7, rng.randint(-8, 7))[(i + c) % 3] for c in range(k))
        return self.acc(pt, self.rand_elt(rng), kx, ky, tuple(rng.choice((-1, 0, 1)) for _ in range(k)),
                        tuple(rng.choice((-1, 0, 1)) for _ in range(k)))


_curves = {}


@pytest.fixture(scope="module", params=[0, 1], ids=["g1", "g2"])
def cv(request):
    if request.param not in _curves:
        _curves[request.param] = Curve(request.param)
    return _curves[request.param]


def test_built_accumulators_are_in_their_classes(cv):
    rng = random.Random(2920)
    seen_neg, seen_hi = False, False
    for i in range(24):
        a = cv.varied_acc(cv.pts[i], rng, i)
        assert cv.in_classes(a) and cv.point(a) == cv.pts[i]
        seen_neg |= min(a[0][:8]) == -8
        seen_hi |= max(a[0][:8]) == LIMB + 7
        assert cv.point(cv.acc(None, None)) is None
    assert seen_neg and seen_hi


# ---- madd / madd_select -------------------------------------------------------------------------------------------
def test_madd_generic_and_infinities(hooks, cv):
    rng = random.Random(2921)
    cases, want = [], []
    for i in range(64):
        q, p = cv.pts[i % 40], cv.pts[(i * 7 + 1) % 40]
        assert q != p and q != cv.C.neg(p)
        cases.append(dict(acc=cv.varied_acc(q, rng, i), **cv.affine(p)))
        want.append(cv.C.add(q, p))
    fin = cv.varied_acc(cv.pts[3], rng, 1)
    for a, p, w in ((cv.acc(None, None), cv.pts[5], cv.pts[5]), (fin, None, cv.pts[3]), (cv.acc(None, None), None, None),
                    (cv.varied_acc(cv.pts[4], rng, 3), None, cv.pts[4])):
        cases.append(dict(acc=a, **cv.affine(p)))
        want.append(w)
    assert len(cases) % 64 != 0
    got, _ = hooks.ec(cv.g2, M.E_MADD, cases)
    sel, special = hooks.ec(cv.g2, M.E_MADD_SELECT, cases)
    for i, w in enumerate(want):
        cv.check(got[i], w, ("madd", i))
        assert special[i] == 0, i
        cv.check(sel[i], w, ("madd_select", i))
    # an affine point at infinity leaves the accumulator's limbs as they are; a point into an empty one has zz = 1
    assert cv.split(got[65])[:4] == fin and cv.split(sel[65])[:4] == fin
    one = cv.limbs(cv.internal((1,) + (0,) * (cv.k - 1)))
    assert cv.split(got[64])[2] == one and cv.split(sel[64])[3] == one


def _special_cases(cv, rng):
    """P = +-Q with Pp = U2 - x = j p exactly: j over [-8, 9] in every component (the far ends need a U2 outside
    [0, p), searched for), R = i p over [-2, 3] for the doublings"""
    k = cv.k
    cases, want, js, is_ = [], [], [set() for _ in range(k)], [set() for _ in range(k)]
    n = 0
    for comp in range(k):
        for j in range(-8, 10):
            for same in (True, False):
                iv = [(n // 2 + c) % 6 - 2 for c in range(k)]
                for _try in range(4000):
                    q = cv.pts[(n + _try) % 40]
                    kzz = tuple(rng.choice((-1, 0, 1)) if abs(j) < 8 else (1 if j > 0 else -1) for _ in range(k))
                    a = cv.acc(q, cv.rand_elt(rng), None, None, kzz, tuple(rng.choice((-1, 0, 1)) for _ in range(k)))
                    aff = cv.affine(q if same else cv.C.neg(q))
                    u2, s2 = cv.lmul(aff["p"][0], a[2]), cv.lmul(aff["p"][1], a[3])
                    jv = [rng.randint(-7, 8) for _ in range(k)]
                    jv[comp] = j
                    xv = [u - jj * P for u, jj in zip(u2, jv)]
                    yv = [s - ii * P for s, ii in zip(s2, iv)]
                    if all(abs(v) < 8 * P for v in xv) and (not same or all(abs(v) < 3 * P for v in yv)):
                        break
                else:
                    raise AssertionError(f"no accumulator found for j = {j}")
                n += 1
                a[0] = cv.limbs(xv)
                if same:                                   # R = S2 - y = i p as well
                    a[1] = cv.limbs(yv)
                    for c in range(k):
                        is_[c].add(iv[c])
                assert cv.in_classes(a) and cv.point(a) == q
                # what the kernel will see, limb by limb
                pp = [x - y for x, y in zip(cv.limbs(u2), a[0])]
                assert cv.vals(pp) == tuple(jj * P for jj in jv)
                for c in range(k):
                    js[c].add(jv[c])
                cases.append(dict(acc=a, **aff))
                want.append(cv.C.add(q, q) if same else None)
    return cases, want, js, is_


def test_madd_takes_the_special_branch_for_every_multiple_of_p(hooks, cv):
    cases, want, js, is_ = _special_cases(cv, random.Random(2922))
    for c in range(cv.k):
        assert js[c] == set(range(-8, 10)) and is_[c] == set(range(-2, 4))      # the coverage this test claims
    assert len(cases) % 64 != 0
    got, _ = hooks.ec(cv.g2, M.E_MADD, cases)
    _, special = hooks.ec(cv.g2, M.E_MADD_SELECT, cases)
    for i, w in enumerate(want):
        cv.check(got[i], w, ("madd special", i))
        assert special[i] == 1, ("madd_select misses P = +-Q", i)
    # madd_rare itself: Pp and R as the kernel forms them
    rare = []
    for c in cases:
        a, aff = c["acc"], c["p"]
        u2, s2 = cv.limbs(cv.lmul(aff[0], a[2])), cv.limbs(cv.lmul(aff[1], a[3]))
        rare.append(dict(acc=[[x - y for x, y in zip(u2, a[0])], [x - y for x, y in zip(s2, a[1])]], p=aff, inf=0))
    rare.append(dict(acc=[cv.limbs((1,) * cv.k), cv.limbs((0,) * cv.k)], p=cases[0]["p"], inf=0))     # Pp = 1: not handled
    res, handled = hooks.ec(cv.g2, M.E_MADD_RARE, rare)
    for i, w in enumerate(want):
        assert handled[i] == 1, i
        cv.check(res[i], w, ("madd_rare", i))
    assert handled[len(want)] == 0


def _near_misses(cv, rng):
    """P != +-Q, yet Pp = j p + 2^29 t passes the cheap filter (its low limb is that of j p, |j| <= 40; j = +-41 is
    the first that does not), or Pp = +-1; z is solved for: zz = Pp / (X_p - X_q)"""
    k = cv.k
    cases, want, passes = [], [], []
    pats = [("filter", j) for j in (-40, -9, -1, 0, 1, 2, 17, 40)] + [("outside", 41), ("outside", -41), ("one", 1), ("one", -1)]
    for n, (kind, j) in enumerate(pats):
        for _try in range(200):
            q, p = cv.pts[(n + _try) % 40], cv.pts[(n + 3 * _try + 11) % 40]
            if q == p or q == cv.C.neg(p):
                continue
            if kind != "one":        # the low limb of j p under a small value: the filter sees j, |j| <= 40 passes
                ppv = tuple(j * P - (j * P >> 29 << 29) + (rng.randrange(1, 1 << 190) << 29) * rng.choice((-1, 1))
                            for _ in range(k))
            else:
                ppv = tuple(j if c == 0 else rng.choice((1, -1)) for c in range(k))
            assert all(v % P for v in ppv)
            d = fsub(cv.elt(p[0]), cv.elt(q[0]))
            z = fsqrt(fmul(tuple(v * RPI % P for v in ppv), finv(d)))
            if z is None:
                continue
            a = cv.acc(q, z)
            aff = cv.affine(p)
            u2 = cv.lmul(aff["p"][0], a[2])
            a[0] = cv.limbs([u - v for u, v in zip(u2, ppv)])
            if not cv.in_classes(a):
                continue
            assert cv.point(a) == q
            break
        else:
            raise AssertionError("no near miss found")
        cases.append(dict(acc=a, **aff))
        want.append(cv.C.add(q, p))
        passes.append(kind == "filter")
    return cases, want, passes


def test_madd_near_misses_take_the_general_formula(hooks, cv):
    cases, want, passes = _near_misses(cv, random.Random(2923))
    got, _ = hooks.ec(cv.g2, M.E_MADD, cases)
    sel, special = hooks.ec(cv.g2, M.E_MADD_SELECT, cases)
    _, may = hooks.field("fq2" if cv.g2 else "fq", M.F_MAYBE_ZERO,
                         [([x - y for x, y in zip(cv.limbs(cv.lmul(c["p"][0], c["acc"][2])), c["acc"][0])],) for c in cases])
    for i, w in enumerate(want):
        cv.check(got[i], w, ("near miss", i))
        assert bool(may[i]) == passes[i] and bool(special[i]) == passes[i], i
        if not special[i]:
            cv.check(sel[i], w, ("near miss, madd_select", i))
    assert sum(passes) >= 8 and not all(passes)


# ---- add ----------------------------------------------------------------------------------------------------------
def _pp_multiple(cv, a, q):
    """j per component with Pp = U2 - U1 = j p (None if P != +-Q)"""
    u1, u2 = cv.lmul(a[0], q[2]), cv.lmul(q[0], a[2])
    d = [y - x for x, y in zip(u1, u2)]
    return tuple(v // P for v in d) if all(v % P == 0 for v in d) else None


def test_add(hooks, cv):
    rng = random.Random(2924)
    k = cv.k
    cases, want = [], []
    for i in range(64):                                                        # generic
        a, b = cv.pts[i % 40], cv.pts[(i * 7 + 1) % 40]
        cases.append(dict(acc=cv.varied_acc(a, rng, i), q=cv.varied_acc(b, rng, i + 1)))
        want.append(cv.C.add(a, b))
    inf = cv.acc(None, None)
    cases += [dict(acc=inf, q=cv.varied_acc(cv.pts[2], rng, 3)), dict(acc=cv.varied_acc(cv.pts[6], rng, 2), q=inf),
              dict(acc=inf, q=inf)]
    want += [cv.pts[2], cv.pts[6], None]
    js = [set() for _ in range(k)]
    for i in range(90):                                                        # P = +-Q, another z and other shifts
        pt = cv.pts[i % 40]
        hi = i % 3                   # products pushed out of [0, p): x near +-8p against zz in (p, 2p) / (-p, 0)
        kx1 = tuple((7, -8, rng.randint(-8, 7))[hi] for _ in range(k))
        kx2 = tuple((-8, 7, rng.randint(-8, 7))[hi] for _ in range(k))
        kz = lambda: tuple(rng.choice((1, 1, -1, 0)) for _ in range(k))
        a = cv.acc(pt, cv.rand_elt(rng), kx1, tuple(rng.randint(-3, 2) for _ in range(k)), kz(), kz())
        other = pt if i % 2 == 0 else cv.C.neg(pt)
        b = cv.acc(other, cv.rand_elt(rng), kx2, tuple(rng.randint(-3, 2) for _ in range(k)), kz(), kz())
        if i % 9 == 4:
            b = cv.extreme_x_acc(other, rng)
        assert cv.in_classes(a) and cv.in_classes(b) and a[2] != b[2]
        j = _pp_multiple(cv, a, b)
        assert j is not None
        for c in range(k):
            js[c].add(j[c])
        cases.append(dict(acc=a, q=b))
        want.append(cv.C.add(pt, pt) if i % 2 == 0 else None)
    for c in range(k):
        assert js[c] >= {-1, 0, 1}, js                                         # the coverage this test claims
    assert len(cases) % 64 != 0
    got, _ = hooks.ec(cv.g2, M.E_ADD, cases)
    for i, w in enumerate(want):
        cv.check(got[i], w, ("add", i))
    assert cv.split(got[64])[:4] == cases[64]["q"] and cv.split(got[65])[:4] == cases[65]["acc"]


# ---- the other operations -------------------------------------------------------------------------------------------
def test_dbl_neg_from_affine(hooks, cv):
    rng = random.Random(2925)
    accs = [cv.varied_acc(cv.pts[i], rng, i) for i in range(36)] + [cv.acc(None, None)]
    pts = cv.pts[:36] + [None]
    cases = [dict(acc=a, **cv.affine(p)) for a, p in zip(accs, pts)]
    dbl, _ = hooks.ec(cv.g2, M.E_DBL, cases)
    dba, _ = hooks.ec(cv.g2, M.E_DBL_AFFINE, cases)
    neg, _ = hooks.ec(cv.g2, M.E_NEG, cases)
    fra, _ = hooks.ec(cv.g2, M.E_FROM_AFFINE, cases)
    one = cv.limbs(cv.internal((1,) + (0,) * (cv.k - 1)))
    for i, p in enumerate(pts):
        two = None if p is None else cv.C.add(p, p)
        cv.check(dbl[i], two, ("dbl_in_place", i))
        cv.check(dba[i], two, ("dbl_affine", i))
        cv.check(neg[i], None if p is None else cv.C.neg(p), ("neg", i))
        a = cv.check(fra[i], p, ("from_affine", i))
        if p is not None:
            assert a == cases[i]["p"] + [one, one]
            assert cv.split(neg[i])[0] == accs[i][0] and cv.split(neg[i])[2:4] == accs[i][2:]


def test_to_affine_both_ways(hooks, cv):
    rng = random.Random(2926)
    pts = cv.pts[:21] + [None]
    cases = [dict(acc=cv.varied_acc(p, rng, i) if p else cv.acc(None, None)) for i, p in enumerate(pts)]
    fer, inf1 = hooks.ec(cv.g2, M.E_TO_AFFINE, cases)
    var, inf2 = hooks.ec(cv.g2, M.E_TO_AFFINE_VARTIME, cases)
    for i, p in enumerate(pts):
        a, b = cv.split(fer[i])[:2], cv.split(var[i])[:2]
        assert a == b and inf1[i] == inf2[i] == (p is None), i
        if p is not None:                                                      # canonical, internal form
            assert a == cv.affine(p)["p"], i


def _storage_words(cv, pt):
    """Affine<F> in the storage form: Montgomery R = 2^256 words, all-zero = infinity"""
    if pt is None:
        return [0] * (16 * cv.k)
    return [w for c in pt for v in cv.elt(c) for w in M.words(v * (1 << 256) % P)]


def test_hbm_conversions(hooks, cv):
    rng = random.Random(2927)
    pts = cv.pts[:20] + [None]
    nw = 8 * cv.k
    # affine_from_mont256
    got, inf = hooks.ec(cv.g2, M.E_AFFINE_FROM_MONT, [dict(p=[_storage_words(cv, p)]) for p in pts])
    for i, p in enumerate(pts):
        assert inf[i] == (p is None)
        if p is not None:
            x, y = cv.split(got[i])[:2]
            assert all(M.is_m_class(c[9 * h:9 * h + 9], P) for c in (x, y) for h in range(cv.k))
            assert (cv.coord(cv.true(x)), cv.coord(cv.true(y))) == p, i
    # xyzz_to_mont256
    accs = [cv.varied_acc(p, rng, i) if p else cv.acc(None, None) for i, p in enumerate(pts)]
    got, _ = hooks.ec(cv.g2, M.E_XYZZ_TO_MONT, [dict(acc=a) for a in accs])
    r256 = pow(1 << 256, -1, P)
    for i, p in enumerate(pts):
        el = [tuple(M.from_words(got[i][(e * cv.k + c) * 8:(e * cv.k + c) * 8 + 8]) for c in range(cv.k)) for e in range(4)]
        if p is None:
            assert not any(any(e) for e in el)
            continue
        assert all(v < P for e in el for v in e)
        x, y, zz, zzz = [tuple(v * r256 % P for v in e) for e in el]
        assert (cv.coord(fmul(x, finv(zz))), cv.coord(fmul(y, finv(zzz)))) == p, i
        assert x == cv.true(accs[i][0]) and zzz == cv.true(accs[i][3])
    # store_packed_affine, then load_packed_affine of what it stored
    lazy = []
    for i, p in enumerate(pts):
        if p is None:
            lazy.append(cv.affine(None))
            continue
        a = cv.varied_acc(p, rng, i)                                           # any lazy x / y pair will do
        lazy.append(dict(p=[a[0], a[1]], inf=0))
    st, _ = hooks.ec(cv.g2, M.E_STORE_PACKED_AFFINE, lazy)
    for i, c in enumerate(lazy):
        want = [v % P for e in c["p"] for v in cv.vals(e)] if not c["inf"] else [0] * (2 * cv.k)
        assert [M.from_words(st[i][8 * h:8 * h + 8]) for h in range(2 * cv.k)] == want, i
    ld, inf = hooks.ec(cv.g2, M.E_LOAD_PACKED_AFFINE, [dict(p=[list(r[:2 * nw])]) for r in st])
    for i, c in enumerate(lazy):
        assert inf[i] == c["inf"]
        x, y = cv.split(ld[i])[:2]
        assert x == cv.limbs([v % P for v in cv.vals(c["p"][0])]) and y == cv.limbs([v % P for v in cv.vals(c["p"][1])]), i


# ---- drift ----------------------------------------------------------------------------------------------------------
def test_classes_hold_along_a_chain(hooks, cv):
    """32 steps madd p / add q / double: the classes are invariants, not just true after one step"""
    rng = random.Random(2928)
    starts = []
    for i in range(5):
        a, q, p = cv.pts[3 * i], cv.pts[3 * i + 1], cv.pts[3 * i + 2]
        k = cv.k
        acc = cv.extreme_x_acc(a, rng, (-3,) * k) if i % 2 else cv.acc(a, cv.rand_elt(rng), ((-8, 7)[i // 2 % 2],) * k,
                                                                     (2,) * k, (1,) * k, (-1,) * k)
        starts.append((a, q, p, dict(acc=acc, q=cv.varied_acc(q, rng, i + 1), **cv.affine(p))))
    got, _ = hooks.ec(cv.g2, M.E_CHAIN, [s[3] for s in starts])
    for i, (a, q, p, _) in enumerate(starts):
        rows = cv.split(got[i])
        for step in range(M.CHAIN_STEPS):
            a = cv.C.add(a, p) if step % 3 == 0 else cv.C.add(a, q) if step % 3 == 1 else cv.C.add(a, a)
            cv.check([x for part in rows[4 * step:4 * step + 4] for x in part], a, ("chain", i, step))
            assert a is not None
