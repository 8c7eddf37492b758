"""field29.h -- the lazy 9 x 29-bit limbs -- operation by operation against Python integers.

Raw limbs go in and RAW limbs come back (tests/arith/arith_hooks.hip), on the emulator build (F29_CHECK asserts on:
an input outside a product's contract aborts) and on the gfx950 build of the same file.  The reference is exact
integer arithmetic, so nothing here has a tolerance: a product must return the integer (T + m p) / 2^261 and not
merely its residue, and every output must lie in the limb / value class its header comment promises.  Every case is
asserted to be inside the documented input contract before it is sent."""
import random

import pytest

import bn254_ref as o
import lazy_model as M
from lazy_model import ALT, LIMB, MINUS, PLUS, RP, SIGNS, edge, norm, value
from test_emu_arith import _edge

E8, E16, WIDE = LIMB + 8, LIMB + 16, 2 * LIMB + 16        # +-(2^29 + 8), +-(2^29 + 16), +-(2^30 + 16)


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks(request):
    return M.load_hooks(request)


PRIME = ["fq", "fr"]


def _p(f):
    return M.FIELDS[f][1]


def _split(row, f):
    return [list(map(int, row[:9]))] if M.FIELDS[f][2] == 9 else [list(map(int, row[:9])), list(map(int, row[9:]))]


# ---- products -----------------------------------------------------------------------------------------------------
def _mul_cases(p, rng):
    """(a, b) for a * b"""
    cs = [(norm(rng.randrange(p)), norm(rng.randrange(p))) for _ in range(120)]
    tens = lambda x: x * p // 10
    targets = ((8 * p, -13 * p), (-9 * p, 13 * p), (tens(129), -13 * p), (-tens(129), -13 * p), (0, 13 * p),
               (p // 3, -5 * p), (12 * p, 13 * p))
    for mag in (E8, WIDE):
        w = min(M.COL_MAX // (9 * mag) - 1, WIDE)         # the other side as wide as the column bound allows
        for sa in SIGNS:
            for sb in SIGNS:
                for ta, tb in targets:
                    cs.append((edge(sa, mag, ta), edge(sb, w, tb)))
                    cs.append((edge(sb, w, tb), edge(sa, mag, ta)))
    top = 12 * p >> 232                                    # the top limb near its bound, the others zero / maximal
    cs.append(([0] * 8 + [top], [0] * 8 + [-top]))
    cs.append(([LIMB - 1] * 8 + [top], [LIMB - 1] * 8 + [top - 1]))
    one = norm(RP % p)
    a = norm(rng.randrange(p))
    for x in ([0] * 9, norm(1), one, norm(p), norm(-p), norm(-1)):
        cs += [(x, a), (a, x), (x, x)]
    for _ in range(16):                                    # T = a b negative
        cs.append((norm(-rng.randrange(13 * p)), norm(rng.randrange(p))))
        cs.append((norm(rng.randrange(p)), norm(-rng.randrange(13 * p))))
    return cs


def _sqr_cases(p, rng):
    cs = [norm(rng.randrange(p)) for _ in range(120)]
    w = int((M.COL_MAX // 9) ** 0.5) - 1                   # 9 w^2 at the column bound: about 1.6 * 2^29
    assert w > E16
    for mag in (E8, E16, w):
        for s in SIGNS:
            for t in (12 * p, -12 * p, 129 * p // 10, -129 * p // 10, 8 * p, -9 * p, 0, p // 3):
                cs.append(edge(s, mag, t))
    cs += [[0] * 9, norm(1), norm(RP % p), norm(p), norm(-p), norm(-1), [0] * 8 + [12 * p >> 232],
           [LIMB - 1] * 8 + [-(12 * p >> 232)]]
    cs += [norm(-rng.randrange(12 * p)) for _ in range(16)]
    return cs


def _mul2_cases(p, rng):
    """(a, b, c, d) for a b + c d and a b - c d: limbs within +-(2^29 + 16), |a b| + |c d| < 169 p^2"""
    cs = [tuple(norm(rng.randrange(p)) for _ in range(4)) for _ in range(120)]
    targets = ((8 * p, 9 * p, 9 * p, 10 * p), (-8 * p, 9 * p, 9 * p, -10 * p), (8 * p, -9 * p, -9 * p, -10 * p),
               (129 * p // 10, 13 * p, 0, 0), (0, p, -129 * p // 10, 13 * p), (-9 * p, -9 * p, 9 * p, 9 * p),
               (p // 3, -5 * p, 7 * p, p // 5))
    pats = [(sa, sb, sc, sd) for sa in SIGNS for sb in SIGNS for sc, sd in ((PLUS, PLUS), (MINUS, ALT), (ALT, MINUS))]
    for sg in pats:                                        # all four operands at +-(2^29 + 16)
        for tg in targets:
            cs.append(tuple(edge(s, E16, t) for s, t in zip(sg, tg)))
    one, a, b = norm(RP % p), norm(rng.randrange(p)), norm(rng.randrange(p))
    for x in ([0] * 9, norm(1), one, norm(p), norm(-p)):
        cs += [(x, a, b, x), (a, x, x, b), (x, x, x, x), (a, b, a, b), (a, b, b, a)]
    for _ in range(16):
        cs.append((norm(-rng.randrange(8 * p)), norm(rng.randrange(p)), norm(rng.randrange(p)), norm(rng.randrange(9 * p))))
    return cs


def _check_m(got, want, p, what):
    assert value(got) == want, what                        # the exact integer, not its residue
    assert M.is_m_class(got, p), (what, got)


@pytest.mark.parametrize("f", PRIME)
def test_mul_exact_value_and_class(hooks, f):
    p = _p(f)
    cs = _mul_cases(p, random.Random(2901))
    assert len(cs) % 64 != 0 and len(cs) > 300
    for a, b in cs:
        assert M.in_contract([(a, b)], p), (a, b)
    assert any(value(a) * value(b) < 0 for a, b in cs)
    assert any(10 * abs(value(a) * value(b)) > 1670 * p * p for a, b in cs)         # the value bound is approached
    out, _ = hooks.field(f, M.F_MUL, cs)
    for i, (a, b) in enumerate(cs):
        _check_m(_split(out[i], f)[0], M.mont_exact(value(a) * value(b), p), p, ("mul", f, i))


@pytest.mark.parametrize("f", PRIME)
def test_sqr_exact_value_and_class(hooks, f):
    p = _p(f)
    cs = _sqr_cases(p, random.Random(2902))
    assert len(cs) % 64 != 0 and len(cs) > 200
    for a in cs:
        assert M.in_contract([(a, a)], p), a
    out, _ = hooks.field(f, M.F_SQR, [(a,) for a in cs])
    for i, a in enumerate(cs):
        _check_m(_split(out[i], f)[0], M.mont_exact(value(a) ** 2, p), p, ("sqr", f, i))


@pytest.mark.parametrize("f", PRIME)
def test_mul2_and_mul_sub_exact_value_and_class(hooks, f):
    p = _p(f)
    cs = _mul2_cases(p, random.Random(2903))
    assert len(cs) % 64 != 0 and len(cs) > 300
    for a, b, c, d in cs:
        assert M.in_contract([(a, b), (c, d)], p), (a, b, c, d)
    assert sum(all(abs(x) == E16 for op in c for x in op[:8]) for c in cs) >= 100
    add, _ = hooks.field(f, M.F_MUL2, cs)
    sub, _ = hooks.field(f, M.F_MUL_SUB, cs)
    neg = 0
    for i, (a, b, c, d) in enumerate(cs):
        ab, cd = value(a) * value(b), value(c) * value(d)
        neg += (ab - cd) < 0
        _check_m(_split(add[i], f)[0], M.mont_exact(ab + cd, p), p, ("mul2", f, i))
        _check_m(_split(sub[i], f)[0], M.mont_exact(ab - cd, p), p, ("mul_sub", f, i))
    assert neg > 20


def _fq2_pool(p, rng):
    """components a caller may hold: limbs within +-(2^29 + 8), |value| < 9 p (F29x2's header)"""
    pool = [norm(rng.randrange(p)) for _ in range(12)]
    for s in SIGNS:
        for t in (8 * p, -8 * p, 3 * p, 0, -5 * p, p // 3):
            pool.append(edge(s, E8, t))
    top = 8 * p >> 232
    pool += [[0] * 9, norm(1), norm(RP % p), norm(p), norm(-p), [0] * 8 + [top], [LIMB - 1] * 8 + [-top]]
    return pool


def _fq2_mul_T(a, b):
    return (value(a[0]) * value(b[0]) - value(a[1]) * value(b[1]), value(a[0]) * value(b[1]) + value(a[1]) * value(b[0]))


def _fq2_mul_ok(a, b, p):
    return M.in_contract([(a[0], b[0]), (a[1], b[1])], p) and M.in_contract([(a[0], b[1]), (a[1], b[0])], p)


def _fq2_operands(p, seed, n):
    rng = random.Random(seed)
    pool = _fq2_pool(p, rng)
    xs = [(pool[i % len(pool)], pool[(7 * i + 3) % len(pool)]) for i in range(len(pool))]        # every pattern once
    xs += [(rng.choice(pool), rng.choice(pool)) for _ in range(n - len(xs))]
    for a in xs:
        assert all(abs(x) <= E8 for c in a for x in c[:8]) and all(abs(value(c)) < 9 * p for c in a)
    return xs


def test_fq2_mul_exact_value_and_class(hooks):
    p = o.Q_MOD
    xs, ys = _fq2_operands(p, 2904, 331), _fq2_operands(p, 2905, 331)
    ys = ys[::-1]
    for a, b in zip(xs, ys):
        assert _fq2_mul_ok(a, b, p)
    out, _ = hooks.field("fq2", M.F_MUL, [(a[0] + a[1], b[0] + b[1]) for a, b in zip(xs, ys)])
    for i, (a, b) in enumerate(zip(xs, ys)):
        t0, t1 = _fq2_mul_T(a, b)
        g0, g1 = _split(out[i], "fq2")
        _check_m(g0, M.mont_exact(t0, p), p, ("fq2 mul c0", i))
        _check_m(g1, M.mont_exact(t1, p), p, ("fq2 mul c1", i))


def test_fq2_sqr_exact_value_and_class(hooks):
    p = o.Q_MOD
    xs = _fq2_operands(p, 2906, 331)
    for c0, c1 in xs:                      # sqr = (c0 + c1).carry() * (c0 - c1) | 2 c0 * c1
        s = M.carry([x + y for x, y in zip(c0, c1)])
        d = [x - y for x, y in zip(c0, c1)]
        assert M.in_contract([(s, d)], p) and M.in_contract([([2 * x for x in c0], c1)], p)
    out, _ = hooks.field("fq2", M.F_SQR, [(c0 + c1,) for c0, c1 in xs])
    for i, (c0, c1) in enumerate(xs):
        v0, v1 = value(c0), value(c1)
        g0, g1 = _split(out[i], "fq2")
        _check_m(g0, M.mont_exact((v0 + v1) * (v0 - v1), p), p, ("fq2 sqr c0", i))
        _check_m(g1, M.mont_exact(2 * v0 * v1, p), p, ("fq2 sqr c1", i))


def test_fq2_mul_sub_exact_value_and_carried_bounds(hooks):
    """(a b - c d).carry(): the difference of two M-class products has limbs in (-2^29, 2^29), so the carry step
    (k = 0 of its contract) leaves limbs 0..7 in [-1, 2^29 + 1); the value is the difference of two in (-p, 2p)"""
    p = o.Q_MOD
    A, B, Cc, D = (_fq2_operands(p, 2907 + k, 203) for k in range(4))
    B, D = B[::-1], D[::-1]
    for a, b, c, d in zip(A, B, Cc, D):
        assert _fq2_mul_ok(a, b, p) and _fq2_mul_ok(c, d, p)
    out, _ = hooks.field("fq2", M.F_MUL_SUB, [tuple(x[0] + x[1] for x in q) for q in zip(A, B, Cc, D)])
    for i, (a, b, c, d) in enumerate(zip(A, B, Cc, D)):
        tab, tcd = _fq2_mul_T(a, b), _fq2_mul_T(c, d)
        for k, g in enumerate(_split(out[i], "fq2")):
            assert value(g) == M.mont_exact(tab[k], p) - M.mont_exact(tcd[k], p), (i, k)
            assert M.in_class(g, p, -3, 3, 1) and abs(g[8]) < (1 << 24), (i, k, g)


# ---- carry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ["fq", "fr", "fq2"])
def test_carry_keeps_the_value_and_bounds_the_limbs(hooks, f):
    rng = random.Random(2910)
    W = M.FIELDS[f][2]
    cs, ks = [], []
    for k in (1, 2, 3):
        bound = min((1 << (29 + k)) - 1, M.INT32 - 1)       # k = 3: all an int32 limb can hold
        pats = [[s(i) * bound for i in range(8)] for s in SIGNS] + [[-s(i) * bound for i in range(8)] for s in (ALT,)]
        pats += [[rng.randint(-bound, bound) for _ in range(8)] for _ in range(41)]
        pats += [[rng.choice((-bound, bound, -LIMB, LIMB, LIMB - 1, -1, 0)) for _ in range(8)] for _ in range(20)]
        for low in pats:
            for top in (rng.randint(-(1 << 26), -1), rng.randint(0, 1 << 26)):
                cs.append(low + [top])
                ks.append(k)
    if W == 18:
        cs = [a + b for a, b in zip(cs, cs[1:] + cs[:1])]
    assert len(cs) % 64 != 0
    out, _ = hooks.field(f, M.F_CARRY, [(c,) for c in cs])
    for i, c in enumerate(cs):
        for h, g in enumerate(_split(out[i], f)):
            src = c[9 * h:9 * h + 9]
            k = ks[(i + h) % len(ks)]
            assert value(g) == value(src), i                                   # exact, not mod p
            assert all(-(1 << k) <= x < LIMB + (1 << k) for x in g[:8]), (i, k, g)
            assert g == M.carry(src)


# ---- canonical / is_zero_mod_p / maybe_zero_mod_p -------------------------------------------------------------------
def _drift(v, cs):
    """the limbs of v with c_i 2^29 moved from limb i + 1 into limb i: the same value, limbs up to +-(2^31 - 2^4)"""
    l = norm(v)
    for i, c in enumerate(cs):
        if c == 3 and l[i] + 3 * LIMB > M.INT32 - 16:
            c = 2
        if c == -4 and l[i] - 4 * LIMB < -(M.INT32 - 16):
            c = -3
        l[i] += c * LIMB
        l[i + 1] -= c
    assert value(l) == v and all(abs(x) <= M.INT32 - 16 for x in l)
    return l


def _zero_cases(p, rng):
    """(limbs, value) for j p, j p +- 1 and random v + j p, j in [-31, 31], normalised and drifted"""
    cs = []
    drifts = ([3] * 8, [-4] * 8, [3, -4] * 4, [-4, 3] * 4)
    for j in range(-31, 32):
        vals = [j * p, j * p + 1, j * p - 1, j * p + rng.randrange(p), j * p + rng.randrange(p)]
        for v in vals:
            assert abs(v) < 32 * p
            cs.append((norm(v), v))
            cs.append((_drift(v, drifts[(j + len(cs)) % 4]), v))
            cs.append((_drift(v, [rng.randint(-4, 3) for _ in range(8)]), v))
    assert max(max(map(abs, l)) for l, _ in cs) > M.INT32 - 16 - LIMB // 2
    return cs


@pytest.mark.parametrize("f", PRIME)
def test_canonical_and_zero_tests(hooks, f):
    p = _p(f)
    cs = _zero_cases(p, random.Random(2911))
    assert len(cs) % 64 != 0
    ops = [(l,) for l, _ in cs]
    can, _ = hooks.field(f, M.F_CANONICAL, ops)
    _, isz = hooks.field(f, M.F_IS_ZERO, ops)
    _, may = hooks.field(f, M.F_MAYBE_ZERO, ops)
    multiples = 0
    for i, (l, v) in enumerate(cs):
        assert _split(can[i], f)[0] == norm(v % p), (i, v // p)                # the representative in [0, p), normalised
        assert bool(isz[i]) == (v % p == 0), (i, v // p)
        if v % p == 0:
            multiples += 1
            assert may[i] == 1, ("maybe_zero_mod_p misses a multiple of p", v // p)
    assert multiples == 63 * 3


def test_fq2_canonical_and_zero_tests(hooks):
    p = o.Q_MOD
    cs = _zero_cases(p, random.Random(2912))
    zeros = [c for c in cs if c[1] % p == 0]
    pairs = list(zip(cs, cs[5:] + cs[:5])) + list(zip(zeros, zeros[7:] + zeros[:7]))
    assert len(pairs) % 64 != 0
    ops = [(a[0] + b[0],) for a, b in pairs]
    can, _ = hooks.field("fq2", M.F_CANONICAL, ops)
    _, isz = hooks.field("fq2", M.F_IS_ZERO, ops)
    _, may = hooks.field("fq2", M.F_MAYBE_ZERO, ops)
    both = 0
    for i, (a, b) in enumerate(pairs):
        assert _split(can[i], "fq2") == [norm(a[1] % p), norm(b[1] % p)], i
        z = a[1] % p == 0 and b[1] % p == 0
        both += z
        assert bool(isz[i]) == z, i
        if z:
            assert may[i] == 1, i
    assert both >= 63 * 3


# ---- conversions --------------------------------------------------------------------------------------------------
def _lazy_forms(v, p, rng):
    """a canonical value as the lazy registers may hold it: shifted by multiples of p, limbs within +-8 of normal"""
    yield norm(v)
    for k in (-8, -3, -1, 1, 2, 7):
        yield norm(v + k * p)
    l = norm(v + rng.randint(-7, 6) * p)
    d = [rng.randint(-8, 7) for _ in range(8)]
    yield [l[0] + d[0]] + [l[i] + d[i] for i in range(1, 8)] + [l[8]]           # value changes: recomputed by callers


@pytest.mark.parametrize("f", PRIME)
def test_pack_unpack_and_montgomery_conversions(hooks, f):
    p = _p(f)
    rng = random.Random(2913)
    xs = _edge(p, rng, 90)
    assert 0 in xs and p - 1 in xs and len(xs) % 64 != 0
    # unpack o pack on canonical values
    packed, _ = hooks.field(f, M.F_PACK, [(norm(x),) for x in xs])
    assert [M.from_words(r[:8]) for r in packed] == xs
    unp, _ = hooks.field(f, M.F_UNPACK, [(M.words(x),) for x in xs])
    assert [_split(r, f)[0] for r in unp] == [norm(x) for x in xs]
    # from_mont256: storage form x R -> internal x R', M class, and the exact product with 2^266 mod p
    c266 = (1 << 266) % p
    stor = [x * (1 << 256) % p for x in xs]
    fm, _ = hooks.field(f, M.F_FROM_MONT, [(M.words(w),) for w in stor])
    for i, (x, w) in enumerate(zip(xs, stor)):
        g = _split(fm[i], f)[0]
        assert M.is_m_class(g, p) and value(g) % p == x * RP % p, i
        assert value(g) == M.mont_exact(w * c266, p), i
    # to_mont256 / pack_internal of lazy registers
    lazy = [l for x in xs for l in _lazy_forms(x * RP % p, p, rng)]
    one256 = norm((1 << 256) % p)
    for l in lazy:
        assert M.in_contract([(l, one256)], p) and abs(value(l)) < 32 * p
    tm, _ = hooks.field(f, M.F_TO_MONT, [(l,) for l in lazy])
    pi, _ = hooks.field(f, M.F_PACK_INTERNAL, [(l,) for l in lazy])
    rpi = pow(RP, -1, p)
    for i, l in enumerate(lazy):
        assert M.from_words(tm[i][:8]) == value(l) * rpi * (1 << 256) % p, i
        assert M.from_words(pi[i][:8]) == value(l) % p, i
    if f == "fq":
        ld, _ = hooks.field(f, M.F_LOAD_PACKED, [(M.words(x),) for x in xs])
        assert [_split(r, f)[0] for r in ld] == [norm(x) for x in xs]
        stp, _ = hooks.field(f, M.F_STORE_PACKED, [(l,) for l in lazy])
        assert [M.from_words(r[:8]) for r in stp] == [value(l) % p for l in lazy]
        back, _ = hooks.field(f, M.F_LOAD_PACKED, [(list(r[:8]),) for r in stp])
        assert [value(r[:9]) for r in back] == [value(l) % p for l in lazy]


def test_fq2_montgomery_conversions_and_packed_form(hooks):
    p = o.Q_MOD
    rng = random.Random(2914)
    xs = _edge(p, rng, 60)
    ys = xs[3:] + xs[:3]
    assert len(xs) % 64 != 0
    stor = [(x * (1 << 256) % p, y * (1 << 256) % p) for x, y in zip(xs, ys)]
    fm, _ = hooks.field("fq2", M.F_FROM_MONT, [(M.words(a) + M.words(b),) for a, b in stor])
    for i, (x, y) in enumerate(zip(xs, ys)):
        g0, g1 = _split(fm[i], "fq2")
        assert M.is_m_class(g0, p) and M.is_m_class(g1, p)
        assert (value(g0) % p, value(g1) % p) == (x * RP % p, y * RP % p), i
    lazy = [(a, b) for x, y in zip(xs, ys) for a, b in zip(_lazy_forms(x * RP % p, p, rng), _lazy_forms(y * RP % p, p, rng))]
    ops = [(a + b,) for a, b in lazy]
    rpi = pow(RP, -1, p)
    tm, _ = hooks.field("fq2", M.F_TO_MONT, ops)
    stp, _ = hooks.field("fq2", M.F_STORE_PACKED, ops)
    for i, (a, b) in enumerate(lazy):
        assert (M.from_words(tm[i][:8]), M.from_words(tm[i][8:16])) == tuple(value(c) * rpi * (1 << 256) % p for c in (a, b)), i
        assert (M.from_words(stp[i][:8]), M.from_words(stp[i][8:16])) == (value(a) % p, value(b) % p), i
    # load_packed (the opaque limbs) of the stored words: the canonical value, normalised limbs
    back, _ = hooks.field("fq2", M.F_LOAD_PACKED, [(list(r[:16]),) for r in stp])
    for i, (a, b) in enumerate(lazy):
        assert _split(back[i], "fq2") == [norm(value(a) % p), norm(value(b) % p)], i


# ---- inversions ---------------------------------------------------------------------------------------------------
def _inv_inputs(p, rng):
    base = [1, p - 1, 2, (p - 1) // 2] + [rng.randrange(1, p) for _ in range(20)]
    base += [v * RP % p for v in base[:4]]                                     # the same as internal forms
    cs = [norm(v) for v in base]
    for v in base[:12]:
        for k in (-31, -17, -8, -1, 1, 8, 30):                                 # lazy: negative, up to the 32 p of canonical()
            cs.append(norm(v + k * p))
        l = norm(v + rng.randint(-7, 6) * p)
        cs.append([x + rng.randint(-8, 7) for x in l[:8]] + [l[8]])
    cs = [c for c in cs if value(c) % p]
    assert all(abs(value(c)) < 32 * p for c in cs) and any(value(c) < -16 * p for c in cs)
    return cs


@pytest.mark.parametrize("f", PRIME)
def test_inversions(hooks, f):
    p = _p(f)
    cs = _inv_inputs(p, random.Random(2915))
    zeros = [[0] * 9] + [norm(j * p) for j in (1, -1, 5, -31)]
    allc = cs + zeros
    assert len(allc) % 64 != 0
    m_top = [LIMB - 1] * 8 + [2 * p >> 232]
    for c in allc:
        assert M.in_contract([(m_top, c)], p)                                   # r * a with r in M class
    fer, _ = hooks.field(f, M.F_INV, [(c,) for c in allc])
    var, _ = hooks.field(f, M.F_INV_VARTIME, [(c,) for c in allc])
    for i, c in enumerate(allc):
        a, b = _split(fer[i], f)[0], _split(var[i], f)[0]
        assert M.is_m_class(a, p) and M.is_m_class(b, p), i
        assert value(a) % p == value(b) % p, i                                 # the two inversions agree
        want = 0 if value(c) % p == 0 else RP * RP % p                          # r a / R' = the internal one
        assert value(a) * value(c) % p == want and value(b) * value(c) % p == want, i
        if value(c) % p == 0:
            assert value(a) % p == 0 and b == [0] * 9, i                        # 0 -> 0
    assert _split(fer[len(cs)], f)[0] == [0] * 9


def test_fq2_inversions(hooks):
    p = o.Q_MOD
    rng = random.Random(2916)
    comp = [norm(v) for v in (0, 1, p - 1, 2, (p - 1) // 2, RP % p)] + [norm(rng.randrange(p)) for _ in range(10)]
    comp += [norm(rng.randrange(p) + k * p) for k in (-8, -5, -1, 1, 4, 7)]
    comp += [edge(s, E8, t) for s in SIGNS for t in (8 * p, -8 * p, p // 3)]
    cs = [(rng.choice(comp), rng.choice(comp)) for _ in range(100)] + [(comp[1], comp[0]), (comp[0], comp[1])]
    cs = [c for c in cs if value(c[0]) % p or value(c[1]) % p] + [([0] * 9, [0] * 9)]
    assert len(cs) % 64 != 0
    m_top = [LIMB - 1] * 8 + [2 * p >> 232]
    for c0, c1 in cs:
        assert M.in_contract([(c0, c0), (c1, c1)], p) and M.in_contract([(c0, m_top)], p) and M.in_contract([(c1, m_top)], p)
    fer, _ = hooks.field("fq2", M.F_INV, [(c0 + c1,) for c0, c1 in cs])
    var, _ = hooks.field("fq2", M.F_INV_VARTIME, [(c0 + c1,) for c0, c1 in cs])
    one = RP * RP % p
    for i, (c0, c1) in enumerate(cs):
        a, b = _split(fer[i], "fq2"), _split(var[i], "fq2")
        for r in (a, b):
            assert M.is_m_class(r[0], p) and M.is_m_class([-x for x in r[1]], p), i      # (c0 n, -(c1 n))
        ra, rb = [tuple(value(c) % p for c in r) for r in (a, b)]
        assert ra == rb, i
        x = (value(c0) % p, value(c1) % p)
        want = (0, 0) if x == (0, 0) else (one, 0)
        assert o.f2_mul(ra, x) == want, i
    assert _split(fer[-1], "fq2") == [[0] * 9, [0] * 9] and _split(var[-1], "fq2") == [[0] * 9, [0] * 9]
