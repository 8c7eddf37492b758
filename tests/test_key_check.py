"""Proving-key validation on the GPU (g16_key_check / cc.check_key / cc.read_zkey(validate=True)).

Structural checks: every point of every query canonical, on its curve and (G2) in the r-torsion; the
expected (query, index, reason) lists are the PLANTED faults, never what the library reports.  Relations:
e(beta_g1, g2) = e(g1, beta_g2), the same for delta, and e(sum rho_i B1_i, g2) = e(g1, sum rho_i B2_i);
expected verdicts come from the oracle (oracle/bn254_ref.py): its curve arithmetic, msm and pairing.

A point's reason is the first test it fails (non-canonical, off the curve, outside the subgroup): the
later tests mean nothing on such a point (include/g16_amd.h)."""
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_verify import _twist_point_outside_g2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONCANON, OFF_CURVE, SUBGROUP = 1, 2, 4
PAIR_BETA, PAIR_DELTA, PAIR_B, VK_MISMATCH = 1, 2, 4, 8
CHUNK = 16           # G16_KEYCHECK_CHUNK of the small cases: the 64-wire chain key is 4 chunks per query
QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query", "ic", "singles")
SINGLES = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2")


def _rho(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


def _clone(cc, pk):
    """a ProvingKey with its own writable copies of every array"""
    vk = cc.VerifyingKey(bytes(pk.vk.alpha_g1), bytes(pk.vk.beta_g2), bytes(pk.vk.gamma_g2), bytes(pk.vk.delta_g2),
                         np.array(pk.vk.gamma_abc_g1, dtype=np.uint8, copy=True))
    return cc.ProvingKey(pk.n_vars, pk.n_public, pk.domain_size, vk, bytes(pk.beta_g1), bytes(pk.delta_g1),
                         *(np.array(getattr(pk, q), dtype=np.uint8, copy=True)
                           for q in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")))


_keys = {}


def _chain_key(cc, lib, k=6, seed=606):
    """cc.trapdoor_setup key of the squaring chain at 2^k (n_vars = 2^k, one public input)"""
    key = (id(lib), k, seed)
    if key not in _keys:
        cons, _w, n_vars, n_pub = H.squaring_chain(k)
        A, Bm, Cm = (cc.Csr.from_rows([[(cf, idx) for idx, cf in row[j]] for row in cons], lib) for j in range(3))
        rng = random.Random(seed)
        tox = [rng.randrange(1, o.R_MOD) for _ in range(5)]
        _keys[key] = cc.trapdoor_setup(A, Bm, Cm, n_vars, n_pub, tox, lib=lib)
    return _clone(cc, _keys[key])


def _get(pk, q, i):
    if q == "ic":
        return bytes(pk.vk.gamma_abc_g1[i])
    if q == "singles":
        name = SINGLES[i]
        return bytes(getattr(pk.vk, name) if name in ("alpha_g1", "beta_g2", "delta_g2", "gamma_g2") else getattr(pk, name))
    return bytes(getattr(pk, q)[i])


def _put(pk, q, i, raw):
    if q == "ic":
        pk.vk.gamma_abc_g1[i] = np.frombuffer(raw, dtype=np.uint8)
    elif q == "singles":
        name = SINGLES[i]
        setattr(pk.vk if name in ("alpha_g1", "beta_g2", "delta_g2", "gamma_g2") else pk, name, bytes(raw))
    else:
        getattr(pk, q)[i] = np.frombuffer(raw, dtype=np.uint8)


def _plus_q(raw, word):
    """stored value m of 32-byte word `word` -> m + q (< 2^256): a second encoding of the same element"""
    off = 32 * word
    v = int.from_bytes(raw[off:off + 32], "little") + o.Q_MOD
    assert v < 1 << 256
    return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]


def _y_plus_1(raw):
    """the first word of y + 1: another residue, so the point leaves its curve"""
    off = len(raw) // 2
    v = int.from_bytes(raw[off:off + 32], "little") + 1
    assert v < o.Q_MOD
    return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]


def _plant(pk, q, i, kind, salt=0):
    """overwrite entry i of query q with a fault of the given kind; returns its reason bit"""
    raw = _get(pk, q, i)
    assert any(raw), (q, i)                                    # a finite point to corrupt
    if kind == "noncanon":
        _put(pk, q, i, _plus_q(raw, (i + salt) % (len(raw) // 32)))
        return NONCANON
    if kind == "offcurve":
        _put(pk, q, i, _y_plus_1(raw))
        return OFF_CURVE
    if kind == "cofactor":
        _put(pk, q, i, o.g2_to_bytes(_twist_point_outside_g2(1 + salt)))
        return SUBGROUP
    assert kind == "order10069"
    T = _twist_point_outside_g2(7)
    P = o.G2.mul(T, o.R_MOD * ((2 * o.Q_MOD - o.R_MOD) // 10069))
    assert P is not None and o.G2.mul(P, 10069) is None and o.G2.mul(P, o.R_MOD) is not None and o.G2.on_curve(P)
    _put(pk, q, i, o.g2_to_bytes(P))
    return SUBGROUP


def _oracle_pair_equal(P, Q):
    """e(P, g2) == e(g1, Q) on the CPU"""
    f = o._f12_mul(o.miller_loop(o.G2_GEN, P), o.miller_loop(Q, o.G1.neg(o.G1_GEN)))
    return o.final_exponentiation(f) == o.miller_loop(None, None)


def _oracle_pair_b(pk, rho):
    b1 = [o.g1_from_bytes(bytes(x)) for x in pk.b_g1_query]
    b2 = [o.g2_from_bytes(bytes(x)) for x in pk.b_g2_query]
    s1 = o.G1.sum([o.G1.mul(P, k) for P, k in zip(b1, rho)])
    s2 = o.G2.sum([o.G2.mul(P, k) for P, k in zip(b2, rho)])
    assert s1 == o.G1.msm(b1, rho) and s2 == o.G2.msm(b2, rho)
    return _oracle_pair_equal(s1, s2)


def _clean(rep, n_points=None):
    assert rep.ok and rep.relations_checked and rep.relations_failed == 0 and rep.bad == []
    assert all(v == 0 for v in rep.n_bad.values()), rep.n_bad
    if n_points is not None:
        assert rep.n_points == n_points


# ---- 1. real keys pass ---------------------------------------------------------------------------
def test_reference_zkey_passes(lib, golden):
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, _ = cc.read_zkey(data, lib=lib)
    opk, _ = o.read_zkey(data)
    # the oracle's view of the same key: every point on its curve, B2 in G2, the three relations
    for P in opk["a_query"] + opk["b_g1_query"] + opk["l_query"] + opk["h_query"] + opk["ic"]:
        assert o.G1.on_curve(P)
    assert all(o.G2.on_curve(P) and o.G2.mul(P, o.R_MOD) is None for P in opk["b_g2_query"])
    assert _oracle_pair_equal(opk["beta_g1"], opk["beta_g2"]) and _oracle_pair_equal(opk["delta_g1"], opk["delta_g2"])
    rho = _rho(1, pk.n_vars)
    assert _oracle_pair_b(pk, rho)
    rep = cc.check_key(pk, rho=rho, lib=lib)
    _clean(rep, dict(a_query=4, b_g1_query=4, b_g2_query=4, l_query=2, h_query=4, ic=2, singles=6))
    assert rep.n_infinity["b_g1_query"] == 3 and rep.n_infinity["b_g2_query"] == 3
    assert rep.n_infinity["b_g1_query"] == sum(P is None for P in opk["b_g1_query"])
    assert rep.n_infinity["a_query"] == sum(P is None for P in opk["a_query"])
    _clean(cc.check_key(pk, lib=lib))                                                 # rho from the OS
    rep = cc.check_key(pk, vk=False, lib=lib)
    _clean(rep)
    assert rep.n_points["ic"] == 0 and rep.n_points["singles"] == 5


def test_chain_key_passes_in_chunks(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(CHUNK))
    pk = _chain_key(cc, lib)
    assert pk.n_vars == 64 and pk.n_vars // CHUNK >= 3
    rho = _rho(2, pk.n_vars)
    assert _oracle_pair_b(pk, rho)
    rep = cc.check_key(pk, rho=rho, lib=lib)
    _clean(rep, dict(a_query=64, b_g1_query=64, b_g2_query=64, l_query=62, h_query=64, ic=2, singles=6))
    for q in ("b_g1_query", "b_g2_query"):
        assert rep.n_infinity[q] == sum(not any(bytes(x)) for x in getattr(pk, q))
    _clean(cc.check_key(pk, lib=lib))


# ---- 2. every structural reason, at its exact location --------------------------------------------
@pytest.mark.parametrize("q", ["a_query", "b_g1_query", "b_g2_query", "l_query", "h_query", "ic", "singles"])
def test_structural_faults_are_located(lib, monkeypatch, q):
    """one fault at index 0, one at a chunk boundary, one at the last index of the query (B entries that are the
    point at infinity are stepped over): the list is exactly what was planted, the relations are not evaluated"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(CHUNK))
    pk = _chain_key(cc, lib)
    n = {"ic": 2, "singles": 6}.get(q) or len(getattr(pk, q))
    where = sorted({0, CHUNK - 1, CHUNK, n - 1} & set(range(n))) if n > 6 else list(range(n))
    if q in ("b_g1_query", "b_g2_query"):
        finite = [i for i in range(n) if any(_get(pk, q, i))]
        where = sorted({min(finite, key=lambda i: (abs(i - w), i)) for w in where})
    g2 = q == "b_g2_query"
    kinds = ["noncanon", "offcurve", "cofactor", "order10069"] if g2 else ["noncanon", "offcurve"]
    planted = []
    for j, i in enumerate(where):
        kind = kinds[j % len(kinds)]
        if q == "singles" and i >= 3 and j % 3 == 2:
            kind = "cofactor"                                   # gamma_g2: on the twist, outside G2
        planted.append((q, i, _plant(pk, q, i, kind, salt=j)))
    if g2:
        assert {r for _, _, r in planted} == {NONCANON, OFF_CURVE, SUBGROUP} and len(planted) == 4
    rep = cc.check_key(pk, rho=_rho(3, pk.n_vars), lib=lib)
    assert not rep.ok and not rep.relations_checked and rep.relations_failed == 0
    assert rep.bad == planted
    assert rep.n_bad == {name: (len(planted) if name == q else 0) for name in QUERIES}
    # a list shorter than the faults: the first ones, every one still counted
    rep = cc.check_key(pk, rho=_rho(3, pk.n_vars), lib=lib, max_listed=2)
    assert rep.bad == planted[:2] and rep.n_bad[q] == len(planted) and not rep.ok
    rep = cc.check_key(pk, lib=lib, max_listed=0)
    assert rep.bad == [] and rep.n_bad[q] == len(planted) and not rep.ok


def test_faults_in_several_queries_come_sorted(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(CHUNK))
    pk = _chain_key(cc, lib)
    fin2 = [i for i in range(pk.n_vars) if any(_get(pk, "b_g2_query", i))]
    fin1 = [i for i in range(pk.n_vars) if any(_get(pk, "b_g1_query", i))]
    plan = [("h_query", 63, "offcurve"), ("a_query", 17, "noncanon"), ("b_g2_query", fin2[-1], "order10069"),
            ("b_g1_query", fin1[-1], "offcurve"), ("b_g2_query", fin2[0], "cofactor"), ("singles", 4, "noncanon"),
            ("l_query", 31, "offcurve"), ("ic", 1, "noncanon"), ("b_g1_query", fin1[0], "noncanon")]
    planted = [(q, i, _plant(pk, q, i, kind)) for q, i, kind in plan]
    planted.sort(key=lambda t: (QUERIES.index(t[0]), t[1]))
    rep = cc.check_key(pk, lib=lib)
    assert rep.bad == planted and not rep.ok and not rep.relations_checked
    assert cc.check_key(pk, lib=lib, max_listed=4).bad == planted[:4]
    assert sum(rep.n_bad.values()) == len(planted)


# ---- 3. relations ----------------------------------------------------------------------------------
def test_relations(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(CHUNK))
    base = _chain_key(cc, lib)
    rho = _rho(4, base.n_vars)
    other = o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE))
    fin = [i for i in range(base.n_vars) if any(_get(base, "b_g1_query", i))]

    def verdict(pk, **kw):
        rep = cc.check_key(pk, rho=rho, lib=lib, **kw)
        assert rep.relations_checked and rep.bad == [] and all(v == 0 for v in rep.n_bad.values())
        assert rep.ok == (rep.relations_failed == 0)
        return rep.relations_failed

    for i in (fin[0], fin[len(fin) // 2], fin[-1]):                                  # another valid G1 point
        pk = _clone(cc, base)
        _put(pk, "b_g1_query", i, other)
        assert not _oracle_pair_b(pk, rho)
        assert verdict(pk) == PAIR_B
    pk = _clone(cc, base)
    pk.beta_g1 = other
    assert verdict(pk) == PAIR_BETA
    pk.delta_g1 = other
    assert verdict(pk) == PAIR_BETA | PAIR_DELTA
    pk.beta_g1 = base.beta_g1
    assert verdict(pk) == PAIR_DELTA
    # a verifying key with another delta_g2 (a valid G2 point)
    pk = _clone(cc, base)
    vk = cc.VerifyingKey(pk.vk.alpha_g1, pk.vk.beta_g2, pk.vk.gamma_g2, o.g2_to_bytes(o.G2.mul(o.G2_GEN, 77)),
                         pk.vk.gamma_abc_g1)
    assert verdict(pk, vk=vk) == VK_MISMATCH
    assert verdict(pk, vk=False) == 0 and verdict(pk) == 0
    # B1_i at infinity opposite a finite B2_i
    pk = _clone(cc, base)
    _put(pk, "b_g1_query", fin[1], bytes(64))
    rep = cc.check_key(pk, rho=rho, lib=lib)
    assert rep.relations_failed == PAIR_B and rep.bad == [] and not rep.ok
    assert rep.n_infinity["b_g1_query"] == rep.n_infinity["b_g2_query"] + 1
    # and both at infinity: one pair fewer, still consistent
    _put(pk, "b_g2_query", fin[1], bytes(128))
    assert verdict(pk) == 0


# ---- 4. the coefficients are used ------------------------------------------------------------------
def test_coefficients_are_used(lib, monkeypatch):
    """against a KNOWN rho two entries of b_g1_query are moved so that they cancel in sum rho_i B1_i
    (B1_j + rho_k D, B1_k - rho_j D): the B relation holds under exactly that rho -- oracle (msm + pairing) and
    library agree, which pins the two sums -- and under no other"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(CHUNK))
    pk = _chain_key(cc, lib)
    rho = _rho(5, pk.n_vars)
    fin = [i for i in range(pk.n_vars) if any(_get(pk, "b_g1_query", i))]
    j, k = fin[1], fin[-2]                                                           # in different chunks
    assert j // CHUNK != k // CHUNK
    D = o.G1.mul(o.G1_GEN, 0xD15EA5E)
    bj = o.G1.add(o.g1_from_bytes(_get(pk, "b_g1_query", j)), o.G1.mul(D, rho[k]))
    bk = o.G1.sub(o.g1_from_bytes(_get(pk, "b_g1_query", k)), o.G1.mul(D, rho[j]))
    _put(pk, "b_g1_query", j, o.g1_to_bytes(bj))
    _put(pk, "b_g1_query", k, o.g1_to_bytes(bk))
    assert _oracle_pair_b(pk, rho) is True
    rep = cc.check_key(pk, rho=rho, lib=lib)
    assert rep.ok and rep.relations_checked and rep.relations_failed == 0
    other = _rho(6, pk.n_vars)
    assert _oracle_pair_b(pk, other) is False
    assert cc.check_key(pk, rho=other, lib=lib).relations_failed == PAIR_B
    swapped = list(rho)
    swapped[j], swapped[k] = rho[k], rho[j]
    assert cc.check_key(pk, rho=swapped, lib=lib).relations_failed == PAIR_B
    assert cc.check_key(pk, lib=lib).relations_failed == PAIR_B                      # drawn by the library


# ---- 5. edges --------------------------------------------------------------------------------------
def test_edges(lib, monkeypatch):
    import ctypes as C
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    pk = _chain_key(cc, lib)
    n = pk.n_vars
    for bad_rho in ([5] * (n - 1) + [0], [5] * (n - 1), [5] * (n + 1), [5] * (n - 1) + [1 << 128], [5] * (n - 1) + [-1]):
        with pytest.raises(cc.G16Error) as e:
            cc.check_key(pk, rho=bad_rho, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    # the C ABI itself refuses a zero coefficient and missing arguments
    kd = pk.to_c()
    rep = B.KeyReportC()
    rho = np.array([[5, 0]] * n, dtype=np.uint64)
    rho[n // 2] = 0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.g16_key_check(0, C.byref(kd), None, ptr(rho), None, 0, C.byref(rep)) == B.G16_ERR_INVALID
    rho[n // 2, 1] = 1                                                               # 2^64: non-zero in the high word only
    assert lib.g16_key_check(0, C.byref(kd), None, ptr(rho), None, 0, C.byref(rep)) == B.G16_OK
    assert rep.ok == 1 and rep.relations_checked == 1 and rep.n_listed == 0
    assert lib.g16_key_check(0, C.byref(kd), None, ptr(rho), None, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert lib.g16_key_check(0, None, None, None, None, 0, C.byref(rep)) == B.G16_ERR_INVALID
    assert lib.g16_key_check(0, C.byref(kd), None, None, None, 0, None) == B.G16_ERR_INVALID
    assert lib.g16_key_check(-1, C.byref(kd), None, None, None, 0, C.byref(rep)) == B.G16_ERR_INVALID
    # rho = None twice: same verdicts; explicit rho: identical reports across runs and chunk sizes
    assert cc.check_key(pk, lib=lib) == cc.check_key(pk, lib=lib)
    faulty = _clone(cc, pk)
    planted = [("a_query", 40, _plant(faulty, "a_query", 40, "offcurve")),
               ("h_query", 5, _plant(faulty, "h_query", 5, "noncanon"))]
    wrong = _clone(cc, pk)
    wrong.delta_g1 = o.g1_to_bytes(o.G1.mul(o.G1_GEN, 9))
    assert cc.check_key(faulty, lib=lib) == cc.check_key(faulty, lib=lib)
    fixed = _rho(8, n)
    reports = {}
    for chunk in (None, 7, 16, 64, 1000):
        if chunk is None:
            monkeypatch.delenv("G16_KEYCHECK_CHUNK", raising=False)
        else:
            monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(chunk))
        reports[chunk] = [cc.check_key(key, rho=fixed, lib=lib) for key in (pk, faulty, wrong)]
        assert reports[chunk] == [cc.check_key(key, rho=fixed, lib=lib) for key in (pk, faulty, wrong)]
        assert reports[chunk] == reports[None]
    good, bad, rel = reports[None]
    assert good.ok and bad.bad == planted and rel.relations_failed == PAIR_DELTA


def test_no_public_inputs(lib):
    import circom_compat_amd as cc
    m, n_vars = 5, 7
    cons = [([(1 + i, 1)], [(1 + i, 1)], [(2 + i, 1)]) for i in range(m)]
    rng = random.Random(50)
    opk = o.trapdoor_setup(cons, n_vars, 0, *[rng.randrange(1, o.R_MOD) for _ in range(5)])
    pk = H.pk_from_oracle(opk)
    rep = cc.check_key(pk, lib=lib)
    _clean(rep)
    assert rep.n_points["ic"] == 1 and rep.n_points["l_query"] == n_vars - 1 and rep.n_points["singles"] == 6
    bad = _clone(cc, pk)
    why = _plant(bad, "ic", 0, "offcurve")
    assert cc.check_key(bad, lib=lib).bad == [("ic", 0, why)]


def test_read_zkey_validate(lib, golden, tmp_path):
    import circom_compat_amd as cc
    src = os.path.join(golden, "test.zkey")
    data = open(src, "rb").read()
    pk, mats = cc.read_zkey(src, lib=lib, validate=True)
    pk0, _ = cc.read_zkey(src, lib=lib)
    for name in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query"):
        assert np.array_equal(getattr(pk, name), getattr(pk0, name))
    assert cc.read_zkey(data, lib=lib, validate=True)[0].n_vars == 4
    # one bit of a finite b_g2_query point flipped in a copy of the file
    first = next(i for i in range(pk.n_vars) if any(bytes(pk.b_g2_query[i])))
    at = data.index(bytes(pk.b_g2_query[first]))
    assert data.count(bytes(pk.b_g2_query[first])) == 1
    broken = bytearray(data)
    broken[at + 70] ^= 4
    path = tmp_path / "broken.zkey"
    path.write_bytes(bytes(broken))
    bpk, _ = cc.read_zkey(str(path), lib=lib)                                        # the default still loads it
    assert bytes(bpk.b_g2_query[first]) != bytes(pk.b_g2_query[first])
    with pytest.raises(cc.G16Error) as e:
        cc.read_zkey(str(path), lib=lib, validate=True)
    assert f"b_g2_query[{first}]" in str(e.value) and "off the curve" in str(e.value)
    with pytest.raises(cc.G16Error):
        cc.read_zkey(bytes(broken), lib=lib, validate=True)
    # a well-formed but wrong beta_g1: the failed relation is named
    at = data.index(bytes(pk.beta_g1))
    swapped = data[:at] + o.g1_to_bytes(o.G1.mul(o.G1_GEN, 5)) + data[at + 64:]
    with pytest.raises(cc.G16Error) as e:
        cc.read_zkey(swapped, lib=lib, validate=True)
    assert "beta_g1" in str(e.value)


# ---- 6. GPU only -----------------------------------------------------------------------------------
def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


_gpu_key = {}


def _chain16(cc):
    if not _gpu_key:
        bench = _bench()
        mats, (A, Bm, Cm), w, n_vars = bench.chain_circuit(cc, 16)
        rng = random.Random(1616)
        pk = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)])
        _gpu_key["k"] = (pk, mats, w)
    return _gpu_key["k"]


@pytest.mark.gpu
def test_chain_2_16_passes_gpu(gpulib):
    import circom_compat_amd as cc
    pk, _mats, _w = _chain16(cc)
    rep = cc.check_key(pk, lib=gpulib)
    _clean(rep, dict(a_query=1 << 16, b_g1_query=1 << 16, b_g2_query=1 << 16, l_query=(1 << 16) - 2,
                     h_query=1 << 16, ic=2, singles=6))
    assert rep == cc.check_key(pk, rho=_rho(16, pk.n_vars), lib=gpulib)


@pytest.mark.gpu
def test_chain_2_16_planted_faults_gpu(gpulib, monkeypatch):
    """five faults spread over the chunks of a 2^16 key (four chunks of 2^14 per query)"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_KEYCHECK_CHUNK", str(1 << 14))
    pk = _clone(cc, _chain16(cc)[0])
    fin2 = [i for i in range(pk.n_vars) if any(bytes(pk.b_g2_query[i]))]
    plan = [("a_query", (1 << 14) - 1, "noncanon"), ("b_g2_query", fin2[len(fin2) // 2], "order10069"),
            ("b_g2_query", fin2[-1], "cofactor"), ("l_query", (1 << 16) - 3, "offcurve"), ("h_query", 3 << 14, "offcurve")]
    planted = [(q, i, _plant(pk, q, i, kind)) for q, i, kind in plan]
    rep = cc.check_key(pk, lib=gpulib)
    assert rep.bad == planted and not rep.ok and not rep.relations_checked
    assert sum(rep.n_bad.values()) == 5
    monkeypatch.delenv("G16_KEYCHECK_CHUNK")
    assert cc.check_key(pk, lib=gpulib) == rep                                       # one chunk per query


@pytest.mark.gpu
def test_live_prover_is_untouched_gpu(gpulib):
    import circom_compat_amd as cc
    pk, mats, w = _chain16(cc)
    pr = cc.Prover(pk, mats, lib=gpulib)
    r, s = 1234567, 7654321
    before = pr.prove(r, s, w)
    rep = cc.check_key(pk, lib=gpulib)
    assert rep.ok
    bad = _clone(cc, pk)
    _plant(bad, "h_query", 77, "offcurve")
    assert not cc.check_key(bad, lib=gpulib).ok
    assert pr.prove(r, s, w).raw == before.raw
    pr.close()
