"""Phase-2 delta contributions on the GPU: cc.contribute_key (g16_key_contribute) and cc.check_contribution
(g16_key_contribution_check).

A contribution by d to the key of (tau, alpha, beta, gamma, delta) is, byte for byte, the key of
(tau, alpha, beta, gamma, delta * d): delta1, delta2 times d, every point of l_query and h_query times d^-1.
Expected bytes come from the oracle (oracle/bn254_ref.py: G1.mul, G2.mul, trapdoor_setup, g1_to_bytes) and, at
sizes where forming points in Python takes too long, from the library's own trapdoor generator, which
tests/test_kernels.py::test_trapdoor_setup_vs_oracle and tests/test_gpu_large.py pin to the oracle.  Expected
verdicts of the contribution check are the PLANTED changes."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R_MOD
UNCHANGED_MISMATCH, PAIR_DELTA, PAIR_L, PAIR_H, DELTA_INFINITE = 1, 2, 4, 8, 16
NONCANON, OFF_CURVE = 1, 2
CHUNK = 24            # G16_CONTRIB_CHUNK of the small cases: 62 = 24 + 24 + 14, 64 = 24 + 24 + 16 (ragged ends)
QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query")
D1 = 0x1D0C0FFEE0DDBA11F00D5EED0FACADE5C0DEC0DE1234567890ABCDEF13579BDF % R
D2 = (R - 1) // 3 * 2 + 12345


def _rho(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


def _clone(cc, pk):
    """a ProvingKey with its own writable copies of every array"""
    vk = cc.VerifyingKey(bytes(pk.vk.alpha_g1), bytes(pk.vk.beta_g2), bytes(pk.vk.gamma_g2), bytes(pk.vk.delta_g2),
                         np.array(pk.vk.gamma_abc_g1, dtype=np.uint8, copy=True))
    return cc.ProvingKey(pk.n_vars, pk.n_public, pk.domain_size, vk, bytes(pk.beta_g1), bytes(pk.delta_g1),
                         *(np.array(getattr(pk, q), dtype=np.uint8, copy=True) for q in QUERIES))


def _same_key(a, b):
    """every field of two ProvingKeys, as bytes"""
    assert (a.n_vars, a.n_public, a.domain_size) == (b.n_vars, b.n_public, b.domain_size)
    for name in ("beta_g1", "delta_g1"):
        assert bytes(getattr(a, name)) == bytes(getattr(b, name)), name
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert bytes(getattr(a.vk, name)) == bytes(getattr(b.vk, name)), name
    assert np.array_equal(np.asarray(a.vk.gamma_abc_g1), np.asarray(b.vk.gamma_abc_g1))
    for q in QUERIES:
        x, y = np.asarray(getattr(a, q)), np.asarray(getattr(b, q))
        assert x.shape == y.shape, q
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert bad.size == 0, (q, bad[:8])


def _untouched(new, old):
    """what a contribution leaves alone is shared with (or equal to) the parent"""
    for q in ("a_query", "b_g1_query", "b_g2_query"):
        assert getattr(new, q) is getattr(old, q)
    assert new.vk.gamma_abc_g1 is old.vk.gamma_abc_g1
    assert bytes(new.beta_g1) == bytes(old.beta_g1) and bytes(new.vk.alpha_g1) == bytes(old.vk.alpha_g1)
    assert bytes(new.vk.beta_g2) == bytes(old.vk.beta_g2) and bytes(new.vk.gamma_g2) == bytes(old.vk.gamma_g2)


def _chain_rows(k):
    cons, w, n_vars, n_pub = H.squaring_chain(k)
    return cons, w, n_vars, n_pub


def _csrs(cc, cons, lib):
    return tuple(cc.Csr.from_rows([[(cf, idx) for idx, cf in row[j]] for row in cons], lib) for j in range(3))


def _tox(seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(5)]


_keys = {}


def _chain_key(cc, lib, k=6, seed=707, scale=1, reduction="circom"):
    """cc.trapdoor_setup key of the squaring chain at 2^k with delta * scale (n_vars = 2^k, one public input)"""
    key = (id(lib), k, seed, scale, reduction)
    if key not in _keys:
        cons, _w, n_vars, n_pub = _chain_rows(k)
        tox = _tox(seed)
        tox[4] = tox[4] * scale % R
        _keys[key] = cc.trapdoor_setup(*_csrs(cc, cons, lib), n_vars, n_pub, tox, lib=lib, reduction=reduction)
    return _keys[key]


def _wide_circuit(m=20, n_pub=3, n_vars=40, seed=9):
    """m rows over n_vars wires with n_pub public inputs: domain 32 < 40 wires; every wire occurs"""
    rng = random.Random(seed)
    cons = []
    for i in range(m):
        lc = lambda k: [(w, rng.randrange(1, R)) for w in rng.sample(range(n_vars), k)]
        cons.append((lc(3) + [(i % n_vars, 1)], lc(2) + [((2 * i + 1) % n_vars, 5)], lc(2) + [((i + 20) % n_vars, 7)]))
    return cons, n_vars, n_pub


# ---- 1. oracle bytes -----------------------------------------------------------------------------
def test_oracle_bytes_reference_zkey(lib, golden):
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, mats = cc.read_zkey(data, lib=lib)
    opk, _ = o.read_zkey(data)
    new = cc.contribute_key(pk, D1, lib=lib)
    di = o.fr_inv(D1)
    assert new.l_query.shape == (2, 64) and new.h_query.shape == (4, 64)
    assert new.l_query.tobytes() == b"".join(o.g1_to_bytes(o.G1.mul(P, di)) for P in opk["l_query"])
    assert new.h_query.tobytes() == b"".join(o.g1_to_bytes(o.G1.mul(P, di)) for P in opk["h_query"])
    assert bytes(new.delta_g1) == o.g1_to_bytes(o.G1.mul(opk["delta_g1"], D1))
    assert bytes(new.vk.delta_g2) == o.g2_to_bytes(o.G2.mul(opk["delta_g2"], D1))
    _untouched(new, pk)
    # the parent is not written to
    pk2, _ = cc.read_zkey(data, lib=lib)
    _same_key(pk, pk2)
    assert cc.check_contribution(pk, new, lib=lib).ok


def test_write_zkey_takes_the_new_key(lib, golden, tmp_path):
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, mats = cc.read_zkey(data, lib=lib)
    new = cc.contribute_key(pk, D2, lib=lib)
    path = str(tmp_path / "next.zkey")
    cc.write_zkey(path, new, mats, lib=lib)
    back, _ = cc.read_zkey(path, lib=lib)
    _same_key(back, new)


# ---- 2. trapdoor equivalence, exact --------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_trapdoor_equivalence_oracle(lib, monkeypatch, reduction):
    """several public inputs, more wires (40) than domain points (32): contribute(key(delta), d) is the ORACLE's
    key(delta * d) in every field"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_CONTRIB_CHUNK", "13")
    cons, n_vars, n_pub = _wide_circuit()
    tox = _tox(21)
    pk = H.pk_from_oracle(o.trapdoor_setup(cons, n_vars, n_pub, *tox, reduction=reduction))
    assert pk.domain_size == 32 and pk.n_vars == 40 and len(pk.l_query) == 36
    want = H.pk_from_oracle(o.trapdoor_setup(cons, n_vars, n_pub, *tox[:4], tox[4] * D1 % R, reduction=reduction))
    new = cc.contribute_key(pk, D1, lib=lib)
    _same_key(new, want)
    _untouched(new, pk)
    if reduction == "libsnark":                                                      # the padding entry
        assert not new.h_query[-1].any() and not pk.h_query[-1].any()


@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_trapdoor_equivalence_generator(lib, reduction):
    """the same against the library's trapdoor generator at 2^6 .. 2^10 points"""
    import circom_compat_amd as cc
    for k in (6, 10):
        pk = _chain_key(cc, lib, k=k, reduction=reduction)
        want = _chain_key(cc, lib, k=k, scale=D2, reduction=reduction)
        assert bytes(pk.delta_g1) != bytes(want.delta_g1)
        _same_key(cc.contribute_key(pk, D2, lib=lib), want)


# ---- 3. composition ------------------------------------------------------------------------------
def test_composition_identity_chunks_aliasing(lib, monkeypatch):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    pk = _chain_key(cc, lib)
    assert len(pk.l_query) == 62 and len(pk.h_query) == 64
    monkeypatch.delenv("G16_CONTRIB_CHUNK", raising=False)
    one_shot = cc.contribute_key(pk, D1 * D2 % R, lib=lib)
    two = cc.contribute_key(cc.contribute_key(pk, D1, lib=lib), D2, lib=lib)
    _same_key(two, one_shot)
    _same_key(one_shot, _chain_key(cc, lib, scale=D1 * D2 % R))
    _same_key(cc.contribute_key(pk, 1, lib=lib), pk)
    # and back: d then d^-1
    _same_key(cc.contribute_key(cc.contribute_key(pk, D1, lib=lib), o.fr_inv(D1), lib=lib), pk)
    # ragged last chunks, one point per chunk, one chunk
    for chunk in (CHUNK, 1, 7, 64, 100000):
        monkeypatch.setenv("G16_CONTRIB_CHUNK", str(chunk))
        _same_key(cc.contribute_key(pk, D1 * D2 % R, lib=lib), one_shot)
    # outputs aliased to the inputs, through the C ABI
    for chunk in (CHUNK, None):
        if chunk is None:
            monkeypatch.delenv("G16_CONTRIB_CHUNK")
        mine = _clone(cc, pk)
        kd = mine.to_c()
        d = cc.fr_from_ints([D1 * D2 % R], lib)
        d1, d2 = (C.c_uint8 * 64)(), (C.c_uint8 * 128)()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        st = lib.g16_key_contribute(0, C.byref(kd), ptr(d), ptr(mine.l_query), ptr(mine.h_query), d1, d2)
        assert st == B.G16_OK
        assert np.array_equal(mine.l_query, one_shot.l_query) and np.array_equal(mine.h_query, one_shot.h_query)
        assert bytes(d1) == bytes(one_shot.delta_g1) and bytes(d2) == bytes(one_shot.vk.delta_g2)


# ---- 4. end to end -------------------------------------------------------------------------------
def _vk_dict(pk):
    vk = pk.vk
    return dict(alpha_g1=o.g1_from_bytes(bytes(vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(vk.beta_g2)),
                gamma_g2=o.g2_from_bytes(bytes(vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(vk.delta_g2)),
                ic=[o.g1_from_bytes(bytes(x)) for x in vk.gamma_abc_g1])


def test_end_to_end_proof_under_the_new_key(lib):
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub = _chain_rows(6)
    pk = _chain_key(cc, lib)
    new = cc.contribute_key(pk, D1, lib=lib)
    assert cc.check_key(new, lib=lib).ok
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    pr = cc.Prover(new, H.matrices_from_rows(a_rows, b_rows, 2, n_vars, lib), lib=lib)
    proof = H.proof_from_bytes(pr.prove(1234567, 7654321, w).raw)
    pr.close()
    assert o.verify_proof(_vk_dict(new), w[1:2], proof) is True
    assert o.verify_proof(_vk_dict(pk), w[1:2], proof) is False


# ---- 5. the contribution check -------------------------------------------------------------------
def _pair(cc, lib):
    base = _chain_key(cc, lib)
    return base, cc.contribute_key(base, D1, lib=lib)


def test_check_honest_and_changed(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_CONTRIB_CHUNK", str(CHUNK))
    base, new = _pair(cc, lib)
    rho = _rho(1, 62 + 64)
    rep = cc.check_contribution(base, new, rho=rho, lib=lib)
    assert rep.ok and rep.relations_checked and rep.relations_failed == 0 and rep.bad == []
    assert rep.n_bad == dict(l_query=0, h_query=0) and rep.describe() == "ok"
    assert cc.check_contribution(base, new, lib=lib) == cc.check_contribution(base, new, lib=lib) == rep
    # a key is not a contribution to itself under another delta, but it is one under d = 1
    assert cc.check_contribution(base, _clone(cc, base), rho=rho, lib=lib).ok
    other = o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE))

    def verdict(after, **kw):
        rep = cc.check_contribution(base, after, rho=rho, lib=lib, **kw)
        assert rep.relations_checked and rep.bad == [] and rep.n_bad == dict(l_query=0, h_query=0)
        assert rep.ok == (rep.relations_failed == 0)
        return rep.relations_failed

    for j in (0, CHUNK, 61):                                                         # L'_j: another valid point
        bad = _clone(cc, new)
        bad.l_query[j] = np.frombuffer(other, dtype=np.uint8)
        assert verdict(bad) == PAIR_L
    for j in (0, 2 * CHUNK - 1, 63):
        bad = _clone(cc, new)
        bad.h_query[j] = np.frombuffer(other, dtype=np.uint8)
        assert verdict(bad) == PAIR_H
    # delta_g2' from a different d: delta_g1' no longer matches it, and L, H were scaled by another factor
    bad = _clone(cc, new)
    bad.vk.delta_g2 = o.g2_to_bytes(o.G2.mul(o.g2_from_bytes(bytes(base.vk.delta_g2)), D2))
    assert verdict(bad) == PAIR_DELTA | PAIR_L | PAIR_H
    # both deltas from a different d: consistent with each other, not with L and H
    bad.delta_g1 = o.g1_to_bytes(o.G1.mul(o.g1_from_bytes(bytes(base.delta_g1)), D2))
    assert verdict(bad) == PAIR_L | PAIR_H
    # delta_g1' alone
    bad = _clone(cc, new)
    bad.delta_g1 = other
    assert verdict(bad) == PAIR_DELTA
    # something a contribution must not touch
    for q, i in (("a_query", 5), ("b_g1_query", 63), ("b_g2_query", 1)):
        bad = _clone(cc, new)
        getattr(bad, q)[i, 9] ^= 0x10
        assert verdict(bad) == UNCHANGED_MISMATCH
    bad = _clone(cc, new)
    bad.beta_g1 = other
    assert verdict(bad) == UNCHANGED_MISMATCH
    bad = _clone(cc, new)
    bad.vk.gamma_abc_g1[1, 3] ^= 1
    assert verdict(bad) == UNCHANGED_MISMATCH
    # delta at infinity (with L' and H' as they are)
    bad = _clone(cc, new)
    bad.delta_g1, bad.vk.delta_g2 = bytes(64), bytes(128)
    assert verdict(bad) & DELTA_INFINITE


def test_check_structural_faults_are_located(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_CONTRIB_CHUNK", str(CHUNK))
    base, new = _pair(cc, lib)

    def y_plus_1(raw):
        v = int.from_bytes(raw[32:64], "little") + 1
        assert v < o.Q_MOD
        return raw[:32] + v.to_bytes(32, "little")

    def plus_q(raw):
        v = int.from_bytes(raw[:32], "little") + o.Q_MOD
        assert v < 1 << 256
        return v.to_bytes(32, "little") + raw[32:]

    bad = _clone(cc, new)
    j = CHUNK + 3
    bad.l_query[j] = np.frombuffer(y_plus_1(bytes(bad.l_query[j])), dtype=np.uint8)
    rep = cc.check_contribution(base, bad, lib=lib)
    assert not rep.ok and rep.relations_checked is False and rep.relations_failed == 0
    assert rep.bad == [("l_query", j, OFF_CURVE)] and rep.n_bad == dict(l_query=1, h_query=0)
    assert "l_query[27]" in rep.describe() and "off the curve" in rep.describe()
    # several, over both queries and the single points, listed in (query, index) order
    bad.h_query[63] = np.frombuffer(plus_q(bytes(bad.h_query[63])), dtype=np.uint8)
    bad.h_query[0] = np.frombuffer(y_plus_1(bytes(bad.h_query[0])), dtype=np.uint8)
    bad.l_query[0] = np.frombuffer(plus_q(bytes(bad.l_query[0])), dtype=np.uint8)
    bad.delta_g1 = y_plus_1(bytes(bad.delta_g1))
    planted = [("l_query", 0, NONCANON), ("l_query", j, OFF_CURVE), ("h_query", 0, OFF_CURVE),
               ("h_query", 63, NONCANON), ("singles", 2, OFF_CURVE)]
    rep = cc.check_contribution(base, bad, lib=lib)
    assert rep.bad == planted and rep.n_bad == dict(l_query=2, h_query=2) and not rep.relations_checked
    assert cc.check_contribution(base, bad, lib=lib, max_listed=3).bad == planted[:3]
    rep0 = cc.check_contribution(base, bad, lib=lib, max_listed=0)
    assert rep0.bad == [] and rep0.n_bad == dict(l_query=2, h_query=2) and not rep0.ok
    # delta_g2' on the twist but outside G2
    from test_verify import _twist_point_outside_g2
    bad = _clone(cc, new)
    bad.vk.delta_g2 = o.g2_to_bytes(_twist_point_outside_g2(1))
    rep = cc.check_contribution(base, bad, lib=lib)
    assert rep.bad == [("singles", 4, 4)] and not rep.relations_checked


def test_check_coefficients_are_used(lib, monkeypatch):
    """against a KNOWN rho two entries of L' are moved so that they cancel in sum rho_i L'_i (L'_j + rho_k D,
    L'_k - rho_j D): the pair is accepted under exactly that rho and under no other"""
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_CONTRIB_CHUNK", str(CHUNK))
    base, new = _pair(cc, lib)
    rho = _rho(5, 62 + 64)
    j, k = 2, 60                                                                     # in different chunks
    assert j // CHUNK != k // CHUNK
    Dp = o.G1.mul(o.G1_GEN, 0xD15EA5E)
    forged = _clone(cc, new)
    lj = o.G1.add(o.g1_from_bytes(bytes(new.l_query[j])), o.G1.mul(Dp, rho[k]))
    lk = o.G1.sub(o.g1_from_bytes(bytes(new.l_query[k])), o.G1.mul(Dp, rho[j]))
    forged.l_query[j] = np.frombuffer(o.g1_to_bytes(lj), dtype=np.uint8)
    forged.l_query[k] = np.frombuffer(o.g1_to_bytes(lk), dtype=np.uint8)
    # the oracle's view: the two sums agree under rho, not under another
    s_new = o.G1.msm([o.g1_from_bytes(bytes(x)) for x in new.l_query], rho[:62])
    s_forged = o.G1.msm([o.g1_from_bytes(bytes(x)) for x in forged.l_query], rho[:62])
    assert s_new == s_forged
    rep = cc.check_contribution(base, forged, rho=rho, lib=lib)
    assert rep.ok and rep.relations_checked and rep.relations_failed == 0
    other = _rho(6, 62 + 64)
    assert o.G1.msm([o.g1_from_bytes(bytes(x)) for x in forged.l_query], other[:62]) != \
        o.G1.msm([o.g1_from_bytes(bytes(x)) for x in new.l_query], other[:62])
    assert cc.check_contribution(base, forged, rho=other, lib=lib).relations_failed == PAIR_L
    swapped = list(rho)
    swapped[j], swapped[k] = rho[k], rho[j]
    assert cc.check_contribution(base, forged, rho=swapped, lib=lib).relations_failed == PAIR_L
    assert cc.check_contribution(base, forged, lib=lib).relations_failed == PAIR_L   # drawn by the library
    # the same move in H, whose coefficients are the second part of rho
    forged = _clone(cc, new)
    hj = o.G1.add(o.g1_from_bytes(bytes(new.h_query[j])), o.G1.mul(Dp, rho[62 + k]))
    hk = o.G1.sub(o.g1_from_bytes(bytes(new.h_query[k])), o.G1.mul(Dp, rho[62 + j]))
    forged.h_query[j] = np.frombuffer(o.g1_to_bytes(hj), dtype=np.uint8)
    forged.h_query[k] = np.frombuffer(o.g1_to_bytes(hk), dtype=np.uint8)
    assert cc.check_contribution(base, forged, rho=rho, lib=lib).ok
    assert cc.check_contribution(base, forged, rho=other, lib=lib).relations_failed == PAIR_H


def test_check_pairings_against_the_oracle(lib, golden):
    """the relation itself on the reference key, with the oracle's pairing: e(S, delta2) = e(S', delta2')"""
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, _ = cc.read_zkey(data, lib=lib)
    new = cc.contribute_key(pk, D2, lib=lib)
    rho = _rho(7, 2 + 4)
    g1s = lambda arr: [o.g1_from_bytes(bytes(x)) for x in arr]
    d2, d2n = o.g2_from_bytes(bytes(pk.vk.delta_g2)), o.g2_from_bytes(bytes(new.vk.delta_g2))
    for before, after, r in ((pk.l_query, new.l_query, rho[:2]), (pk.h_query, new.h_query, rho[2:])):
        assert o.pairing(d2, o.G1.msm(g1s(before), r)) == o.pairing(d2n, o.G1.msm(g1s(after), r))
    assert o.pairing(o.G2_GEN, o.g1_from_bytes(bytes(new.delta_g1))) == o.pairing(d2n, o.G1_GEN)
    assert cc.check_contribution(pk, new, rho=rho, lib=lib).ok
    wrong = _clone(cc, new)
    wrong.h_query[1] = wrong.h_query[2]
    assert o.pairing(d2, o.G1.msm(g1s(pk.h_query), rho[2:])) != o.pairing(d2n, o.G1.msm(g1s(wrong.h_query), rho[2:]))
    assert cc.check_contribution(pk, wrong, rho=rho, lib=lib).relations_failed == PAIR_H


# ---- 6. edges --------------------------------------------------------------------------------------
def test_edges_arguments(lib):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    base, new = _pair(cc, lib)
    for bad_d in (0, R, R + 5, -1):
        with pytest.raises(cc.G16Error) as e:
            cc.contribute_key(base, bad_d, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    # the C ABI itself: d = 0, d = r and d = 2^256 - 1 as stored words
    kd = base.to_c()
    l_out, h_out = np.empty((62, 64), np.uint8), np.empty((64, 64), np.uint8)
    d1, d2 = (C.c_uint8 * 64)(), (C.c_uint8 * 128)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    words = lambda v: np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64).copy()
    for v in (0, R, R + 1, (1 << 256) - 1):
        assert lib.g16_key_contribute(0, C.byref(kd), ptr(words(v)), ptr(l_out), ptr(h_out), d1, d2) == B.G16_ERR_INVALID
    assert lib.g16_key_contribute(0, C.byref(kd), ptr(words(R - 1)), ptr(l_out), ptr(h_out), d1, d2) == B.G16_OK
    assert lib.g16_key_contribute(0, C.byref(kd), ptr(words(1)), None, ptr(h_out), d1, d2) == B.G16_ERR_INVALID
    assert lib.g16_key_contribute(0, None, ptr(words(1)), ptr(l_out), ptr(h_out), d1, d2) == B.G16_ERR_INVALID
    assert lib.g16_key_contribute(-1, C.byref(kd), ptr(words(1)), ptr(l_out), ptr(h_out), d1, d2) == B.G16_ERR_INVALID
    # rho: a zero entry, wrong lengths, out of range
    n = 62 + 64
    for bad_rho in ([5] * (n - 1) + [0], [0] + [5] * (n - 1), [5] * (n - 1), [5] * (n + 1), [5] * (n - 1) + [1 << 128]):
        with pytest.raises(cc.G16Error) as e:
            cc.check_contribution(base, new, rho=bad_rho, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    ka = new.to_c()
    rep = B.ContributionReportC()
    rho = np.array([[5, 0]] * n, dtype=np.uint64)
    rho[62] = 0                                                                      # H's first coefficient
    assert lib.g16_key_contribution_check(0, C.byref(kd), C.byref(ka), ptr(rho), None, 0, C.byref(rep)) == B.G16_ERR_INVALID
    rho[62, 1] = 1                                                                   # 2^64: non-zero in the high word only
    assert lib.g16_key_contribution_check(0, C.byref(kd), C.byref(ka), ptr(rho), None, 0, C.byref(rep)) == B.G16_OK
    assert rep.ok == 1 and rep.relations_checked == 1 and rep.n_listed == 0
    assert lib.g16_key_contribution_check(0, C.byref(kd), C.byref(ka), ptr(rho), None, 4, C.byref(rep)) == B.G16_ERR_INVALID
    assert lib.g16_key_contribution_check(0, C.byref(kd), None, None, None, 0, C.byref(rep)) == B.G16_ERR_INVALID
    assert lib.g16_key_contribution_check(0, C.byref(kd), C.byref(ka), None, None, 0, None) == B.G16_ERR_INVALID
    # keys of different sizes
    small = _chain_key(cc, lib, k=6, seed=708)
    big = _chain_key(cc, lib, k=10)
    rep = cc.check_contribution(small, big, lib=lib)
    assert not rep.ok and not rep.relations_checked and rep.relations_failed == UNCHANGED_MISMATCH


def test_edges_infinity_and_empty_l(lib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_CONTRIB_CHUNK", str(CHUNK))
    base = _clone(cc, _chain_key(cc, lib))
    for q, idx in (("l_query", (0, 23, 24, 61)), ("h_query", (5, 47, 63))):
        for i in idx:
            getattr(base, q)[i] = 0
    new = cc.contribute_key(base, D1, lib=lib)
    ref = cc.contribute_key(_chain_key(cc, lib), D1, lib=lib)
    for q, idx in (("l_query", (0, 23, 24, 61)), ("h_query", (5, 47, 63))):
        arr = getattr(new, q)
        for i in range(len(arr)):
            if i in idx:
                assert not arr[i].any(), (q, i)
            else:
                assert np.array_equal(arr[i], getattr(ref, q)[i]), (q, i)
    rep = cc.check_contribution(base, new, lib=lib)
    assert rep.ok and rep.n_bad == dict(l_query=0, h_query=0)
    # the libsnark H query ends in the point at infinity
    lk = _chain_key(cc, lib, reduction="libsnark")
    assert not lk.h_query[-1].any()
    assert cc.check_contribution(lk, cc.contribute_key(lk, D2, lib=lib), lib=lib).ok
    # no private wire at all: n_vars == n_public + 1, an empty l_query
    cons = [([(1, 1)], [(2, 1)], [(3, 1)]), ([(2, 1)], [(3, 1)], [(1, 1)])]
    tox = _tox(33)
    pk = H.pk_from_oracle(o.trapdoor_setup(cons, 4, 3, *tox))
    assert pk.l_query.shape == (0, 64)
    new = cc.contribute_key(pk, D1, lib=lib)
    _same_key(new, H.pk_from_oracle(o.trapdoor_setup(cons, 4, 3, *tox[:4], tox[4] * D1 % R)))
    assert new.l_query.shape == (0, 64)
    assert cc.check_contribution(pk, new, lib=lib).ok
    assert cc.check_contribution(pk, new, rho=_rho(3, pk.domain_size), lib=lib).ok
    wrong = _clone(cc, new)
    wrong.h_query[0] = wrong.h_query[1]
    assert cc.check_contribution(pk, wrong, lib=lib).relations_failed == PAIR_H


def test_edges_random_d(lib):
    import circom_compat_amd as cc
    base = _chain_key(cc, lib)
    a = cc.contribute_key(base, lib=lib)
    b = cc.contribute_key(base, None, lib=lib)
    for new in (a, b):
        assert bytes(new.delta_g1) != bytes(base.delta_g1) and bytes(new.vk.delta_g2) != bytes(base.vk.delta_g2)
        assert cc.check_contribution(base, new, lib=lib).ok
        _untouched(new, base)
    assert bytes(a.delta_g1) != bytes(b.delta_g1) and bytes(a.vk.delta_g2) != bytes(b.vk.delta_g2)
    assert not np.array_equal(a.l_query, b.l_query) and not np.array_equal(a.h_query, b.h_query)
    # b is a contribution to a as well (by d_b / d_a)
    assert cc.check_contribution(a, b, lib=lib).ok


# ---- 7. GPU only -----------------------------------------------------------------------------------
def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


_gpu_key = {}


def _chain16(cc, scale=1, reduction="circom"):
    """the 2^16 chain key of tests/test_key_check.py (same circuit, same toxic waste) with delta * scale"""
    key = (scale, reduction)
    if key not in _gpu_key:
        bench = _bench()
        mats, (A, Bm, Cm), w, n_vars = bench.chain_circuit(cc, 16)
        rng = random.Random(1616)
        tox = [rng.randrange(1, R) for _ in range(5)]
        tox[4] = tox[4] * scale % R
        _gpu_key[key] = (cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, tox, reduction=reduction), mats, w)
    return _gpu_key[key]


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_trapdoor_equivalence_2_16_gpu(gpulib, monkeypatch, reduction):
    import circom_compat_amd as cc
    pk = _chain16(cc, reduction=reduction)[0]
    want = _chain16(cc, scale=D1, reduction=reduction)[0]
    new = cc.contribute_key(pk, D1, lib=gpulib)
    _same_key(new, want)
    monkeypatch.setenv("G16_CONTRIB_CHUNK", str(10007))                              # 7 chunks, ragged
    _same_key(cc.contribute_key(pk, D1, lib=gpulib), want)
    rep = cc.check_contribution(pk, new, lib=gpulib)
    assert rep.ok and rep.relations_checked
    assert rep == cc.check_contribution(pk, new, rho=_rho(16, 2 * (1 << 16) - 2), lib=gpulib)


@pytest.mark.gpu
def test_check_2_16_planted_gpu(gpulib, monkeypatch):
    import circom_compat_amd as cc
    monkeypatch.setenv("G16_CONTRIB_CHUNK", str(1 << 14))
    pk = _chain16(cc)[0]
    new = cc.contribute_key(pk, D2, lib=gpulib)
    assert cc.check_key(new, lib=gpulib).ok
    other = np.frombuffer(o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE)), dtype=np.uint8)
    bad = _clone(cc, new)
    bad.l_query[(1 << 16) - 3] = other
    assert cc.check_contribution(pk, bad, lib=gpulib).relations_failed == PAIR_L
    bad = _clone(cc, new)
    bad.h_query[3 << 14] = other
    assert cc.check_contribution(pk, bad, lib=gpulib).relations_failed == PAIR_H
    raw = bytes(bad.h_query[77])
    bad.h_query[77] = np.frombuffer(raw[:32] + (int.from_bytes(raw[32:], "little") + 1).to_bytes(32, "little"), dtype=np.uint8)
    rep = cc.check_contribution(pk, bad, lib=gpulib)
    assert rep.bad == [("h_query", 77, OFF_CURVE)] and not rep.relations_checked
    monkeypatch.delenv("G16_CONTRIB_CHUNK")
    assert cc.check_contribution(pk, bad, lib=gpulib) == rep


@pytest.mark.gpu
def test_live_prover_is_untouched_gpu(gpulib):
    import circom_compat_amd as cc
    pk, mats, w = _chain16(cc)
    pr = cc.Prover(pk, mats, lib=gpulib)
    r, s = 1234567, 7654321
    before = pr.prove(r, s, w)
    new = cc.contribute_key(pk, lib=gpulib)
    assert cc.check_contribution(pk, new, lib=gpulib).ok
    assert pr.prove(r, s, w).raw == before.raw
    # and the new key proves: accepted under its own verifying key, rejected under the parent's
    pr2 = cc.Prover(new, mats, lib=gpulib)
    p2 = pr2.prove(r, s, w)
    assert cc.verify_batch(new.vk, [p2], [w[1:2]], lib=gpulib) == [True]
    assert cc.verify_batch(pk.vk, [p2], [w[1:2]], lib=gpulib) == [False]
    assert pr.prove(r, s, w).raw == before.raw
    pr.close()
    pr2.close()
