"""Verification under many keys in one pass (g16_verify_aggregate_keys / g16_verify_batch_keys and
cc.verify_aggregate_keys / cc.verify_batch_keys / cc.verify_batch_fast_keys).  A group is one key with the proofs
under it; every verdict must be what the single-key call gives on that group alone.  Expected verdicts come from
the oracle (o.verify_proof, and the combined equation as test_verify_aggregate._oracle_aggregate evaluates it)
for groups of at most 5 proofs; larger groups are compared with the single-key calls cc.verify_aggregate /
cc.verify_batch on a planted wrong input.  The single-key calls are the one-group case of the same device code, so
at that size the oracle-checked small groups and the planted input carry the meaning, not the comparison."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_verify import _vk
from test_verify_aggregate import BIG, BLOCK, _malformed_batch, _oracle_aggregate, _rho, _test_zkey_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = o.R_MOD

_cache = {}
_oracle = {}


def _trapdoor_batch(lib, n_pub):
    """(vk, opk, 3 proofs, their public inputs) under a trapdoor key of the 3-row squaring chain with n_pub
    public inputs, as test_aggregate_public_input_counts makes them; cached per session"""
    import circom_compat_amd as cc
    key = (id(lib), n_pub)
    if key not in _cache:
        m = 3
        base = 1 + n_pub
        n_vars = base + m + 1
        cons = [([(base + i, 1)], [(base + i, 1)], [(base + i + 1, 1)]) for i in range(m)]
        rng = random.Random(100 + n_pub)
        tox = [rng.randrange(1, P) for _ in range(5)]
        opk = o.trapdoor_setup(cons, n_vars, n_pub, *tox)
        a_rows, b_rows = o.matrices_from_r1cs(cons)
        mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
        pr = cc.Prover(H.pk_from_oracle(opk), mats, lib=lib)
        raws, pubs = [], []
        for k in range(3):
            w = [1] + [rng.randrange(P) for _ in range(n_pub)] + [3 + k]
            for _ in range(m):
                w.append(w[-1] * w[-1] % P)
            raws.append(pr.prove(rng.randrange(P), rng.randrange(P), w).raw)
            pubs.append(w[1:1 + n_pub])
        pr.close()
        _cache[key] = (_vk(cc, opk), opk, raws, pubs)
    return _cache[key]


class G:
    """one group and what the checks need of it"""

    def __init__(self, src, n=None, start=0):
        vk, opk, raws, pubs = src[:4]
        n = len(raws) - start if n is None else n
        self.vk, self.opk = vk, opk
        self.raws, self.pubs = list(raws[start:start + n]), [list(p) for p in pubs[start:start + n]]

    def arg(self):
        return (self.vk, self.raws, self.pubs)

    def with_bad_input(self, i):
        g = G((self.vk, self.opk, self.raws, self.pubs))
        g.pubs[i][0] = (g.pubs[i][0] + 1) % P
        return g

    def _memo(self, rho, compute):
        key = (bytes(self.vk.delta_g2), bytes(self.vk.gamma_g2), len(self.vk.gamma_abc_g1), tuple(self.raws),
               tuple(map(tuple, self.pubs)), rho and tuple(rho))
        if key not in _oracle:                                                       # shared by the emulator and the GPU leg
            _oracle[key] = compute()
        return _oracle[key]

    def oracle_aggregate(self, rho):
        """the combined equation over this group alone, on the CPU (each distinct question is evaluated once)"""
        assert len(self.raws) <= 5
        if not self.raws:
            return True
        return self._memo(rho, lambda: bool(_oracle_aggregate(self.opk, self.raws, self.pubs, rho)))

    def oracle_each(self):
        assert len(self.raws) <= 5
        return list(self._memo(None, lambda: [bool(o.verify_proof(self.opk, p, H.proof_from_bytes(r)))
                                              for r, p in zip(self.raws, self.pubs)]))


def _rhos(seed, groups):
    return [_rho(seed + 1000 * k, len(g.raws)) for k, g in enumerate(groups)]


def _agg_keys(cc, lib, groups, rho, **kw):
    return cc.verify_aggregate_keys([g.arg() for g in groups], rho=rho, lib=lib, **kw)


def _agg_single(cc, lib, groups, rho):
    return [cc.verify_aggregate(g.vk, g.raws, g.pubs, rho=r, lib=lib) for g, r in zip(groups, rho)]


def _batch_single(cc, lib, groups):
    return [cc.verify_batch(g.vk, g.raws, g.pubs, lib=lib) for g in groups]


# ---- 1. one key -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, BIG])
def test_one_key_equals_the_single_key_calls(lib, golden, n):
    import circom_compat_amd as cc
    good = G(_test_zkey_batch(lib, golden, n))
    bad = good.with_bad_input(n - 1)
    rho = _rhos(n, [good])
    for g, want in ((good, True), (bad, False)):
        if n <= 5:
            assert g.oracle_aggregate(rho[0]) is want
        assert _agg_single(cc, lib, [g], rho) == [want]
        assert _agg_keys(cc, lib, [g], rho) == [want]
    want = [True] * (n - 1) + [False]
    if n <= 5:
        assert bad.oracle_each() == want
    assert _batch_single(cc, lib, [bad]) == [want]
    assert cc.verify_batch_keys([bad.arg()], lib=lib) == [want]


# ---- 2. ragged groups, different numbers of public inputs ----------------------------------------
def _ragged(lib, golden):
    return [G(_test_zkey_batch(lib, golden, 5), 3), G(_trapdoor_batch(lib, 0), 0), G(_trapdoor_batch(lib, 3), 2)]


def test_ragged_groups_with_different_input_counts(lib, golden):
    import circom_compat_amd as cc
    groups = _ragged(lib, golden)
    assert [len(g.raws) for g in groups] == [3, 0, 2]
    assert [len(g.vk.gamma_abc_g1) - 1 for g in groups] == [1, 0, 3]
    rho = _rhos(2, groups)
    for flip, want in ((None, [True, True, True]), ((0, 2), [False, True, True]), ((2, 0), [True, True, False])):
        gs = list(groups)
        if flip:
            gs[flip[0]] = gs[flip[0]].with_bad_input(flip[1])
        assert [g.oracle_aggregate(r) for g, r in zip(gs, rho)] == want
        assert _agg_single(cc, lib, gs, rho) == want
        assert _agg_keys(cc, lib, gs, rho) == want
        each = [g.oracle_each() for g in gs]
        assert [all(e) for e in each] == want
        assert _batch_single(cc, lib, gs) == each
        assert cc.verify_batch_keys([g.arg() for g in gs], lib=lib) == each


# ---- 3. group boundaries and block boundaries -------------------------------------------------------
def _boundary_groups(lib, golden):
    """counts (3, 67, 2): group 1 spans two blocks; in a layout that packed proofs densely groups 0 and 2 would
    share its blocks"""
    return [G(_trapdoor_batch(lib, 3), 3), G(_test_zkey_batch(lib, golden, BIG)), G(_trapdoor_batch(lib, 3), 2, 1)]


@pytest.mark.parametrize("where", [None, (1, 0), (1, BLOCK - 1), (1, BLOCK), (1, BIG - 1), (0, 2), (2, 0)])
def test_boundaries(lib, golden, where):
    import circom_compat_amd as cc
    gs = _boundary_groups(lib, golden)
    assert [len(g.raws) for g in gs] == [3, BIG, 2]
    rho = _rhos(3, gs)
    want = [True, True, True]
    if where:
        gs[where[0]] = gs[where[0]].with_bad_input(where[1])
        want[where[0]] = False
    assert [gs[0].oracle_aggregate(rho[0]), gs[2].oracle_aggregate(rho[2])] == [want[0], want[2]]
    assert cc.verify_aggregate(gs[1].vk, gs[1].raws, gs[1].pubs, rho=rho[1], lib=lib) is want[1]
    ok, structural = _agg_keys(cc, lib, gs, rho, return_structural=True)
    assert ok == want
    assert structural == [[True] * 3, [True] * BIG, [True] * 2]


def test_boundaries_per_proof(lib, golden):
    import circom_compat_amd as cc
    gs = _boundary_groups(lib, golden)
    gs[0] = gs[0].with_bad_input(2)
    gs[1] = gs[1].with_bad_input(BLOCK - 1).with_bad_input(BLOCK)
    gs[2] = gs[2].with_bad_input(0)
    want = [[True, True, False], [i not in (BLOCK - 1, BLOCK) for i in range(BIG)], [False, True]]
    assert [gs[0].oracle_each(), gs[2].oracle_each()] == [want[0], want[2]]
    assert cc.verify_batch(gs[1].vk, gs[1].raws, gs[1].pubs, lib=lib) == want[1]
    assert cc.verify_batch_keys([g.arg() for g in gs], lib=lib) == want


# ---- 4. more groups than one block of key-side lanes --------------------------------------------
def _many_groups(lib, golden, n=BLOCK + 2):
    src = [_test_zkey_batch(lib, golden, 5), _trapdoor_batch(lib, 0), _trapdoor_batch(lib, 3)]
    return [G(src[k % 3], 1, (k // 3) % 3) for k in range(n)]


@pytest.mark.parametrize("bad", [None, 0, BLOCK - 1, BLOCK, BLOCK + 1])
def test_more_groups_than_lanes_in_a_block(lib, golden, bad):
    import circom_compat_amd as cc
    gs = _many_groups(lib, golden)
    assert len(gs) == 66
    rho = _rhos(4, gs)
    want = [True] * len(gs)
    if bad is not None:
        # groups 0, 63 and 65 are under keys with public inputs; group 64's key has none: the proof of another
        # witness's group is wrong there as well (its C belongs to other randomness, its A and B too)
        if len(gs[bad].pubs[0]):
            gs[bad] = gs[bad].with_bad_input(0)
        else:
            gs[bad].raws[0] = gs[bad].raws[0][:192] + o.g1_to_bytes(o.G1_GEN)
        want[bad] = False
        assert gs[bad].oracle_aggregate(rho[bad]) is False
        assert gs[bad].oracle_each() == [False]
    else:
        assert all(gs[k].oracle_each() == [True] for k in range(3))
    assert _agg_keys(cc, lib, gs, rho) == want
    if bad in (None, BLOCK):
        assert cc.verify_batch_keys([g.arg() for g in gs], lib=lib) == [[v] for v in want]


# ---- 5. sums do not cross groups ----------------------------------------------------------------------
def test_sums_do_not_cross_groups(lib, golden):
    """the forged pair of test_aggregate_coefficients_are_used: as ONE group it passes under exactly the rho it
    was made for; split over two groups of the same key, with the same rho, both groups fail"""
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 2)
    rho = _rho(31, 2)
    D = o.G1.mul(o.G1_GEN, 0xD15EA5E)
    c0 = o.G1.add(o.g1_from_bytes(raws[0][192:]), o.G1.mul(D, rho[1]))
    c1 = o.G1.add(o.g1_from_bytes(raws[1][192:]), o.G1.neg(o.G1.mul(D, rho[0])))
    forged = [raws[0][:192] + o.g1_to_bytes(c0), raws[1][:192] + o.g1_to_bytes(c1)]
    pair = G((vk, opk, forged, pubs))
    swapped = [rho[1], rho[0]]
    assert pair.oracle_aggregate(rho) is True and pair.oracle_aggregate(swapped) is False
    assert _agg_keys(cc, lib, [pair], [rho]) == [True]
    assert _agg_keys(cc, lib, [pair], [swapped]) == [False]
    halves = [G((vk, opk, forged, pubs), 1, 0), G((vk, opk, forged, pubs), 1, 1)]
    assert [h.oracle_aggregate([r]) for h, r in zip(halves, rho)] == [False, False]
    assert _agg_keys(cc, lib, halves, [[rho[0]], [rho[1]]]) == [False, False]
    # and beside each other in one call: the pair as a group, then its halves
    assert _agg_keys(cc, lib, [pair] + halves, [rho, [rho[0]], [rho[1]]]) == [True, False, False]


# ---- 6. structural ----------------------------------------------------------------------------------
def test_structural_rejects_between_valid_groups(lib, golden):
    import circom_compat_amd as cc
    vk, opk, batch, bpubs, where = _malformed_batch(lib, golden)
    gs = [G(_trapdoor_batch(lib, 3)), G((vk, opk, batch, bpubs)), G(_trapdoor_batch(lib, 0), 2)]
    rho = _rhos(6, gs)
    ok, structural = _agg_keys(cc, lib, gs, rho, return_structural=True)
    assert ok == [True, False, True]
    single = cc.verify_aggregate(vk, batch, bpubs, rho=rho[1], lib=lib, return_structural=True)
    assert single == (False, [i not in where for i in range(14)])
    assert structural == [[True] * 3, single[1], [True] * 2]
    # the raw ABI: the flags of group 1 sit at the global offsets 3 .. 16
    vks, counts, buf, pubs, keep = cc._verify_groups_args([g.arg() for g in gs], lib)
    flat = np.full(19, 7, dtype=np.uint8)
    oks = np.full(3, 7, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.g16_verify_aggregate_keys(0, vks, ptr(counts), 3, ptr(buf), ptr(pubs), None, ptr(oks), ptr(flat)) == 0
    assert list(oks) == [1, 0, 1]
    assert list(flat) == [1] * 3 + [int(i not in where) for i in range(14)] + [1] * 2
    want = _batch_single(cc, lib, gs)
    assert want == [[True] * 3, [i not in where for i in range(14)], [True] * 2]
    assert cc.verify_batch_keys([g.arg() for g in gs], lib=lib) == want
    assert cc.verify_batch_fast_keys([g.arg() for g in gs], lib=lib) == want


def test_single_key_structural_out_matches_groups(lib, golden):
    """structural_out of the single-key call at the C ABI is the flat structural array of the one-group call"""
    import circom_compat_amd as cc
    vk, opk, batch, bpubs, where = _malformed_batch(lib, golden)
    n = 5
    want = [i not in where for i in range(n)]
    assert True in want and False in want
    g = G((vk, opk, batch, bpubs), n)
    rho = _rhos(9, [g])
    d, buf, pb, cnt, _ic = cc._verify_args(g.vk, g.raws, g.pubs, lib)
    assert cnt == n
    rho_arr = cc._rho_array(rho[0], n, "one coefficient per proof")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = np.full(1, 7, dtype=np.uint8)
    flat = np.full(n + 1, 7, dtype=np.uint8)
    assert lib.g16_verify_aggregate(0, C.byref(d), ptr(buf), ptr(pb), n, ptr(rho_arr), ptr(ok), ptr(flat)) == 0
    assert list(ok) == [0] and flat[n] == 7                                          # n bytes, no more
    assert [bool(x) for x in flat[:n]] == want
    assert _agg_keys(cc, lib, [g], rho, return_structural=True) == ([False], [want])


def test_batch_fast_keys_makes_at_most_two_library_calls(lib, golden):
    """one aggregate pass; then one per-proof pass over the well-formed proofs of the rejected groups only"""
    import circom_compat_amd as cc
    gs = _ragged(lib, golden) + [G(_trapdoor_batch(lib, 3)).with_bad_input(1)]
    gs[0] = gs[0].with_bad_input(0)
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("g16_verify"):
                return fn

            def wrapped(*a):                                                         # (entry point, proofs it was given)
                n = a[4] if not name.endswith("_keys") else \
                    int(np.ctypeslib.as_array(C.cast(a[2], C.POINTER(C.c_uint32)), (a[3],)).sum())
                calls.append((name, n))
                return fn(*a)
            return wrapped
    want = [[False, True, True], [], [True, True], [True, False, True]]
    assert [g.oracle_each() for g in gs] == want
    assert cc.verify_batch_fast_keys([g.arg() for g in gs], lib=Spy()) == want
    assert calls == [("g16_verify_aggregate_keys", 8), ("g16_verify_batch_keys", 6)]
    del calls[:]
    gs = _ragged(lib, golden)
    assert cc.verify_batch_fast_keys([g.arg() for g in gs], lib=Spy()) == [[True] * 3, [], [True] * 2]
    assert calls == [("g16_verify_aggregate_keys", 5)]


# ---- 7. edges -----------------------------------------------------------------------------------------
def test_edges(lib, golden):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    gs = _ragged(lib, golden)
    args = [g.arg() for g in gs]
    # no groups; only empty groups
    assert cc.verify_aggregate_keys([], lib=lib) == []
    assert cc.verify_aggregate_keys([], rho=[], lib=lib, return_structural=True) == ([], [])
    assert cc.verify_batch_keys([], lib=lib) == [] and cc.verify_batch_fast_keys([], lib=lib) == []
    empty = [(g.vk, [], []) for g in gs]
    assert cc.verify_aggregate_keys(empty, lib=lib) == [True] * 3
    assert cc.verify_aggregate_keys(empty, rho=[[], [], []], lib=lib, return_structural=True) == ([True] * 3, [[], [], []])
    assert cc.verify_batch_keys(empty, lib=lib) == [[], [], []] and cc.verify_batch_fast_keys(empty, lib=lib) == [[], [], []]
    # the all-infinity proof as a group of one: whatever verify_batch (and the oracle) say about it
    inf = bytes(256)
    want = cc.verify_batch(gs[0].vk, [inf], [gs[0].pubs[0]], lib=lib)[0]
    assert want == bool(o.verify_proof(gs[0].opk, gs[0].pubs[0], H.proof_from_bytes(inf)))
    one = [(gs[0].vk, [inf], [gs[0].pubs[0]])]
    assert cc.verify_aggregate_keys(one, rho=[[12345]], lib=lib, return_structural=True) == ([want], [[True]])
    assert cc.verify_batch_keys(one, lib=lib) == [[want]]
    # what Python refuses
    for rho in ([[1, 2, 3], [], [0, 5]], [[1, 2, 3], [], [5, 1 << 128]], [[1, 2, 3], [], [5, -1]], [[1, 2, 3], []],
                [[1, 2, 3], [], [5]], [[1, 2, 3], [4], [5, 6]], [[1, 2, 3], [], [5, 6], []]):
        with pytest.raises(cc.G16Error) as e:
            cc.verify_aggregate_keys(args, rho=rho, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID, rho
    short = list(args)
    short[2] = (gs[2].vk, gs[2].raws, [gs[2].pubs[0], gs[2].pubs[1][:2]])       # a wrong input count in one group
    for fn in (cc.verify_aggregate_keys, cc.verify_batch_keys, cc.verify_batch_fast_keys):
        with pytest.raises(cc.G16Error) as e:
            fn(short, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
        with pytest.raises(cc.G16Error) as e:
            fn([args[0], args[1], (gs[2].vk, gs[2].raws, gs[2].pubs[:1])], lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    # the C ABI itself: a zero coefficient in the SECOND non-empty group, NULLs, and no groups at all
    vks, counts, buf, pubs, keep = cc._verify_groups_args(args, lib)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rho = np.array([[5, 0], [6, 0], [7, 0], [8, 0], [0, 0]], dtype=np.uint64)
    ok = np.full(3, 7, dtype=np.uint8)
    call = lambda *a: lib.g16_verify_aggregate_keys(0, *a)
    assert call(vks, ptr(counts), 3, ptr(buf), ptr(pubs), ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    assert list(ok) == [7, 7, 7]
    rho[4, 1] = 1                                                                # 2^64: non-zero in the high word only
    assert call(vks, ptr(counts), 3, ptr(buf), ptr(pubs), ptr(rho), ptr(ok), None) == B.G16_OK
    assert list(ok) == [1, 1, 1]
    ok[:] = 7
    assert call(None, ptr(counts), 3, ptr(buf), ptr(pubs), ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    assert call(vks, None, 3, ptr(buf), ptr(pubs), ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    assert call(vks, ptr(counts), 3, None, ptr(pubs), ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    assert call(vks, ptr(counts), 3, ptr(buf), None, ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    assert call(vks, ptr(counts), 3, ptr(buf), ptr(pubs), ptr(rho), None, None) == B.G16_ERR_INVALID
    holed = (C.POINTER(B.VkDesc) * 3)(vks[0], None, vks[2])
    assert call(holed, ptr(counts), 3, ptr(buf), ptr(pubs), ptr(rho), ptr(ok), None) == B.G16_ERR_INVALID
    assert lib.g16_verify_batch_keys(0, holed, ptr(counts), 3, ptr(buf), ptr(pubs), ptr(ok)) == B.G16_ERR_INVALID
    assert lib.g16_verify_batch_keys(0, vks, ptr(counts), 3, ptr(buf), ptr(pubs), None) == B.G16_ERR_INVALID
    assert call(None, None, 0, None, None, None, None, None) == B.G16_OK            # n_keys = 0: nothing is written
    assert lib.g16_verify_batch_keys(0, None, None, 0, None, None, None) == B.G16_OK
    assert list(ok) == [7, 7, 7]


def test_drawn_coefficients(lib, golden):
    """rho = None: drawn by the library; valid groups are accepted, the bad one is rejected"""
    import circom_compat_amd as cc
    gs = _ragged(lib, golden)
    assert cc.verify_aggregate_keys([g.arg() for g in gs], lib=lib) == [True, True, True]
    gs[2] = gs[2].with_bad_input(1)
    assert gs[2].oracle_each() == [True, False]
    assert cc.verify_aggregate_keys([g.arg() for g in gs], lib=lib) == [True, True, False]


# ---- 8. determinism -----------------------------------------------------------------------------------
def test_keys_calls_are_deterministic(lib, golden):
    import circom_compat_amd as cc
    gs = _ragged(lib, golden) + [G(_trapdoor_batch(lib, 3)).with_bad_input(2)]
    rho = _rhos(8, gs)
    assert [g.oracle_aggregate(r) for g, r in zip(gs, rho)] == [True, True, True, False]
    first = _agg_keys(cc, lib, gs, rho, return_structural=True)
    assert first == ([True, True, True, False], [[True] * 3, [], [True] * 2, [True] * 3])
    assert _agg_keys(cc, lib, gs, rho, return_structural=True) == first
    each = cc.verify_batch_keys([g.arg() for g in gs], lib=lib)
    assert each == [g.oracle_each() for g in gs]
    assert cc.verify_batch_keys([g.arg() for g in gs], lib=lib) == each


# ---- 9. the use the feature is for --------------------------------------------------------------------
@pytest.mark.gpu
def test_three_contributed_keys_after_prove_batch_gpu(gpulib):
    """three keys x 100 proofs from prove_batch on the 2^10 squaring chain; keys 1 and 2 are phase-2
    contributions to key 0 (the snarkjs situation: alpha, beta, gamma shared, delta differs).  One bad public
    input under the middle key: verify_batch_fast_keys names exactly that proof"""
    import circom_compat_amd as cc
    sys.path.insert(0, ROOT)
    import bench
    count = 100
    mats, (A, Bm, Cm), _, n_vars = bench.chain_circuit(cc, 10)
    m = n_vars - 2
    rng = random.Random(4343)
    pk0 = cc.trapdoor_setup(A, Bm, Cm, n_vars, 1, [rng.randrange(1, P) for _ in range(5)])
    pks = [pk0, cc.contribute_key(pk0, rng.randrange(1, P), lib=gpulib)]
    pks.append(cc.contribute_key(pks[1], rng.randrange(1, P), lib=gpulib))
    assert len({bytes(pk.vk.delta_g2) for pk in pks}) == 3 and len({bytes(pk.vk.gamma_g2) for pk in pks}) == 1
    groups = []
    for pk in pks:
        w_ints = []
        for _ in range(count):
            xs = [rng.randrange(2, P)]
            for _ in range(m):
                xs.append(xs[-1] * xs[-1] % P)
            w_ints.append([1, xs[m]] + xs[:m])
        rs = [(rng.randrange(P), rng.randrange(P)) for _ in range(count)]
        pr = cc.Prover(pk, mats, tables=0)
        proofs = pr.prove_batch(rs, np.stack([cc.fr_from_ints(w) for w in w_ints]))
        pr.close()
        groups.append((pk.vk, proofs, [[w[1]] for w in w_ints]))
    vk = groups[2][0]
    vk_dict = dict(alpha_g1=o.g1_from_bytes(bytes(vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(vk.beta_g2)),
                   gamma_g2=o.g2_from_bytes(bytes(vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(vk.delta_g2)),
                   ic=[o.g1_from_bytes(bytes(x)) for x in vk.gamma_abc_g1])
    assert o.verify_proof(vk_dict, groups[2][2][-1], H.proof_from_bytes(groups[2][1][-1].raw))
    assert cc.verify_aggregate_keys(groups, lib=gpulib) == [True, True, True]
    assert cc.verify_batch_fast_keys(groups, lib=gpulib) == [[True] * count] * 3
    bad = [list(p) for p in groups[1][2]]
    bad[50][0] = (bad[50][0] + 1) % P
    wrong = [groups[0], (groups[1][0], groups[1][1], bad), groups[2]]
    assert cc.verify_aggregate_keys(wrong, lib=gpulib) == [True, False, True]
    assert cc.verify_aggregate(groups[1][0], groups[1][1], bad, lib=gpulib) is False
    assert cc.verify_batch_fast_keys(wrong, lib=gpulib) == [[True] * count, [i != 50 for i in range(count)], [True] * count]
    # a proof under a sibling key is a proof under another delta: wrong
    crossed = [(groups[1][0], groups[0][1][:2], groups[0][2][:2]), (groups[0][0], groups[0][1][:2], groups[0][2][:2])]
    assert cc.verify_batch_keys(crossed, lib=gpulib) == [[False, False], [True, True]]
