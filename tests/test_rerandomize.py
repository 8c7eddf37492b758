"""Proof re-randomisation on the GPU (g16_proofs_rerandomize / _keys, cc.rerandomize / cc.rerandomize_keys,
Proof.rerandomize, Groth16.rerandomize_proof): for a proof (A, B, C) under a key with delta in G2,
  A' = r1^-1 A,  B' = r1 B + (r1 r2) delta,  C' = C + r2 A.
Expected bytes come from the oracle (oracle/bn254_ref.py: G1 / G2 mul, add, neg and the pairing check), never from
the library."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from circom_compat_amd import _binding as B
from test_verify import _twist_point_outside_g2, _vk
from test_verify_aggregate import _test_zkey_batch

R = o.R_MOD
REC = 256


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _want(raw, delta, r1, r2):
    """the three formulas on the CPU; delta as an oracle point (None = infinity)"""
    p = H.proof_from_bytes(raw)
    a = o.G1.mul(p["a"], pow(r1, R - 2, R))
    b = o.G2.add(o.G2.mul(p["b"], r1), o.G2.mul(delta, r1 * r2 % R))
    c = o.G1.add(p["c"], o.G1.mul(p["a"], r2))
    return o.g1_to_bytes(a) + o.g2_to_bytes(b) + o.g1_to_bytes(c)


def _scalars(seed, n):
    rng = random.Random(seed)
    return [(rng.randrange(1, R), rng.randrange(R)) for _ in range(n)]


def _batch(lib, golden, n):
    """the first n of ONE shared batch of 5 valid proofs of test.zkey: (vk, oracle key, proof bytes, public inputs)"""
    vk, opk, raws, pubs = _test_zkey_batch(lib, golden, 5)
    return vk, opk, raws[:n], pubs[:n]


def _raws(proofs):
    return [p.raw for p in proofs]


def _call(lib, delta, raws, scalars, n=None, out=None, ok=None, device=0):
    """the C ABI as it is: returns (status, out array, ok array); out / ok are 0xA5-filled unless given"""
    n = len(raws) if n is None else n
    buf = np.frombuffer(b"".join(raws), dtype=np.uint8).copy() if raws else np.zeros(1, np.uint8)
    out = np.full(max(n, 1) * REC, 0xA5, np.uint8) if out is None else out
    ok = np.full(max(n, 1), 0xA5, np.uint8) if ok is None else ok
    sc = H.fr_mont_arr([x for pair in scalars for x in pair]) if scalars is not None else None
    st = lib.g16_proofs_rerandomize(device, delta, ptr(buf), n, ptr(sc) if sc is not None else None, ptr(out), ptr(ok))
    return st, out, ok


# ---- 1. oracle bytes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
def test_valid_proofs_match_the_oracle_and_verify(lib, golden, n):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, n)
    sc = _scalars(100 + n, n)
    before = list(raws)
    got, ok = cc.rerandomize(vk, raws, sc, lib=lib, return_ok=True)
    assert ok == [True] * n
    assert raws == before                                              # the input is not written
    for g, raw, (r1, r2), pub in zip(got, raws, sc, pubs):
        assert g.raw == _want(raw, opk["delta_g2"], r1, r2)
        assert g.raw != raw
        assert o.verify_proof(opk, pub, H.proof_from_bytes(g.raw))
        assert not o.verify_proof(opk, [(pub[0] + 1) % R], H.proof_from_bytes(g.raw))
    assert cc.verify_batch(vk, got, pubs, lib=lib) == [True] * n
    assert cc.verify_batch(vk, got, [[(p[0] + 1) % R] for p in pubs], lib=lib) == [False] * n
    # the other spellings: Proof objects in, 128 bytes of delta for the key, the single-proof forms
    assert cc.rerandomize(bytes(vk.delta_g2), [cc.Proof(r) for r in raws], sc, lib=lib) == got
    assert cc.Proof(raws[0]).rerandomize(vk, *sc[0], lib=lib) == got[0]
    rng = random.Random(5)
    want_rng = random.Random(5)
    pair = (want_rng.randrange(1, R), want_rng.randrange(R))
    assert cc.Groth16.rerandomize_proof(vk, cc.Proof(raws[0]), rng, lib=lib).raw == \
        _want(raws[0], opk["delta_g2"], *pair)


# ---- 2. invalid stays invalid ----------------------------------------------------------------------------------
def test_an_invalid_proof_stays_invalid(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 1)
    bad = raws[0][:192] + o.g1_to_bytes(o.G1.mul(o.G1_GEN, 12345))      # C is another curve point
    assert not o.verify_proof(opk, pubs[0], H.proof_from_bytes(bad))
    (got,), ok = cc.rerandomize(vk, [bad], [(7, 9)], lib=lib, return_ok=True)
    assert ok == [True]
    assert got.raw == _want(bad, opk["delta_g2"], 7, 9)
    assert not o.verify_proof(opk, pubs[0], H.proof_from_bytes(got.raw))
    assert cc.verify_batch(vk, [got], pubs, lib=lib) == [False]


# ---- 3. edge scalars -------------------------------------------------------------------------------------------
def test_edge_scalars(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 1)
    raw, delta = raws[0], opk["delta_g2"]
    p = H.proof_from_bytes(raw)
    big, pow200 = ((1 << 253) - 1) % R, 1 << 200
    sc = [(1, 0), (R - 1, 0), (1, R - 1), (big, pow200), (pow200, big)]
    got = _raws(cc.rerandomize(vk, [raw] * len(sc), sc, lib=lib))
    assert got[0] == raw
    assert got[1] == o.g1_to_bytes(o.G1.neg(p["a"])) + o.g2_to_bytes(o.G2.neg(p["b"])) + raw[192:]
    assert got[2] == raw[:64] + o.g2_to_bytes(o.G2.sub(p["b"], delta)) + o.g1_to_bytes(o.G1.sub(p["c"], p["a"]))
    assert got[3] == _want(raw, delta, big, pow200)
    assert got[4] == _want(raw, delta, pow200, big)
    assert cc.verify_batch(vk, got, pubs * len(sc), lib=lib) == [True] * len(sc)


# ---- 4. exceptional additions ----------------------------------------------------------------------------------
def test_exceptional_additions_beside_finite_neighbours(lib, golden):
    """B = +-delta, C = +-A and operands at infinity, each in a batch of 9 (one inversion run of 8 plus one) whose
    other members are ordinary proofs"""
    import circom_compat_amd as cc
    vk, opk, raws, _ = _batch(lib, golden, 5)
    delta = opk["delta_g2"]
    dbytes = o.g2_to_bytes(delta)
    base = raws[0]
    p = H.proof_from_bytes(base)
    cases = [
        (base[:64] + dbytes + base[192:], (1, 1)),                                         # B = delta: 2 delta
        (base[:64] + o.g2_to_bytes(o.G2.neg(delta)) + base[192:], (1, 1)),                 # B = -delta: infinity
        (base[:192] + base[:64], (3, 1)),                                                  # C = A: 2 A
        (base[:192] + o.g1_to_bytes(o.G1.neg(p["a"])), (3, 1)),                            # C = -A: infinity
        (bytes(64) + base[64:], (5, 6)),                                                   # A = infinity
        (base[:64] + bytes(128) + base[192:], (5, 6)),                                     # B = infinity
        (base[:192] + bytes(64), (5, 6)),                                                  # C = infinity
    ]
    assert _want(*[cases[0][0], delta, 1, 1])[64:192] == o.g2_to_bytes(o.G2.mul(delta, 2))
    assert _want(*[cases[1][0], delta, 1, 1])[64:192] == bytes(128)
    assert _want(*[cases[2][0], delta, 3, 1])[192:] == o.g1_to_bytes(o.G1.mul(p["a"], 2))
    assert _want(*[cases[3][0], delta, 3, 1])[192:] == bytes(64)
    for k, (raw, pair) in enumerate(cases):
        at = (k * 4) % 9                                              # the odd one moves through the run
        batch = [raws[1 + (j % 4)] for j in range(9)]
        sc = _scalars(40 + k, 9)
        batch[at], sc[at] = raw, pair
        got, ok = cc.rerandomize(vk, batch, sc, lib=lib, return_ok=True)
        assert ok == [True] * 9
        for j in (at, (at + 1) % 9, (at + 8) % 9):                     # the case and its two neighbours
            assert got[j].raw == _want(batch[j], delta, *sc[j]), (k, j)
    # delta = infinity: B' = r1 B
    batch = [raws[j % 5] for j in range(9)]
    sc = _scalars(50, 9)
    got = cc.rerandomize(bytes(128), batch, sc, lib=lib)
    for j in (0, 4, 8):
        assert got[j].raw == _want(batch[j], None, *sc[j])
        assert got[j].raw[64:192] == o.g2_to_bytes(o.G2.mul(H.proof_from_bytes(batch[j])["b"], sc[j][0]))


# ---- 5. seams --------------------------------------------------------------------------------------------------
_seam = {}
SEAM_AT = (0, 62, 63, 64, 511, 512, 514)


def _seam_inputs(lib):
    """515 records from the rows of an SRS (points, not valid proofs), scalars, the n = 1 results at SEAM_AT and the
    oracle's bytes at three of them: computed once per library"""
    import circom_compat_amd as cc
    if id(lib) not in _seam:
        srs = cc.trapdoor_srs(10, (3, 5, 7), lib=lib)
        recs = [bytes(srs.tau_g1[i + 1]) + bytes(srs.tau_g2[i + 1]) + bytes(srs.alpha_tau_g1[i]) for i in range(515)]
        assert len(set(recs)) == 515
        delta = o.G2.mul(o.G2_GEN, 987654321)
        sc = _scalars(77, 515)
        single = {i: cc.rerandomize(o.g2_to_bytes(delta), [recs[i]], [sc[i]], lib=lib)[0].raw for i in SEAM_AT}
        for i in (0, 64, 514):
            assert single[i] == _want(recs[i], delta, *sc[i])
        _seam[id(lib)] = (recs, o.g2_to_bytes(delta), sc, single)
    return _seam[id(lib)]


@pytest.mark.parametrize("n", [0, 63, 64, 65, 515])
def test_block_and_inversion_run_seams(lib, n):
    """63 / 64 / 65: one block of 64 lanes less one, full, plus one; 515 = 8 * 64 + 3: past one full block of the
    affine pass (64 lanes x runs of 8) with a ragged end"""
    import circom_compat_amd as cc
    recs, dbytes, sc, single = _seam_inputs(lib)
    got, ok = cc.rerandomize(dbytes, recs[:n], sc[:n], lib=lib, return_ok=True)
    assert len(got) == n and ok == [True] * n
    for i in SEAM_AT:
        if i < n:
            assert got[i].raw == single[i], i


# ---- 6. composition --------------------------------------------------------------------------------------------
def test_two_rounds_compose(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 2)
    first, second = _scalars(61, 2), _scalars(62, 2)
    twice = cc.rerandomize(vk, cc.rerandomize(vk, raws, first, lib=lib), second, lib=lib)
    both = [(r1 * s1 % R, (r2 + s2 * pow(r1, R - 2, R)) % R) for (r1, r2), (s1, s2) in zip(first, second)]
    assert twice == cc.rerandomize(vk, raws, both, lib=lib)
    assert cc.verify_batch(vk, twice, pubs, lib=lib) == [True, True]


# ---- 7. drawn scalars ------------------------------------------------------------------------------------------
def test_drawn_scalars_and_in_place(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 5)
    one, two = cc.rerandomize(vk, raws, lib=lib), cc.rerandomize(vk, raws, lib=lib)
    for x, y, raw in zip(one, two, raws):
        for part in ("a", "b", "c"):
            assert len({getattr(x, part), getattr(y, part), getattr(cc.Proof(raw), part)}) == 3
    assert cc.verify_batch(vk, one, pubs, lib=lib) == [True] * 5
    assert cc.verify_batch(vk, two, pubs, lib=lib) == [True] * 5
    assert cc.Proof(raws[0]).rerandomize(vk, lib=lib) != cc.Proof(raws[0])
    assert cc.verify_batch(vk, [cc.Groth16.rerandomize_proof(vk, raws[1], lib=lib)], pubs[1:2], lib=lib) == [True]
    times = cc.rerandomize_times(lib=lib)
    assert list(times) == ["upload", "prepare", "mul_g1", "mul_g2", "affine", "download"]
    # in place through the C ABI
    sc = _scalars(70, 5)
    delta = (C.c_uint8 * 128).from_buffer_copy(bytes(vk.delta_g2))
    st, out, ok = _call(lib, delta, raws, sc)
    assert st == B.G16_OK and list(ok) == [1] * 5
    buf = np.frombuffer(b"".join(raws), dtype=np.uint8).copy()
    arr = H.fr_mont_arr([x for pair in sc for x in pair])
    assert lib.g16_proofs_rerandomize(0, delta, ptr(buf), 5, ptr(arr), ptr(buf), None) == B.G16_OK
    assert buf.tobytes() == out.tobytes()
    assert out.tobytes() == b"".join(_want(r, opk["delta_g2"], *s) for r, s in zip(raws, sc))


# ---- 8. structural tests ---------------------------------------------------------------------------------------
def test_structural_failures_are_zeroed_and_neighbours_untouched(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 5)
    delta = opk["delta_g2"]
    q_words = o.Q_MOD.to_bytes(32, "little")
    noncanonical = raws[1][:32] + q_words + raws[1][64:]                  # A.y stored as q itself
    noncanonical_b = raws[1][:64 + 32] + q_words + raws[1][64 + 64:]      # B.x.c1 stored as q
    a_off = bytearray(raws[2])
    a_off[0] ^= 1
    b_off = bytearray(raws[3])
    b_off[64] ^= 1
    c_off = bytearray(raws[3])
    c_off[192] ^= 1
    T = _twist_point_outside_g2(3)
    outside = raws[4][:64] + o.g2_to_bytes(T) + raws[4][192:]
    batch = [raws[0], noncanonical, raws[1], bytes(a_off), raws[2], bytes(b_off), raws[3], outside, raws[4],
             noncanonical_b, bytes(c_off)]
    sc = _scalars(80, len(batch))
    got, ok = cc.rerandomize(vk, batch, sc, lib=lib, return_ok=True)
    want_ok = [True, False, True, False, True, False, True, True, True, False, False]
    assert ok == want_ok
    for g, raw, pair, good in zip(got, batch, sc, want_ok):
        assert g.raw == (_want(raw, delta, *pair) if good else bytes(REC))
    # the twist point outside G2 went through; the result fails verification as the input does
    pub = [pubs[0], pubs[1], pubs[2], pubs[3], pubs[4]]
    verdict = cc.verify_batch(vk, [got[0], got[2], got[4], got[6], got[7], got[8]], pub[:4] + [pubs[4], pubs[4]],
                              lib=lib)
    assert verdict == [True, True, True, True, False, True]


# ---- 9. arguments ----------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 2)
    delta = (C.c_uint8 * 128).from_buffer_copy(bytes(vk.delta_g2))
    good = [(3, 4), (5, 0)]
    buf = np.frombuffer(b"".join(raws), dtype=np.uint8).copy()

    def run(**kw):
        out, ok = np.full(2 * REC, 0xA5, np.uint8), np.full(2, 0xA5, np.uint8)
        a = dict(device=0, delta=delta, proofs=ptr(buf), n=2, scalars=H.fr_mont_arr([x for p in good for x in p]),
                 out=ptr(out))
        a.update(kw)
        sc = a["scalars"]
        st = lib.g16_proofs_rerandomize(a["device"], a["delta"], a["proofs"], a["n"],
                                        ptr(sc) if sc is not None else None, a["out"], ptr(ok))
        return st, out, ok

    def raw_scalars(words):
        return np.array(words, dtype=np.uint64).reshape(-1, 4)

    r_words = [int.from_bytes(R.to_bytes(32, "little")[8 * i:8 * i + 8], "little") for i in range(4)]
    ok_rows = H.fr_mont_arr([3, 4, 5, 0])
    bad_scalars = {
        "r1 = 0": np.concatenate([ok_rows[:2], raw_scalars([0, 0, 0, 0]), ok_rows[3:]]),
        "r1 = r": np.concatenate([raw_scalars(r_words), ok_rows[1:]]),
        "r2 = r": np.concatenate([ok_rows[:3], raw_scalars(r_words)]),
        "r2 = 2^256 - 1": np.concatenate([ok_rows[:1], raw_scalars([2 ** 64 - 1] * 4), ok_rows[2:]]),
    }
    for name, kw in [("delta NULL", dict(delta=None)), ("proofs NULL", dict(proofs=None)), ("out NULL", dict(out=None)),
                     ("device -1", dict(device=-1)), ("device 1000", dict(device=1000))] + \
                    [(k, dict(scalars=np.ascontiguousarray(v))) for k, v in bad_scalars.items()]:
        st, out, ok = run(**kw)
        assert st == B.G16_ERR_INVALID, name
        assert (out == 0xA5).all() and (ok == 0xA5).all(), name
    st, out, ok = run()
    assert st == B.G16_OK and list(ok) == [1, 1]
    assert out.tobytes() == b"".join(_want(r, opk["delta_g2"], *s) for r, s in zip(raws, good))
    # empty inputs: G16_OK, nothing written, whatever the pointers
    st, out, ok = run(n=0)
    assert st == B.G16_OK and (out == 0xA5).all() and (ok == 0xA5).all()
    assert lib.g16_proofs_rerandomize(0, None, None, 0, None, None, None) == B.G16_OK
    assert lib.g16_proofs_rerandomize_keys(0, None, None, 0, None, None, None, None) == B.G16_OK
    counts = np.array([2], dtype=np.uint32)
    out = np.full(2 * REC, 0xA5, np.uint8)
    assert lib.g16_proofs_rerandomize_keys(0, delta, None, 1, ptr(buf), None, ptr(out), None) == B.G16_ERR_INVALID
    assert lib.g16_proofs_rerandomize_keys(0, None, ptr(counts), 1, ptr(buf), None, ptr(out), None) == B.G16_ERR_INVALID
    assert (out == 0xA5).all()
    assert lib.g16_proofs_rerandomize_times(None, 6) == B.G16_ERR_INVALID
    # the binding refuses bad values and counts before it calls
    for bad in ([(0, 1), (1, 1)], [(R, 1), (1, 1)], [(1, R), (1, 1)], [(1, -1), (1, 1)], [(1, 1)], [(1, 1)] * 3):
        with pytest.raises(cc.G16Error) as e:
            cc.rerandomize(vk, raws, bad, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    for bad in ([[(1, 1)]], [[(1, 1)], [(1, 1)]], [[(1, 1), (0, 1)]]):
        with pytest.raises(cc.G16Error) as e:
            cc.rerandomize_keys([(vk, raws)], bad, lib=lib)
        assert e.value.status == B.G16_ERR_INVALID
    with pytest.raises(cc.G16Error):
        cc.rerandomize(bytes(127), raws, good, lib=lib)
    with pytest.raises(cc.G16Error):
        cc.Proof(raws[0]).rerandomize(vk, r1=3, lib=lib)
    assert cc.rerandomize(vk, [], lib=lib) == [] and cc.rerandomize(vk, [], [], lib=lib) == []
    assert cc.rerandomize_keys([], lib=lib) == [] and cc.rerandomize_keys([(vk, []), (vk, [])], lib=lib) == [[], []]


def test_the_device_behind_the_last_is_invalid(emu, golden):
    """the emulator has one device: device 1 is the first that does not exist.  The refusal is hostcall.h's device_ok
    now; it is still G16_ERR_INVALID, with drawn scalars (nothing is drawn for it) as with given ones"""
    vk, _opk, raws, _pubs = _batch(emu, golden, 2)
    delta = (C.c_uint8 * 128).from_buffer_copy(bytes(vk.delta_g2))
    for scalars in ([(3, 4), (5, 0)], None):
        st, out, ok = _call(emu, delta, raws, scalars, device=1)
        assert st == B.G16_ERR_INVALID
        assert (out == 0xA5).all() and (ok == 0xA5).all()


# ---- 10. many keys ---------------------------------------------------------------------------------------------
def test_groups_under_several_keys(lib, golden):
    import circom_compat_amd as cc
    vk, opk, raws, pubs = _batch(lib, golden, 5)
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, mats = cc.read_zkey(data, lib=lib)
    pk2 = cc.contribute_key(pk, d=0xC0FFEE, lib=lib)
    assert bytes(pk2.vk.delta_g2) == o.g2_to_bytes(o.G2.mul(opk["delta_g2"], 0xC0FFEE))
    pr = cc.Prover(pk2, mats, lib=lib)
    ws = [[1, 6, 2, 3], [1, 35, 5, 7]]
    under2 = _raws(pr.prove_batch([(11, 12), (13, 14)], ws))
    pr.close()
    assert cc.verify_batch(pk2.vk, under2, [[6], [35]], lib=lib) == [True, True]
    groups = [(vk, raws[:3]), (pk2.vk, []), (pk2.vk, under2), (vk, raws[3:4])]
    sc = [_scalars(90, 3), [], _scalars(91, 2), _scalars(92, 1)]
    got, ok = cc.rerandomize_keys(groups, sc, lib=lib, return_ok=True)
    assert ok == [[True] * 3, [], [True] * 2, [True]]
    assert got == [cc.rerandomize(k, ps, s, lib=lib) for (k, ps), s in zip(groups, sc)]
    delta2 = o.g2_from_bytes(bytes(pk2.vk.delta_g2))
    assert got[2][1].raw == _want(under2[1], delta2, *sc[2][1])
    assert got[3][0].raw == _want(raws[3], opk["delta_g2"], *sc[3][0])
    assert cc.verify_batch_keys([(vk, got[0], pubs[:3]), (pk2.vk, got[2], [[6], [35]]), (vk, got[3], pubs[3:4])],
                                lib=lib) == [[True] * 3, [True] * 2, [True]]
    drawn = cc.rerandomize_keys(groups, lib=lib)
    assert [len(g) for g in drawn] == [3, 0, 2, 1] and drawn[2] != got[2]
    assert cc.verify_batch(pk2.vk, drawn[2], [[6], [35]], lib=lib) == [True, True]


# ---- 11. the product library at size -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_thousand_proofs(gpulib, golden):
    import circom_compat_amd as cc
    n = 1000
    vk, opk, raws, pubs = _test_zkey_batch(gpulib, golden, n)
    drawn = cc.rerandomize(vk, raws, lib=gpulib)
    assert cc.verify_aggregate(vk, drawn, pubs, lib=gpulib) is True
    assert all(d.raw != r for d, r in zip(drawn, raws))
    sc = _scalars(110, n)
    given = cc.rerandomize(vk, raws, sc, lib=gpulib)
    assert cc.verify_aggregate(vk, given, pubs, lib=gpulib) is True
    for i in (0, n - 1):
        assert given[i] == cc.rerandomize(vk, [raws[i]], [sc[i]], lib=gpulib)[0]
        assert given[i].raw == _want(raws[i], opk["delta_g2"], *sc[i])


@pytest.mark.gpu
def test_gpu_a_live_prover_is_left_untouched(gpulib, golden):
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, mats = cc.read_zkey(data, lib=gpulib)
    pr = cc.Prover(pk, mats, lib=gpulib)
    w = [1, 33, 3, 11]
    before = pr.prove(5, 7, w)
    again = cc.rerandomize(pk.vk, [before] * 70, _scalars(120, 70), lib=gpulib)
    after = pr.prove(5, 7, w)
    pr.close()
    assert after == before and len(set(_raws(again))) == 70
    assert cc.verify_batch(pk.vk, [again[0], again[69]], [[33], [33]], lib=gpulib) == [True, True]
