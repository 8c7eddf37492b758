"""Low-latency verification (g16_pvk_create / g16_verify_prepared / g16_pairing_check): a prepared verifying key and
the wave-cooperative pairing of csrc/pairing_coop.h, against the oracle's pairing check and against g16_verify_batch
on the same bytes.  Everything runs on the `lib` fixture (the CPU emulator and the GPU) unless marked."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_verify import _twist_point_outside_g2, _vk

P = o.R_MOD
Q = o.Q_MOD
W = [1, 33, 3, 11]                                   # the witness of tests/golden/test.zkey
_CACHE = {}


def _ref(golden):
    """the reference key, its matrices and three proofs: made once, shared, never changed"""
    if "ref" not in _CACHE:
        data = open(os.path.join(golden, "test.zkey"), "rb").read()
        opk, omats = o.read_zkey(data)
        rs = ((0, 0), (3413513218498352040262653353725127729454431939539290118844322056224532443637,
                       6077776500692565155461894309070795882353485867345896979329447163197530625403), (5, 7))
        proofs = [o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(opk, r, s, omats, 2, 1, W)) for r, s in rs]
        _CACHE["ref"] = (data, opk, proofs)
    return _CACHE["ref"]


def _words_canonical(raw):
    return all(int.from_bytes(raw[k:k + 32], "little") < Q for k in range(0, len(raw), 32))


def _oracle_verdict(opk, pub, raw):
    """the oracle's verify_proof behind the structural rules of deserialisation: canonical words, points on their
    curves, B in the prime-order subgroup"""
    if not _words_canonical(raw):
        return False
    pr = H.proof_from_bytes(raw)
    if not (o.G1.on_curve(pr["a"]) and o.G1.on_curve(pr["c"]) and o.G2.on_curve(pr["b"])):
        return False
    if pr["b"] is not None and o.G2.mul(pr["b"], P) is not None:
        return False
    return bool(o.verify_proof(opk, pub, pr))


def _plus_q(raw, off):
    v = int.from_bytes(raw[off:off + 32], "little") + Q
    assert v < 1 << 256
    return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]


def _f12_from_bytes(b):
    return [o._fq_from_mont(b[32 * i:32 * i + 32]) for i in range(12)]


def _product_is_one(g1, g2):
    f = list(o._F12_ONE)
    for p, q in zip(g1, g2):
        f = o._f12_mul(f, o.miller_loop(q, p))
    return o.final_exponentiation(f) == o._F12_ONE


def _check(cc, lib, g1, g2):
    return cc.pairing_check([o.g1_to_bytes(p) for p in g1], [o.g2_to_bytes(q) for q in g2], lib=lib)


# ---- verdicts ------------------------------------------------------------------------------------------------
def test_verdicts_equal_the_oracle_and_verify_batch(lib, golden):
    """the seven-proof batch of test_verify_batch_on_the_reference_zkey and the batch of
    test_verify_batch_rejects_what_deserialisation_rejects, in one call"""
    import circom_compat_amd as cc
    _, opk, (p0, p1, good) = _ref(golden)
    vk = _vk(cc, opk)
    swapped = o.g1_to_bytes(o.G1_GEN) + good[64:]
    off = bytearray(good)
    off[0] ^= 1
    batch = [p0, p0, p1, p1, swapped, bytes(off), bytes(256)]
    pubs = [[33], [34], [33], [34], [33], [33], [33]]
    T = _twist_point_outside_g2(1)
    cof = good[:64] + o.g2_to_bytes(T) + good[192:]
    B = H.proof_from_bytes(good)["b"]
    mixed = good[:64] + o.g2_to_bytes(o.G2.add(B, o.G2.mul(T, P))) + good[192:]
    noncanon = [_plus_q(good, k) for k in (0, 32, 64, 160, 192, 224)]
    batch += [good, cof, mixed] + noncanon + [good]
    pubs += [[33]] * (len(batch) - len(pubs))
    want = [_oracle_verdict(opk, pi, raw) for raw, pi in zip(batch, pubs)]
    assert want == [True, False, True, False, False, False, False] + [True, False, False] + [False] * 6 + [True]
    pvk = cc.prepare_verifying_key(vk, lib=lib)
    got = cc.verify_prepared(pvk, batch, pubs)
    assert got == want
    assert got == cc.verify_batch(vk, batch, pubs, lib=lib)
    # the single-proof mirror
    pvk2 = cc.Groth16.process_vk(vk, lib=lib)
    assert cc.Groth16.verify_with_processed_vk(pvk2, [33], cc.Proof(good)) is True
    assert cc.Groth16.verify_with_processed_vk(pvk2, [32], cc.Proof(good)) is False
    times = cc.verify_prepared_times(lib=lib)
    assert list(times) == ["upload", "inputs", "g2_tests", "pairing", "download", "prepare"]
    assert all(v >= 0 for v in times.values())
    pvk.close()
    pvk.close()
    with pytest.raises(cc.G16Error):
        cc.verify_prepared(pvk, [good], [[33]])


# ---- public-input counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pub", [0, 3, 65])
def test_public_input_counts(lib, n_pub):
    """no public inputs (X = IC_0), a few, and 65 (more than one wave of terms: the lanes stride) on trapdoor keys:
    the proof verifies, every single wrong input is rejected, and an input stored as a value >= r is treated as
    verify_batch treats it"""
    import circom_compat_amd as cc
    m = 2
    base = 1 + n_pub
    n_vars = base + m + 1
    cons = [([(base + i, 1)], [(base + i, 1)], [(base + i + 1, 1)]) for i in range(m)]
    rng = random.Random(100 + n_pub)
    w = [1] + [rng.randrange(2, 1 << 16) for _ in range(n_pub)] + [3]
    for _ in range(m):
        w.append(w[-1] * w[-1] % P)
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *[rng.randrange(1, P) for _ in range(5)])
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    proof = o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(
        opk, rng.randrange(P), rng.randrange(P), dict(a=a_rows, b=b_rows), n_pub + 1, len(cons), w))
    pub = w[1:1 + n_pub]
    assert o.verify_proof(opk, pub, H.proof_from_bytes(proof))
    vk = _vk(cc, opk)
    pvk = cc.prepare_verifying_key(vk, lib=lib)
    batch, pubs = [proof], [pub]
    for j in range(n_pub):
        bad = list(pub)
        bad[j] = (bad[j] + 1) % P
        batch.append(proof)
        pubs.append(bad)
    assert cc.verify_prepared(pvk, batch, pubs) == [True] + [False] * n_pub
    if n_pub:
        rows = H.fr_mont_arr(pub)
        stored = [int.from_bytes(rows[j].tobytes(), "little") for j in range(n_pub)]
        j = n_pub - 1
        assert stored[j] + P < 1 << 256
        over = rows.copy()
        over[j] = np.frombuffer((stored[j] + P).to_bytes(32, "little"), dtype=np.uint64)
        got = cc.verify_prepared(pvk, [proof, proof], [list(rows), list(over)])
        assert got == cc.verify_batch(vk, [proof, proof], [list(rows), list(over)], lib=lib)
        assert got[0] is True


# ---- the stored (alpha, beta) value ----------------------------------------------------------------------------
def test_stored_alpha_beta_value(lib, golden):
    import circom_compat_amd as cc
    _, opk, _ = _ref(golden)
    pvk = cc.prepare_verifying_key(_vk(cc, opk), lib=lib)
    f = _f12_from_bytes(pvk.alpha_beta())
    assert o.final_exponentiation(f) == o.pairing(opk["beta_g2"], o.G1.neg(opk["alpha_g1"]))


# ---- tables against on-the-fly lines ---------------------------------------------------------------------------
def test_tables_against_on_the_fly_lines(lib, golden):
    """the same four pairs through the on-the-fly path of pairing_check and through the handle's tables"""
    import circom_compat_amd as cc
    _, opk, (_, _, good) = _ref(golden)
    vk = _vk(cc, opk)
    pvk = cc.prepare_verifying_key(vk, lib=lib)
    for pub, want in (([33], True), ([34], False)):
        pr = H.proof_from_bytes(good)
        X = o.G1.add(opk["ic"][0], o.G1.mul(opk["ic"][1], pub[0]))
        g1 = [pr["a"], o.G1.neg(opk["alpha_g1"]), o.G1.neg(X), o.G1.neg(pr["c"])]
        g2 = [pr["b"], opk["beta_g2"], opk["gamma_g2"], opk["delta_g2"]]
        assert _product_is_one(g1, g2) is want
        assert bool(o.verify_proof(opk, pub, pr)) is want
        assert _check(cc, lib, g1, g2) is want
        assert cc.verify_prepared(pvk, [good], [pub]) == [want]


# ---- pairing_check on its own ------------------------------------------------------------------------------------
def _pairs(rng, n, special=()):
    """n pairs whose product is 1: n - 1 pairs (a_i G1, b_i G2) and (-(sum a_i b_i) G1, G2).  special: indices
    whose G1 side ("p") or G2 side ("q") is at infinity, or whose Q repeats the previous one ("same")"""
    g1, g2, bs, total = [], [], [], 0
    for i in range(n - 1):
        a, b = rng.randrange(1, P), rng.randrange(1, P)
        p, q = o.G1.mul(o.G1_GEN, a), o.G2.mul(o.G2_GEN, b)
        kind = dict(special).get(i)
        if kind == "p":
            p, a = None, 0
        elif kind == "q":
            q, b = None, 0
        elif kind == "same":
            q, b = g2[-1], bs[-1]
        g1.append(p)
        g2.append(q)
        bs.append(b)
        total += a * b
    g1.append(o.G1.neg(o.G1.mul(o.G1_GEN, total % P)) if total % P else None)
    g2.append(o.G2_GEN)
    return g1, g2


@pytest.mark.parametrize("n", [1, 2, 5, 16])
def test_pairing_check_products(lib, n):
    import circom_compat_amd as cc
    rng = random.Random(7000 + n)
    if n == 1:
        q = o.G2.mul(o.G2_GEN, 5)
        p = o.G1.mul(o.G1_GEN, 9)
        assert _check(cc, lib, [None], [q]) is True and _product_is_one([None], [q])
        assert _check(cc, lib, [p], [None]) is True and _product_is_one([p], [None])
        assert _check(cc, lib, [p], [q]) is False and not _product_is_one([p], [q])
        return
    if n == 2:
        a, b = rng.randrange(1, P), rng.randrange(1, P)
        g2 = [o.G2.mul(o.G2_GEN, b), o.G2_GEN]
        good = [o.G1.mul(o.G1_GEN, a), o.G1.neg(o.G1.mul(o.G1_GEN, a * b % P))]
        bad = [good[0], o.G1.neg(o.G1.mul(o.G1_GEN, (a * b + 1) % P))]
        assert _product_is_one(good, g2) and not _product_is_one(bad, g2)
        assert _check(cc, lib, good, g2) is True
        assert _check(cc, lib, bad, g2) is False
        return
    special = {1: "same", 2: "p", 3: "q"} if n == 5 else {3: "p", 7: "q", 9: "same", 10: "same"}
    g1, g2 = _pairs(rng, n, special.items())
    assert len(g1) == n and _product_is_one(g1, g2)
    assert _check(cc, lib, g1, g2) is True
    wrong = list(g1)
    wrong[0] = o.G1.add(wrong[0], o.G1_GEN)
    assert not _product_is_one(wrong, g2)
    assert _check(cc, lib, wrong, g2) is False


def test_pairing_check_rejects_malformed_points(lib):
    import circom_compat_amd as cc
    a, b = 11, 13
    g1 = [o.G1.mul(o.G1_GEN, a), o.G1.neg(o.G1.mul(o.G1_GEN, a * b))]
    g2 = [o.G2.mul(o.G2_GEN, b), o.G2_GEN]
    r1, r2 = [o.g1_to_bytes(p) for p in g1], [o.g2_to_bytes(q) for q in g2]
    assert cc.pairing_check(r1, r2, lib=lib) is True
    # a pair that contributes 1 if it is paired at all: the verdict turns on the structural test alone
    inf1, inf2 = bytes(64), bytes(128)
    T = _twist_point_outside_g2(2)
    assert cc.pairing_check(r1 + [inf1], r2 + [o.g2_to_bytes(T)], lib=lib) is False           # Q outside G2
    mixed = o.G2.add(g2[0], o.G2.mul(T, P))
    assert cc.pairing_check(r1, [o.g2_to_bytes(mixed), r2[1]], lib=lib) is False             # Q + cofactor torsion
    off = bytearray(r1[0])
    off[0] ^= 1
    assert cc.pairing_check(r1 + [bytes(off)], r2 + [inf2], lib=lib) is False                # P off the curve
    assert cc.pairing_check([_plus_q(r1[0], 0), r1[1]], r2, lib=lib) is False                # non-canonical P.x
    assert cc.pairing_check(r1, [_plus_q(r2[0], 96), r2[1]], lib=lib) is False               # non-canonical Q.y.c1
    offq = bytearray(r2[0])
    offq[0] ^= 1
    assert cc.pairing_check(r1 + [inf1], r2 + [bytes(offq)], lib=lib) is False               # Q off the twist
    with pytest.raises(cc.G16Error):
        cc.pairing_check([], [], lib=lib)
    with pytest.raises(cc.G16Error):
        cc.pairing_check(r1 * 9, r2 * 9, lib=lib)                                            # 18 pairs
    assert cc.pairing_check(r1 * 8, r2 * 8, lib=lib) is True                                 # 16 pairs


# ---- degenerate keys -----------------------------------------------------------------------------------------------
def test_degenerate_keys(lib, golden):
    import circom_compat_amd as cc
    _, opk, (_, _, good) = _ref(golden)
    vk = _vk(cc, opk)

    def key(**kw):
        f = dict(alpha_g1=bytes(vk.alpha_g1), beta_g2=bytes(vk.beta_g2), gamma_g2=bytes(vk.gamma_g2),
                 delta_g2=bytes(vk.delta_g2), ic=np.array(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64).copy())
        f.update(kw)
        return cc.VerifyingKey(f["alpha_g1"], f["beta_g2"], f["gamma_g2"], f["delta_g2"], f["ic"])

    # delta at infinity: the pair (-C, delta) contributes 1, as in verify_batch
    k_inf = key(delta_g2=bytes(128))
    pvk = cc.prepare_verifying_key(k_inf, lib=lib)
    batch, pubs = [good, good, bytes(256)], [[33], [34], [33]]
    assert cc.verify_prepared(pvk, batch, pubs) == cc.verify_batch(k_inf, batch, pubs, lib=lib)

    off_twist = bytearray(bytes(vk.gamma_g2))
    off_twist[0] ^= 1
    ic_bad = np.array(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64).copy()
    ic_bad[1, 0] ^= 1
    cases = ((key(gamma_g2=bytes(off_twist)), "gamma_g2", "off the curve"),
             (key(gamma_g2=o.g2_to_bytes(_twist_point_outside_g2(3))), "gamma_g2", "subgroup"),
             (key(alpha_g1=_plus_q(bytes(vk.alpha_g1), 32)), "alpha_g1", "non-canonical"),
             (key(ic=ic_bad), "gamma_abc_g1[1]", "off the curve"))
    for bad_key, name, reason in cases:
        with pytest.raises(cc.G16Error) as e:
            cc.prepare_verifying_key(bad_key, lib=lib)
        assert e.value.status == cc._binding.G16_ERR_INVALID
        assert name in str(e.value) and reason in str(e.value), str(e.value)


# ---- seams and reuse -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_batch_seams(lib, golden, n):
    """the only bad proof in the middle; the same handle across three calls"""
    import circom_compat_amd as cc
    _, opk, (p0, p1, good) = _ref(golden)
    pvk = cc.prepare_verifying_key(_vk(cc, opk), lib=lib)
    batch = [(p0, p1, good)[i % 3] for i in range(n)]
    pubs = [[33] for _ in range(n)]
    want = [True] * n
    if n:
        pubs[n // 2] = [35]
        want[n // 2] = False
    first = cc.verify_prepared(pvk, batch, pubs)
    assert first == want
    if n <= 2:
        assert cc.verify_prepared(pvk, batch, pubs) == first
        assert cc.verify_prepared(pvk, batch, pubs) == first
        assert first == cc.verify_batch(_vk(cc, opk), batch, pubs, lib=lib)


def test_two_handles_and_argument_errors(lib, golden):
    """two handles under two keys (the second a phase-2 contribution to the first) used alternately; argument
    errors raise and write nothing"""
    import circom_compat_amd as cc
    data, opk, (_, _, good) = _ref(golden)
    pk, mats = cc.read_zkey(data, lib=lib)
    pk2 = cc.contribute_key(pk, 0x1234567, lib=lib)
    assert bytes(pk2.vk.delta_g2) != bytes(pk.vk.delta_g2)
    pr = cc.Prover(pk2, mats, lib=lib)
    good2 = pr.prove(5, 7, W).raw
    pr.close()
    h1 = cc.prepare_verifying_key(pk.vk, lib=lib)
    h2 = cc.prepare_verifying_key(pk2.vk, lib=lib)
    for _ in range(2):
        assert cc.verify_prepared(h1, [good, good2], [[33], [33]]) == [True, False]
        assert cc.verify_prepared(h2, [good, good2], [[33], [33]]) == [False, True]
    assert cc.verify_batch(pk2.vk, [good, good2], [[33], [33]], lib=lib) == [False, True]

    with pytest.raises(cc.G16Error):
        cc.verify_prepared(h1, [good], [[33, 1]])
    with pytest.raises(cc.G16Error):
        cc.verify_prepared(h1, [good, good], [[33]])
    ok = np.full(4, 7, dtype=np.uint8)
    buf = np.frombuffer(good, dtype=np.uint8)
    pubs = H.fr_mont_arr([33])
    inv = cc._binding.G16_ERR_INVALID
    assert lib.g16_verify_prepared(h1._handle(), None, pubs.ctypes.data, 1, ok.ctypes.data) == inv
    assert lib.g16_verify_prepared(h1._handle(), buf.ctypes.data, None, 1, ok.ctypes.data) == inv
    assert lib.g16_verify_prepared(h1._handle(), buf.ctypes.data, pubs.ctypes.data, 1, None) == inv
    assert lib.g16_verify_prepared(None, buf.ctypes.data, pubs.ctypes.data, 1, ok.ctypes.data) == inv
    assert lib.g16_verify_prepared(h1._handle(), None, None, 0, None) == cc._binding.G16_OK
    assert list(ok) == [7, 7, 7, 7]
    out = C.c_void_p()
    assert lib.g16_pvk_create(0, None, C.byref(out)) == inv and not out.value
    assert lib.g16_pvk_alpha_beta(h1._handle(), None) == inv
    one = np.zeros(1, dtype=np.uint8)
    assert lib.g16_pairing_check(0, None, None, 1, one.ctypes.data) == inv
    lib.g16_pvk_destroy(None)


# ---- the use the feature is for -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_thousand_proofs_beside_a_prover_gpu(gpulib, golden):
    """1000 proofs of test.zkey from prove_batch with five spoiled ones: verify_batch's list.  A Prover created
    before the call still produces its earlier proof bytes afterwards: the call leaves the device's other work alone."""
    import circom_compat_amd as cc
    data, _, _ = _ref(golden)
    pk, mats = cc.read_zkey(data)
    pr = cc.Prover(pk, mats)
    before = pr.prove(5, 7, W).raw
    n = 1000
    rng = random.Random(99)
    rs = [(rng.randrange(P), rng.randrange(P)) for _ in range(n)]
    proofs = [p.raw for p in pr.prove_batch(rs, np.stack([cc.fr_from_ints(W)] * n))]
    pubs = [[33] for _ in range(n)]
    pubs[17] = [34]
    proofs[0] = proofs[1][:64] + proofs[0][64:]                     # another proof's A
    proofs[500] = bytes(64) + proofs[500][64:]                      # A at infinity
    flip = bytearray(proofs[998])
    flip[200] ^= 1
    proofs[998] = bytes(flip)                                       # C off the curve
    proofs[999] = proofs[999][:64] + o.g2_to_bytes(_twist_point_outside_g2(1)) + proofs[999][192:]
    pvk = cc.prepare_verifying_key(pk.vk)
    got = cc.verify_prepared(pvk, proofs, pubs)
    assert got == cc.verify_batch(pk.vk, proofs, pubs)
    assert [i for i, g in enumerate(got) if not g] == [0, 17, 500, 998, 999]
    assert pr.prove(5, 7, W).raw == before
    pr.close()
