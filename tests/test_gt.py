"""Pairing VALUES (g16_pairing_products / g16_gt_multiexp / g16_gt_to_ark / g16_gt_from_ark / g16_pvk_alpha_g1_beta_g2)
and prepared inputs (g16_pvk_prepare_inputs / g16_verify_prepared_inputs), against the oracle's pairing and the golden
verification key.  The library's GT value is the oracle's reduced pairing f = pairing(Q, P) raised to the cofactor
m = 2x(6x^2 + 3x + 1) of the Fuentes-Castaneda hard part, the value snarkjs writes as vk_alphabeta_12: the golden file
pins it.  Everything runs on the `lib` fixture (the CPU emulator and the GPU) unless marked."""
import json
import os
import random

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
from test_verify import _twist_point_outside_g2, _vk

R = o.R_MOD
Q = o.Q_MOD
X = o.BN_X
M = 2 * X * (6 * X * X + 3 * X + 1)                  # the cofactor the device chain (and snarkjs, arkworks) carries
W = [1, 33, 3, 11]                                   # the witness of tests/golden/test.zkey
_CACHE = {}


def _tower(f):
    """flat Fq12 = Fq[w]/(w^12 - 18 w^6 + 82) (coefficient a_i at w^i) -> snarkjs' [2][3][2] decimal strings: for i < 6
    the Fq2 coefficient (a_i + 9 a_{i+6}, a_{i+6}) at [i & 1][i >> 1]; the inverse of the oracle's _embed"""
    out = [[None] * 3 for _ in range(2)]
    for i in range(6):
        out[i & 1][i >> 1] = [str((f[i] + 9 * f[i + 6]) % Q), str(f[i + 6])]
    return out


def _oracle_value(g1, g2):
    """(prod_i pairing(Q_i, P_i))^m: the final exponentiation is a homomorphism, so it is taken once over the product of
    the Miller values, as the oracle's own pairing-product check does"""
    f = list(o._F12_ONE)
    for p, q in zip(g1, g2):
        f = o._f12_mul(f, o.miller_loop(q, p))
    return _tower(o._f12_pow(o.final_exponentiation(f), M))


def _b1(p):
    return o.g1_to_bytes(p)


def _b2(q):
    return o.g2_to_bytes(q)


def _plus_q(raw, off):
    v = int.from_bytes(raw[off:off + 32], "little") + Q
    assert v < 1 << 256
    return raw[:off] + v.to_bytes(32, "little") + raw[off + 32:]


def _golden_key(golden):
    if "gj" not in _CACHE:
        _CACHE["gj"] = json.load(open(os.path.join(golden, "verification_key.json")))
    return _CACHE["gj"]


def _products():
    """products of 0, 1, 2, 5 and 16 pairs of small multiples of the generators with the oracle's values: made once,
    shared, never changed.  18 oracle Miller loops and 5 final exponentiations in all (16 of the pairs repeat four
    points)."""
    if "products" not in _CACHE:
        rng = random.Random(4242)
        pool1 = [o.G1.mul(o.G1_GEN, rng.randrange(2, 200)) for _ in range(4)]
        pool2 = [o.G2.mul(o.G2_GEN, rng.randrange(2, 200)) for _ in range(4)]
        res = []
        for n in (0, 1, 2, 5, 16):
            g1 = [pool1[(k + n) % 4] for k in range(n)]
            g2 = [pool2[(3 * k + n) % 4] for k in range(n)]
            res.append((g1, g2, _oracle_value(g1, g2)))
        _CACHE["products"] = res
    return _CACHE["products"]


def _group(g1, g2):
    return [_b1(p) for p in g1], [_b2(q) for q in g2]


# ---- 1. the golden pin ---------------------------------------------------------------------------------------------
def test_golden_alphabeta(lib, golden):
    """e(alpha, beta) of the golden key three ways, each equal to the file's vk_alphabeta_12; the exported JSON equals
    the golden JSON with nothing deleted, key order included"""
    import circom_compat_amd as cc
    gj = _golden_key(golden)
    vk = cc.read_vk_json(os.path.join(golden, "verification_key.json"), lib=lib)
    want = gj["vk_alphabeta_12"]
    assert want[0][0][0] == "2029413683389138792403550203267699914886160938906632433982220835551125967885"
    e = cc.pairing(bytes(vk.alpha_g1), bytes(vk.beta_g2), lib=lib)
    assert e.to_snarkjs() == want
    pvk = cc.prepare_verifying_key(vk, lib=lib)
    assert pvk.alpha_g1_beta_g2() == e and pvk.alpha_g1_beta_g2().to_snarkjs() == want      # computed, then cached
    j = cc.snarkjs.vk_to_json(vk, lib=lib, alphabeta=True)
    assert j["vk_alphabeta_12"] == want
    assert j == gj and list(j) == list(gj)
    assert "vk_alphabeta_12" not in cc.snarkjs.vk_to_json(vk, lib=lib)
    # the oracle agrees: pairing(beta, alpha)^m in the tower basis, and it is not the plain reduced pairing
    opk, _ = o.read_zkey(open(os.path.join(golden, "test.zkey"), "rb").read())
    f = o.pairing(opk["beta_g2"], opk["alpha_g1"])
    assert _tower(o._f12_pow(f, M)) == want and _tower(f) != want


# ---- 2. against the oracle ------------------------------------------------------------------------------------------
def test_products_equal_the_oracle(lib):
    import circom_compat_amd as cc
    prods = _products()
    got, ok = cc.pairing_products([_group(g1, g2) for g1, g2, _ in prods], lib=lib, return_ok=True)
    assert ok == [True] * 5
    for v, (g1, _, want) in zip(got, prods):
        assert v.to_snarkjs() == want, len(g1)
    assert got[0].is_one() and got[0] == cc.GT.one()
    assert len({v for v in got}) == 5


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_batch_seams(lib, n):
    """the batch sizes around the grid's seams; products of different lengths (the empty one among them) in one call"""
    import circom_compat_amd as cc
    prods = _products()
    order = [4 if i == 40 else 3 if i % 16 == 1 else (1, 2, 0)[i % 3] for i in range(n)]   # 16 pairs once: emulator time
    got = cc.pairing_products([_group(*prods[k][:2]) for k in order], lib=lib)
    assert len(got) == n
    singles = {}
    for v, k in zip(got, order):
        if k not in singles:
            singles[k] = v
            assert v.to_snarkjs() == prods[k][2]
        assert v == singles[k]


# ---- 3. bilinearity on the device alone ----------------------------------------------------------------------------
def test_bilinearity(lib):
    import circom_compat_amd as cc
    a, b = 5, 7
    P1, Q1 = o.G1.mul(o.G1_GEN, 3), o.G2.mul(o.G2_GEN, 2)
    aP, bQ = o.G1.mul(P1, a), o.G2.mul(Q1, b)
    e, eab, eneg = cc.pairing_products([([_b1(P1)], [_b2(Q1)]), ([_b1(aP)], [_b2(bQ)]),
                                        ([_b1(o.G1.neg(P1))], [_b2(Q1)])], lib=lib)
    assert not e.is_one()
    assert eab == e ** (a * b)
    assert (e * eneg).is_one()
    assert e.inverse() == e ** (R - 1) == eneg == e ** -1
    assert (e ** R).is_one() and (e ** 0).is_one() and e ** 1 == e and e ** (R + 1) == e
    assert ((e ** (R - 1)) * e).is_one()
    s1, s2 = random.Random(5).randrange(R), random.Random(6).randrange(R)
    g1 = [(e, s1), (eab, s2)]
    g2 = [(eneg, 3)]
    both = cc.gt_multiexp([g1, g2, []], lib=lib)
    assert both[:2] == [cc.gt_multiexp([g1], lib=lib)[0], cc.gt_multiexp([g2], lib=lib)[0]]
    assert both[2].is_one()
    assert both[0] == (e ** s1) * (eab ** s2) == e ** ((s1 + a * b * s2) % R)
    assert cc.gt_multiexp([[(e, 1)]], lib=lib)[0] == e                       # one pair, scalar 1: a copy
    assert cc.gt_multiexp([[(e, 1), (eab, 1)]], lib=lib)[0] == e * eab       # scalars 1, 1: a product
    assert hash(e ** 2) == hash(e * e) and e != eab and e != 1
    with pytest.raises(AttributeError):
        e.raw = bytes(384)
    # the C entry refuses a scalar that is not below r instead of reducing it
    src = np.frombuffer(e.raw, dtype=np.uint8)
    off = np.array([0, 1], dtype=np.uint32)
    out = np.full(384, 7, dtype=np.uint8)
    for s, st in ((R - 1, cc._binding.G16_OK), (R, cc._binding.G16_ERR_INVALID)):
        sc = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint64)
        assert lib.g16_gt_multiexp(0, src.ctypes.data, sc.ctypes.data, off.ctypes.data, 1, out.ctypes.data) == st
    assert out.tobytes() == e.inverse().raw


# ---- 4. degenerate and malformed ------------------------------------------------------------------------------------
def test_degenerate_and_malformed(lib):
    import circom_compat_amd as cc
    p, q = o.G1.mul(o.G1_GEN, 9), o.G2.mul(o.G2_GEN, 5)
    r1, r2 = _b1(p), _b2(q)
    inf1, inf2 = bytes(64), bytes(128)
    good = ([r1], [r2])
    e = cc.pairing(r1, r2, lib=lib)
    vals, ok = cc.pairing_products([([inf1], [r2]), ([r1], [inf2]), ([r1, inf1], [r2, r2])], lib=lib, return_ok=True)
    assert ok == [True] * 3 and vals[0].is_one() and vals[1].is_one() and vals[2] == e
    off1 = bytearray(r1)
    off1[0] ^= 1
    off2 = bytearray(r2)
    off2[0] ^= 1
    T = _twist_point_outside_g2(2)
    assert o.G2.on_curve(T) and o.G2.mul(T, R) is not None
    bad = {"non-canonical P.x": ([_plus_q(r1, 0)], [r2]), "non-canonical Q.y.c1": ([r1], [_plus_q(r2, 96)]),
           "P off the curve": ([bytes(off1)], [r2]), "Q off the twist": ([r1], [bytes(off2)]),
           "Q outside G2": ([r1], [_b2(T)]), "Q outside G2 beside an infinite P": ([r1, inf1], [r2, _b2(T)])}
    groups = [good]
    for g in bad.values():
        groups += [g, good]
    vals, ok = cc.pairing_products(groups, lib=lib, return_ok=True)
    assert ok == [True] + [False, True] * len(bad)
    for k, name in enumerate(bad):
        assert vals[1 + 2 * k].raw == bytes(384), name
        assert vals[2 * k] == e and vals[2 + 2 * k] == e, name
    for a, b in bad.values():                                                # the single-pair form raises instead
        with pytest.raises(cc.G16Error):
            cc.pairing(a[-1], b[-1], lib=lib)
    # 16 pairs fit, 17 raise and name the product
    assert cc.pairing_products([([r1] * 16, [r2] * 16)], lib=lib)[0] == e ** 16
    with pytest.raises(cc.G16Error) as err:
        cc.pairing_products([good, ([r1] * 17, [r2] * 17)], lib=lib)
    assert err.value.status == cc._binding.G16_ERR_INVALID and "product 1" in str(err.value)
    with pytest.raises(cc.G16Error):
        cc.pairing_products([([r1], [])], lib=lib)
    # argument errors write nothing; the empty call is accepted
    out = np.full(384, 7, dtype=np.uint8)
    off = np.array([0, 1], dtype=np.uint32)
    a1, a2 = np.frombuffer(r1, dtype=np.uint8), np.frombuffer(r2, dtype=np.uint8)
    inv = cc._binding.G16_ERR_INVALID
    assert lib.g16_pairing_products(0, None, a2.ctypes.data, off.ctypes.data, 1, out.ctypes.data, None) == inv
    assert lib.g16_pairing_products(0, a1.ctypes.data, a2.ctypes.data, None, 1, out.ctypes.data, None) == inv
    assert lib.g16_pairing_products(0, a1.ctypes.data, a2.ctypes.data, off.ctypes.data, 1, None, None) == inv
    assert lib.g16_pairing_products(0, None, None, None, 0, None, None) == cc._binding.G16_OK
    assert lib.g16_gt_multiexp(0, None, None, None, 0, None) == cc._binding.G16_OK
    assert lib.g16_gt_to_ark(0, None, 0, None) == cc._binding.G16_OK
    assert lib.g16_gt_from_ark(0, None, 0, 1, None, None) == cc._binding.G16_OK
    assert lib.g16_pvk_alpha_g1_beta_g2(None, out.ctypes.data) == inv
    assert set(out) == {7}
    assert lib.g16_pairing_products(0, a1.ctypes.data, a2.ctypes.data, off.ctypes.data, 1, out.ctypes.data, None) == 0
    assert out.tobytes() == e.raw                                            # ok_out may be NULL
    assert list(cc.gt_times(lib=lib)) == ["upload", "g2_tests", "kernels", "download"]


# ---- 5. codecs -----------------------------------------------------------------------------------------------------
def test_codecs(lib, golden, tmp_path):
    import circom_compat_amd as cc
    gj = _golden_key(golden)
    want = gj["vk_alphabeta_12"]
    g = cc.GT.from_snarkjs(want, lib=lib)
    vk = cc.read_vk_json(os.path.join(golden, "verification_key.json"), lib=lib)
    assert g == cc.pairing(bytes(vk.alpha_g1), bytes(vk.beta_g2), lib=lib)
    ark = g.to_ark()
    assert len(ark) == 384
    # by hand: Fq12.c0.c0.c0 is the first word, Fq12.c1.c2.c1 the last, each 32 bytes little-endian
    assert ark[:32] == int(want[0][0][0]).to_bytes(32, "little")
    assert ark[32:64] == int(want[0][0][1]).to_bytes(32, "little")
    assert ark[64:96] == int(want[0][1][0]).to_bytes(32, "little")
    assert ark[192:224] == int(want[1][0][0]).to_bytes(32, "little")
    assert ark[352:] == int(want[1][2][1]).to_bytes(32, "little")
    assert cc.GT.from_ark(ark, lib=lib) == g and cc.GT.from_ark(ark, validate=False, lib=lib) == g
    one = cc.GT.one(lib=lib)
    assert one.to_ark() == (1).to_bytes(32, "little") + bytes(352) and cc.GT.from_ark(one.to_ark(), lib=lib).is_one()
    several = cc.gt_from_ark(ark + one.to_ark() + (g * g).to_ark(), lib=lib)
    assert several == [g, one, g ** 2]
    # a coordinate >= q, in the first and in the last word
    for k in (0, 352):
        over = ark[:k] + (int.from_bytes(ark[k:k + 32], "little") + Q).to_bytes(32, "little") + ark[k + 32:]
        for validate in (True, False):
            with pytest.raises(cc.G16Error) as err:
                cc.GT.from_ark(over, validate=validate, lib=lib)
            assert ">= q" in str(err.value)
    # Fq12 elements outside GT: 2, 0, and the golden value with one coefficient moved
    two = (2).to_bytes(32, "little") + bytes(352)
    moved = ark[:32] + ((int(want[0][0][1]) + 1) % Q).to_bytes(32, "little") + ark[64:]
    for outside in (two, bytes(384), moved):
        with pytest.raises(cc.G16Error) as err:
            cc.GT.from_ark(outside, lib=lib)
        assert "not in GT" in str(err.value)
    assert cc.GT.from_ark(two, validate=False, lib=lib).to_ark() == two      # unvalidated: decoded as it is
    with pytest.raises(cc.G16Error) as err:
        cc.gt_from_ark(ark + two, lib=lib)
    assert "element 1" in str(err.value)
    for junk in ([], [[["1", "2"]] * 3], "x", [[["1", "-2"]] * 3] * 2, [[["1", "a"]] * 3] * 2):
        with pytest.raises(cc.G16Error):
            cc.GT.from_snarkjs(junk, lib=lib)
    # the key file: the field is checked on request only
    path = os.path.join(golden, "verification_key.json")
    assert bytes(cc.read_vk_json(path, lib=lib, check_alphabeta=True).alpha_g1) == bytes(vk.alpha_g1)
    text = open(path).read()
    digit = want[1][1][0]
    changed = digit[:-1] + str((int(digit[-1]) + 1) % 10)
    assert text.count(digit) == 1
    bad = str(tmp_path / "vk_bad.json")
    open(bad, "w").write(text.replace(digit, changed))
    cc.read_vk_json(bad, lib=lib)                                            # unchecked by default, as before
    with pytest.raises(cc.G16Error) as err:
        cc.read_vk_json(bad, lib=lib, check_alphabeta=True)
    assert "vk_alphabeta_12" in str(err.value)
    # a member of GT that is not e(alpha, beta), and an absent field
    other = dict(gj)
    other["vk_alphabeta_12"] = (g * g).to_snarkjs()
    with pytest.raises(cc.G16Error) as err:
        cc.snarkjs.vk_from_json(other, lib=lib, check_alphabeta=True)
    assert "vk_alphabeta_12" in str(err.value)
    del other["vk_alphabeta_12"]
    cc.snarkjs.vk_from_json(other, lib=lib, check_alphabeta=True)


# ---- 6. prepared inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pub", [0, 3, 65])
def test_prepared_inputs(lib, n_pub):
    """the trapdoor keys of test_public_input_counts: prepare_inputs equals the oracle's IC sum, and
    verify_prepared_inputs gives verify_prepared's verdicts"""
    import circom_compat_amd as cc
    m = 2
    base = 1 + n_pub
    n_vars = base + m + 1
    cons = [([(base + i, 1)], [(base + i, 1)], [(base + i + 1, 1)]) for i in range(m)]
    rng = random.Random(100 + n_pub)
    w = [1] + [rng.randrange(2, 1 << 16) for _ in range(n_pub)] + [3]
    for _ in range(m):
        w.append(w[-1] * w[-1] % R)
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *[rng.randrange(1, R) for _ in range(5)])
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    proof = o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(
        opk, rng.randrange(R), rng.randrange(R), dict(a=a_rows, b=b_rows), n_pub + 1, len(cons), w))
    pub = w[1:1 + n_pub]
    wrong = list(pub)
    if n_pub:
        wrong[n_pub // 2] = (wrong[n_pub // 2] + 1) % R
    pvk = cc.prepare_verifying_key(_vk(cc, opk), lib=lib)

    def ic_sum(vals):
        acc = opk["ic"][0]
        for v, pt in zip(vals, opk["ic"][1:]):
            acc = o.G1.add(acc, o.G1.mul(pt, v))
        return o.g1_to_bytes(acc)

    prepared = cc.prepare_inputs(pvk, [pub, wrong])
    assert prepared == [ic_sum(pub), ic_sum(wrong)]
    assert cc.prepare_inputs(pvk, []) == []
    assert cc.Groth16.prepare_inputs(pvk, pub) == prepared[0]
    off_curve = bytearray(prepared[0])
    off_curve[0] ^= 1
    xs = [prepared[0], prepared[1], bytes(off_curve), _plus_q(prepared[0], 32), prepared[0]]
    want = cc.verify_prepared(pvk, [proof, proof], [pub, wrong])
    assert want == [True, n_pub == 0]
    got = cc.verify_prepared_inputs(pvk, [proof] * 5, xs)
    assert got == want + [False, False, True]
    assert cc.verify_prepared_inputs(pvk, [], []) == []
    assert cc.Groth16.verify_proof_with_prepared_inputs(pvk, cc.Proof(proof), prepared[0]) is True
    spoiled = bytearray(proof)
    spoiled[200] ^= 1                                                        # C off the curve
    assert cc.verify_prepared_inputs(pvk, [bytes(spoiled), proof], [prepared[0]] * 2) == \
        cc.verify_prepared(pvk, [bytes(spoiled), proof], [pub, pub]) == [False, True]
    with pytest.raises(cc.G16Error):
        cc.verify_prepared_inputs(pvk, [proof], [])
    with pytest.raises(cc.G16Error):
        cc.prepare_inputs(pvk, [pub + [1]])


# ---- 7. the command line -------------------------------------------------------------------------------------------
def test_cli_alphabeta(lib, golden, tmp_path, capsys):
    import circom_compat_amd as cc
    from circom_compat_amd.__main__ import main
    zkey = os.path.join(golden, "test.zkey")
    gpath = os.path.join(golden, "verification_key.json")
    with_field, without = str(tmp_path / "vk12.json"), str(tmp_path / "vk.json")
    assert main(["export-vkey", "--alphabeta", zkey, with_field], lib) == 0
    assert json.load(open(with_field)) == _golden_key(golden)
    assert list(json.load(open(with_field))) == list(_golden_key(golden))
    assert main(["export-vkey", zkey, without], lib) == 0
    want = dict(_golden_key(golden))
    del want["vk_alphabeta_12"]
    assert json.load(open(without)) == want
    assert open(without).read() == cc.write_vk_json(None, cc.read_zkey(zkey, lib=lib)[0].vk, lib=lib) + "\n"
    # verify --check-alphabeta: the golden key passes, a key whose field was changed is bad input
    pk, mats = cc.read_zkey(zkey, lib=lib)
    pr = cc.Prover(pk, mats, lib=lib)
    pj, uj = str(tmp_path / "proof.json"), str(tmp_path / "public.json")
    cc.write_proof_json(pj, pr.prove(5, 7, W), lib=lib)
    pr.close()
    cc.write_public_json(uj, [33])
    capsys.readouterr()
    assert main(["verify", "--check-alphabeta", gpath, uj, pj], lib) == 0
    assert capsys.readouterr().out.strip() == "OK"
    tampered = dict(_golden_key(golden))
    tampered["vk_alphabeta_12"] = [[["1", "0"], ["0", "0"], ["0", "0"]], [["0", "0"]] * 3]   # one: in GT, not e(alpha, beta)
    bad = str(tmp_path / "vk_one.json")
    json.dump(tampered, open(bad, "w"))
    assert main(["verify", bad, uj, pj], lib) == 0
    capsys.readouterr()
    assert main(["verify", "--check-alphabeta", bad, uj, pj], lib) == 2
    assert "vk_alphabeta_12" in capsys.readouterr().err


# ---- 8. the use the feature is for ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_thousand_products_beside_a_prover_gpu(gpulib, golden):
    """1000 products of 3 pairs in one call: every value equals the single call on the same pairs (there are 16
    different products), spot-checked against the oracle's bilinearity, and a Prover created before the call still
    produces its earlier proof bytes afterwards"""
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "test.zkey"), "rb").read()
    pk, mats = cc.read_zkey(data)
    pr = cc.Prover(pk, mats)
    before = pr.prove(5, 7, W).raw
    rng = random.Random(31)
    ks1 = [rng.randrange(1, R) for _ in range(6)]
    ks2 = [rng.randrange(1, R) for _ in range(6)]
    p1 = [_b1(o.G1.mul(o.G1_GEN, k)) for k in ks1]
    p2 = [_b2(o.G2.mul(o.G2_GEN, k)) for k in ks2]
    kinds = [[(rng.randrange(6), rng.randrange(6)) for _ in range(3)] for _ in range(16)]
    n = 1000
    order = [rng.randrange(16) for _ in range(n)]
    groups = [([p1[a] for a, _ in kinds[k]], [p2[b] for _, b in kinds[k]]) for k in order]
    got, ok = cc.pairing_products(groups, return_ok=True)
    assert ok == [True] * n
    single = {}
    for i in (0, 1, 499, 998, 999):
        single[order[i]] = cc.pairing_products([groups[i]])[0]
    for k in range(16):
        if k not in single:
            single[k] = got[order.index(k)]
    assert all(got[i] == single[order[i]] for i in range(n))
    e = cc.pairing(_b1(o.G1_GEN), _b2(o.G2_GEN))
    for k in (order[0], order[999]):
        assert single[k] == e ** (sum(ks1[a] * ks2[b] for a, b in kinds[k]) % R)
    assert pr.prove(5, 7, W).raw == before
    pr.close()
