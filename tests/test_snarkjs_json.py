"""snarkjs JSON and the Ethereum forms: the golden verification_key.json (a real snarkjs file) against the key of the
golden zkey, round trips of proof / public / vk JSON, the rejection rules, and the c1-first G2 order of the
Ethereum forms pinned to the EIP-197 generator."""
import json
import os

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

R, Q = o.R_MOD, o.Q_MOD
FIXED_R = 3413513218498352040262653353725127729454431939539290118844322056224532443637
FIXED_S = 6077776500692565155461894309070795882353485867345896979329447163197530625403

# EIP-197: the G2 generator as the precompile takes it -- the imaginary (c1) limb of each coordinate FIRST
EIP197_G2_X = [0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2,
               0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed]
EIP197_G2_Y = [0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b,
               0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa]


@pytest.fixture(scope="module")
def key(golden):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding
    return cc.read_zkey(os.path.join(golden, "test.zkey"), lib=_binding.load())


@pytest.fixture
def proof(lib, key):
    import circom_compat_amd as cc
    pr = cc.Prover(key[0], key[1], lib=lib)
    p = pr.prove(FIXED_R, FIXED_S, [1, 33, 3, 11])
    pr.close()
    return p


def _vk_fields(vk):
    return (bytes(vk.alpha_g1), bytes(vk.beta_g2), bytes(vk.gamma_g2), bytes(vk.delta_g2),
            np.asarray(vk.gamma_abc_g1, dtype=np.uint8).tobytes())


def test_read_vk_json_is_the_zkeys_vk(lib, golden, key):
    import circom_compat_amd as cc
    vk = cc.read_vk_json(os.path.join(golden, "verification_key.json"), lib=lib)
    for got, want in zip(_vk_fields(vk), _vk_fields(key[0].vk)):
        assert got == want
    assert np.asarray(vk.gamma_abc_g1).shape == (2, 64)


def test_write_vk_json_parses_equal_to_the_golden_file(lib, golden, key, tmp_path):
    import circom_compat_amd as cc
    path = str(tmp_path / "vk.json")
    cc.write_vk_json(path, key[0].vk, lib=lib)
    got = json.load(open(path))
    want = json.load(open(os.path.join(golden, "verification_key.json")))
    assert "vk_alphabeta_12" in want and "vk_alphabeta_12" not in got
    del want["vk_alphabeta_12"]
    assert got == want


def test_proof_and_public_round_trip(lib, proof, tmp_path):
    import circom_compat_amd as cc
    pj, uj = str(tmp_path / "proof.json"), str(tmp_path / "public.json")
    cc.write_proof_json(pj, proof, lib=lib)
    cc.write_public_json(uj, [33])
    j = json.load(open(pj))
    assert sorted(j) == ["curve", "pi_a", "pi_b", "pi_c", "protocol"] and j["protocol"] == "groth16" and j["curve"] == "bn128"
    assert j["pi_a"][2] == "1" and j["pi_b"][2] == ["1", "0"] and j["pi_c"][2] == "1"
    # decimal strings of the oracle's affine coordinates, c0 first
    op = H.proof_from_bytes(proof.raw)
    assert j["pi_a"][:2] == [str(op["a"][0]), str(op["a"][1])]
    assert j["pi_b"][:2] == [[str(op["b"][0][0]), str(op["b"][0][1])], [str(op["b"][1][0]), str(op["b"][1][1])]]
    assert cc.read_proof_json(pj, lib=lib) == proof
    assert cc.Proof.from_json(proof.to_json(lib=lib), lib=lib) == proof
    assert cc.Proof.from_json(json.dumps(j), lib=lib) == proof
    assert json.load(open(uj)) == ["33"] and cc.read_public_json(uj) == [33]


def test_infinity(lib, proof):
    import circom_compat_amd as cc
    p = cc.Proof(proof.raw[:192] + bytes(64))
    j = p.to_json(lib=lib)
    assert j["pi_c"] == ["0", "1", "0"]
    assert cc.Proof.from_json(j, lib=lib) == p
    j["pi_b"] = [["0", "0"], ["1", "0"], ["0", "0"]]
    assert cc.Proof.from_json(j, lib=lib).b == bytes(128)
    assert cc.Proof(bytes(256)).to_json(lib=lib)["pi_b"] == [["0", "0"], ["1", "0"], ["0", "0"]]


def test_rejections(lib, proof):
    import circom_compat_amd as cc
    good = proof.to_json(lib=lib)

    def variant(**kw):
        j = json.loads(json.dumps(good))
        j.update(kw)
        return j

    for bad in (variant(pi_a=good["pi_a"][:2] + ["2"]),                       # a third coordinate other than 0 / 1
                variant(pi_b=good["pi_b"][:2] + [["1", "1"]]),
                variant(pi_a=[str(Q), good["pi_a"][1], "1"]),                 # a coordinate equal to q
                variant(pi_b=[[good["pi_b"][0][0], str(Q)], good["pi_b"][1], ["1", "0"]]),
                variant(pi_c=[good["pi_c"][0], good["pi_c"][0], "1"]),        # off the curve
                variant(pi_a=[good["pi_a"][0], "x", "1"]),
                variant(protocol="plonk"),
                {k: v for k, v in good.items() if k != "pi_c"}):
        with pytest.raises(cc.G16Error):
            cc.Proof.from_json(bad, lib=lib)
    with pytest.raises(cc.G16Error):
        cc.read_public_json(json.dumps(["1", str(R)]))                        # an input equal to r
    with pytest.raises(cc.G16Error):
        cc.write_public_json(None, [R])
    assert cc.read_public_json(json.dumps([str(R - 1)])) == [R - 1]


def test_json_proof_verifies_against_json_vk(lib, golden, proof, tmp_path):
    import circom_compat_amd as cc
    pj = str(tmp_path / "proof.json")
    cc.write_proof_json(pj, proof, lib=lib)
    vk = cc.read_vk_json(os.path.join(golden, "verification_key.json"), lib=lib)
    p = cc.read_proof_json(pj, lib=lib)
    assert cc.verify_batch(vk, [p], [cc.read_public_json(json.dumps(["33"]))], lib=lib) == [True]
    assert cc.verify_batch(vk, [p], [[34]], lib=lib) == [False]


# ---- Ethereum -----------------------------------------------------------------------------------------------------
def test_oracle_g2_generator_is_eip197s():
    (x0, x1), (y0, y1) = o.G2_GEN[0], o.G2_GEN[1]
    assert [x1, x0] == EIP197_G2_X and [y1, y0] == EIP197_G2_Y


def test_eth_forms_put_c1_first(lib, proof):
    import circom_compat_amd as cc
    g2 = o.g2_to_bytes(o.G2_GEN)
    p = cc.Proof(proof.raw[:64] + g2 + proof.raw[192:])
    a, b, c = p.to_eth(lib=lib)
    assert [list(b[0]), list(b[1])] == [EIP197_G2_X, EIP197_G2_Y]
    op = H.proof_from_bytes(proof.raw)
    assert tuple(a) == (op["a"][0], op["a"][1]) and tuple(c) == (op["c"][0], op["c"][1])
    assert cc.Proof.from_eth(p.to_eth(lib=lib), lib=lib) == p
    assert cc.Proof.from_eth(proof.to_eth(lib=lib), lib=lib) == proof
    # (0, 0) is the identity
    inf = cc.Proof.from_eth(((0, 0), ((0, 0), (0, 0)), (0, 0)), lib=lib)
    assert inf.raw == bytes(256) and inf.to_eth(lib=lib) == ((0, 0), ((0, 0), (0, 0)), (0, 0))
    # calldata: 8 + n_public words in the order a, b, c, input; the G2 words c1 first
    text = cc.solidity_calldata(p, [33, R - 1], lib=lib)
    words = [int(w, 16) for w in __import__("re").findall(r'"(0x[0-9a-f]{64})"', text)]
    assert len(words) == 10 and text.count('"') == 20
    assert words[:2] == list(a) and words[2:6] == EIP197_G2_X + EIP197_G2_Y and words[6:8] == list(c)
    assert words[8:] == [33, R - 1] == cc.inputs_to_eth([33, R - 1])
    with pytest.raises(cc.G16Error):
        cc.inputs_to_eth([R])


def test_vk_eth_round_trip(lib, key):
    import circom_compat_amd as cc
    vk = key[0].vk
    t = vk.to_eth(lib=lib)
    assert len(t) == 5 and len(t[4]) == 2
    ovk_beta = o.g2_from_bytes(bytes(vk.beta_g2))
    assert t[1] == ((ovk_beta[0][1], ovk_beta[0][0]), (ovk_beta[1][1], ovk_beta[1][0]))
    back = cc.VerifyingKey.from_eth(t, lib=lib)
    assert _vk_fields(back) == _vk_fields(vk)
