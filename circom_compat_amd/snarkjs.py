"""snarkjs JSON (proof.json, public.json, verification_key.json) and the Ethereum forms of a proof and a key.

Host side only, and no new point code: coordinates go to and from canonical integers through the arkworks codec
(points_to_ark / points_from_ark, uncompressed), so a point read here has passed the codec's own tests -- range,
curve and, on G2, the subgroup.  Public inputs are range-tested here and converted where they are used.

    reference src/ethereum.rs                          here
    -------------------------------------------------  ----------------------------------------------
    Proof::from(ark proof).as_tuple()    :104-118      Proof.to_eth()
    ark proof from Proof                 :120-128      Proof.from_eth(t)
    VerifyingKey::from(vk).as_tuple()    :139-161      VerifyingKey.to_eth()
    ark vk from VerifyingKey             :163-173      VerifyingKey.from_eth(t)
    Inputs::from(&[Fr])                  :10-18        inputs_to_eth(values)

The tuples are the ones the reference hands to a Solidity verifier: integers (big-endian on the wire), G2 with the
c1 limb FIRST (as_tuple, :82-85), and (0, 0) for the identity (:30-34, :71-75).
"""
from __future__ import annotations

import json
from typing import List, Optional, Sequence

import numpy as np

from . import _binding as B
from . import FR_MODULUS, GT, G16Error, Proof, VerifyingKey, pairing, points_from_ark, points_to_ark

FQ_MODULUS = 21888242871839275222246405745257275088696311157297823662689037894645226208583

_REASONS = {B.KEY_BAD_ENCODING: "bad encoding", B.KEY_BAD_NONCANONICAL: "a coordinate >= q",
            B.KEY_BAD_OFF_CURVE: "not on the curve", B.KEY_BAD_SUBGROUP: "not in the subgroup"}


def _bad(msg):
    return G16Error(B.G16_ERR_INVALID, msg)


# ---- packed points <-> canonical integer coordinates ---------------------------------------------------------
def _decode(raw, group, device, lib):
    """packed Montgomery points -> per point None (infinity) or its coordinates as ints: (x, y) on G1,
    (x.c0, x.c1, y.c0, y.c1) on G2"""
    rec = 128 if group == "g2" else 64
    ark = points_to_ark(bytes(raw), group, compressed=False, device=device, lib=lib).tobytes()
    out = []
    for i in range(0, len(ark), rec):
        r = ark[i:i + rec]
        if r[-1] & 0x40:
            out.append(None)
            continue
        r = r[:-1] + bytes([r[-1] & 0x3f])   # the sign flag of the uncompressed form
        out.append(tuple(int.from_bytes(r[j:j + 32], "little") for j in range(0, rec, 32)))
    return out


def _encode(points, group, device, lib, what):
    """the inverse: a list of None / coordinate tuples -> packed bytes of all of them; a coordinate >= q or a point the
    codec rejects raises G16Error naming `what`, the index and the reason"""
    rec = 128 if group == "g2" else 64
    blob = bytearray()
    for i, p in enumerate(points):
        if p is None:
            blob += bytes(rec - 1) + b"\x40"
            continue
        if len(p) != rec // 32:
            raise _bad(f"{what}[{i}]: {rec // 32} coordinates expected")
        for c in p:
            if not 0 <= c < FQ_MODULUS:
                raise _bad(f"{what}[{i}]: a coordinate outside [0, q)")
            blob += c.to_bytes(32, "little")
    out, why, n_bad = points_from_ark(bytes(blob), group, len(points), compressed=False, validate=True, device=device,
                                      lib=lib)
    if n_bad:
        i = int(np.flatnonzero(why)[0])
        raise _bad(f"{what}[{i}]: {_REASONS.get(int(why[i]), 'rejected')}")
    return out.tobytes()


def _int(v, what):
    try:
        if isinstance(v, bool) or not isinstance(v, (str, int)):
            raise ValueError
        x = int(v, 10) if isinstance(v, str) else v
    except ValueError:
        raise _bad(f"{what}: a decimal string expected") from None
    if x < 0:
        raise _bad(f"{what}: negative")
    return x


# ---- snarkjs' projective JSON points: third coordinate 1 = affine, 0 = infinity --------------------------------
def _g1_to_json(p):
    return ["0", "1", "0"] if p is None else [str(p[0]), str(p[1]), "1"]


def _g2_to_json(p):
    if p is None:
        return [["0", "0"], ["1", "0"], ["0", "0"]]
    return [[str(p[0]), str(p[1])], [str(p[2]), str(p[3])], ["1", "0"]]


def _g1_from_json(j, what):
    if not isinstance(j, (list, tuple)) or len(j) != 3:
        raise _bad(f"{what}: three coordinates expected")
    x, y, z = (_int(v, what) for v in j)
    if z == 0:
        return None
    if z != 1:
        raise _bad(f"{what}: third coordinate {z} (0 = infinity or 1 expected)")
    return (x, y)


def _g2_from_json(j, what):
    if not isinstance(j, (list, tuple)) or len(j) != 3 or any(not isinstance(c, (list, tuple)) or len(c) != 2 for c in j):
        raise _bad(f"{what}: three pairs of coordinates expected")
    (x0, x1), (y0, y1), (z0, z1) = ([_int(v, what) for v in c] for c in j)
    if (z0, z1) == (0, 0):
        return None
    if (z0, z1) != (1, 0):
        raise _bad(f"{what}: third coordinate [{z0}, {z1}] ([0, 0] = infinity or [1, 0] expected)")
    return (x0, x1, y0, y1)


def _load(src):
    """a parsed JSON value from a path, JSON text / bytes, or an already parsed value"""
    if isinstance(src, (dict, list)):
        return src
    try:
        if isinstance(src, (bytes, bytearray)):
            return json.loads(bytes(src).decode())
        if isinstance(src, str) and src.lstrip()[:1] in ("{", "["):
            return json.loads(src)
        with open(src, "r") as f:
            return json.load(f)
    except (ValueError, UnicodeDecodeError) as e:
        raise _bad(f"not JSON: {e}") from None


def _dump(obj, path):
    text = json.dumps(obj, indent=1)
    if path is not None:
        with open(path, "w") as f:
            f.write(text + "\n")
    return text


def _header(j, what):
    if not isinstance(j, dict):
        raise _bad(f"{what}: a JSON object expected")
    if j.get("protocol", "groth16") != "groth16" or j.get("curve", "bn128") not in ("bn128", "bn254"):
        raise _bad(f"{what}: protocol groth16 on curve bn128 expected")


# ---- proof.json ----------------------------------------------------------------------------------------------
def proof_to_json(proof: Proof, device=0, lib: Optional[B.Library] = None) -> dict:
    """{"pi_a": [x, y, "1"], "pi_b": [[x.c0, x.c1], [y.c0, y.c1], ["1", "0"]], "pi_c": ..., "protocol": "groth16",
    "curve": "bn128"}: decimal strings, c0 first; infinity is ["0", "1", "0"] (G2: a third coordinate ["0", "0"])"""
    a, c = _decode(proof.a + proof.c, "g1", device, lib)
    b, = _decode(proof.b, "g2", device, lib)
    return {"pi_a": _g1_to_json(a), "pi_b": _g2_to_json(b), "pi_c": _g1_to_json(c), "protocol": "groth16",
            "curve": "bn128"}


def proof_from_json(src, device=0, lib: Optional[B.Library] = None) -> Proof:
    """the inverse (a dict, JSON text or a path).  G16Error: a third coordinate other than 0 or 1, a coordinate >= q,
    a point off the curve or, on G2, outside the subgroup."""
    j = _load(src)
    _header(j, "proof.json")
    try:
        a, c = _g1_from_json(j["pi_a"], "pi_a"), _g1_from_json(j["pi_c"], "pi_c")
        b = _g2_from_json(j["pi_b"], "pi_b")
    except KeyError as e:
        raise _bad(f"proof.json: no {e.args[0]}") from None
    g1 = _encode([a, c], "g1", device, lib, "pi_a/pi_c")
    return Proof(g1[:64] + _encode([b], "g2", device, lib, "pi_b") + g1[64:])


def write_proof_json(path, proof: Proof, device=0, lib: Optional[B.Library] = None) -> str:
    return _dump(proof_to_json(proof, device, lib), path)


def read_proof_json(src, device=0, lib: Optional[B.Library] = None) -> Proof:
    return proof_from_json(src, device, lib)


# ---- public.json ---------------------------------------------------------------------------------------------
def write_public_json(path, public_inputs: Sequence[int]) -> str:
    """a list of decimal strings; a value outside [0, r) raises G16Error"""
    vals = [int(v) for v in public_inputs]
    if any(not 0 <= v < FR_MODULUS for v in vals):
        raise _bad("public input outside [0, r)")
    return _dump([str(v) for v in vals], path)


def read_public_json(src) -> List[int]:
    j = _load(src)
    if not isinstance(j, list):
        raise _bad("public.json: a list expected")
    vals = [_int(v, f"public.json[{i}]") for i, v in enumerate(j)]
    for i, v in enumerate(vals):
        if v >= FR_MODULUS:
            raise _bad(f"public.json[{i}]: value >= r")
    return vals


# ---- verification_key.json -------------------------------------------------------------------------------------
def vk_to_json(vk: VerifyingKey, device=0, lib: Optional[B.Library] = None, alphabeta=False) -> dict:
    """protocol, curve, nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2, IC.  alphabeta=True adds
    vk_alphabeta_12 = e(alpha, beta) right after vk_delta_2, where snarkjs writes it (one pairing on the device:
    pairing / GT.to_snarkjs); off by default, snarkjs' own verifier does not read the field."""
    ic = np.ascontiguousarray(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64)
    g1 = _decode(bytes(vk.alpha_g1) + ic.tobytes(), "g1", device, lib)
    g2 = _decode(bytes(vk.beta_g2) + bytes(vk.gamma_g2) + bytes(vk.delta_g2), "g2", device, lib)
    j = {"protocol": "groth16", "curve": "bn128", "nPublic": ic.shape[0] - 1, "vk_alpha_1": _g1_to_json(g1[0]),
         "vk_beta_2": _g2_to_json(g2[0]), "vk_gamma_2": _g2_to_json(g2[1]), "vk_delta_2": _g2_to_json(g2[2])}
    if alphabeta:
        j["vk_alphabeta_12"] = pairing(bytes(vk.alpha_g1), bytes(vk.beta_g2), device=device, lib=lib).to_snarkjs()
    j["IC"] = [_g1_to_json(p) for p in g1[1:]]
    return j


def vk_from_json(src, device=0, lib: Optional[B.Library] = None, check_alphabeta=False) -> VerifyingKey:
    """the inverse; nPublic must agree with len(IC) - 1.  vk_alphabeta_12 is ignored unless check_alphabeta=True: then
    a present field is decoded (G16Error naming it if it is malformed or outside GT), e(alpha, beta) is recomputed on
    the device and a mismatch raises G16Error naming the field; an absent field is accepted."""
    j = _load(src)
    _header(j, "verification_key.json")
    try:
        ic = j["IC"]
        if not isinstance(ic, list) or not ic:
            raise _bad("verification_key.json: IC is empty")
        if "nPublic" in j and _int(j["nPublic"], "nPublic") != len(ic) - 1:
            raise _bad("verification_key.json: nPublic != len(IC) - 1")
        g1 = [_g1_from_json(j["vk_alpha_1"], "vk_alpha_1")] + [_g1_from_json(p, f"IC[{i}]") for i, p in enumerate(ic)]
        g2 = [_g2_from_json(j[k], k) for k in ("vk_beta_2", "vk_gamma_2", "vk_delta_2")]
    except KeyError as e:
        raise _bad(f"verification_key.json: no {e.args[0]}") from None
    b1 = _encode(g1, "g1", device, lib, "vk_alpha_1/IC")
    b2 = _encode(g2, "g2", device, lib, "vk_beta_2/vk_gamma_2/vk_delta_2")
    if check_alphabeta and "vk_alphabeta_12" in j:
        try:
            given = GT.from_snarkjs(j["vk_alphabeta_12"], validate=True, lib=lib, device=device)
        except G16Error as e:
            raise _bad(f"vk_alphabeta_12: {e}") from None
        if given != pairing(b1[:64], b2[:128], device=device, lib=lib):
            raise _bad("vk_alphabeta_12: not e(vk_alpha_1, vk_beta_2)")
    return VerifyingKey(b1[:64], b2[:128], b2[128:256], b2[256:],
                        np.frombuffer(b1[64:], dtype=np.uint8).reshape(-1, 64).copy())


def write_vk_json(path, vk: VerifyingKey, device=0, lib: Optional[B.Library] = None, alphabeta=False) -> str:
    return _dump(vk_to_json(vk, device, lib, alphabeta), path)


def read_vk_json(src, device=0, lib: Optional[B.Library] = None, check_alphabeta=False) -> VerifyingKey:
    return vk_from_json(src, device, lib, check_alphabeta)


# ---- Ethereum forms --------------------------------------------------------------------------------------------
def _g1_eth(p):
    return (0, 0) if p is None else (p[0], p[1])


def _g2_eth(p):   # c1 first
    return ((0, 0), (0, 0)) if p is None else ((p[1], p[0]), (p[3], p[2]))


def _g1_of_eth(t, what):
    x, y = (_int(v, what) for v in t)
    return None if (x, y) == (0, 0) else (x, y)


def _g2_of_eth(t, what):
    (x1, x0), (y1, y0) = ([_int(v, what) for v in c] for c in t)
    return None if (x0, x1, y0, y1) == (0, 0, 0, 0) else (x0, x1, y0, y1)


def proof_to_eth(proof: Proof, device=0, lib: Optional[B.Library] = None):
    """(a, b, c) = ((x, y), ((x.c1, x.c0), (y.c1, y.c0)), (x, y)) as ints; (0, 0) is the identity"""
    a, c = _decode(proof.a + proof.c, "g1", device, lib)
    b, = _decode(proof.b, "g2", device, lib)
    return _g1_eth(a), _g2_eth(b), _g1_eth(c)


def proof_from_eth(t, device=0, lib: Optional[B.Library] = None) -> Proof:
    a, b, c = t
    g1 = _encode([_g1_of_eth(a, "a"), _g1_of_eth(c, "c")], "g1", device, lib, "a/c")
    return Proof(g1[:64] + _encode([_g2_of_eth(b, "b")], "g2", device, lib, "b") + g1[64:])


def vk_to_eth(vk: VerifyingKey, device=0, lib: Optional[B.Library] = None):
    """(alpha1, beta2, gamma2, delta2, [ic...]) in the forms of proof_to_eth"""
    ic = np.ascontiguousarray(vk.gamma_abc_g1, dtype=np.uint8).reshape(-1, 64)
    g1 = _decode(bytes(vk.alpha_g1) + ic.tobytes(), "g1", device, lib)
    g2 = _decode(bytes(vk.beta_g2) + bytes(vk.gamma_g2) + bytes(vk.delta_g2), "g2", device, lib)
    return _g1_eth(g1[0]), _g2_eth(g2[0]), _g2_eth(g2[1]), _g2_eth(g2[2]), [_g1_eth(p) for p in g1[1:]]


def vk_from_eth(t, device=0, lib: Optional[B.Library] = None) -> VerifyingKey:
    alpha, beta, gamma, delta, ic = t
    b1 = _encode([_g1_of_eth(alpha, "alpha1")] + [_g1_of_eth(p, "ic") for p in ic], "g1", device, lib, "alpha1/ic")
    b2 = _encode([_g2_of_eth(p, "g2") for p in (beta, gamma, delta)], "g2", device, lib, "beta2/gamma2/delta2")
    return VerifyingKey(b1[:64], b2[:128], b2[128:256], b2[256:],
                        np.frombuffer(b1[64:], dtype=np.uint8).reshape(-1, 64).copy())


def inputs_to_eth(public_inputs: Sequence[int]) -> List[int]:
    """Inputs::from(&[Fr]): the canonical integers; a value outside [0, r) raises G16Error"""
    vals = [int(v) for v in public_inputs]
    if any(not 0 <= v < FR_MODULUS for v in vals):
        raise _bad("public input outside [0, r)")
    return vals


def solidity_calldata(proof: Proof, public_inputs: Sequence[int], device=0, lib: Optional[B.Library] = None) -> str:
    """The argument string of verifyProof(a, b, c, input), in the order of `snarkjs zkey export soliditycalldata`:
    [a.x, a.y],[[b.x.c1, b.x.c0],[b.y.c1, b.y.c0]],[c.x, c.y],[input...] -- 8 + n_public words, each a quoted 0x plus
    64 hex digits.  The ORDER and the word form are snarkjs'; the punctuation between the words (no space after a
    comma inside a group, none between groups) is written from memory and could not be pinned to snarkjs offline."""
    a, b, c = proof_to_eth(proof, device, lib)

    def word(v):
        return '"0x%064x"' % v

    def group(vs):
        return "[" + ",".join(word(v) for v in vs) + "]"

    return ",".join([group(a), "[" + group(b[0]) + "," + group(b[1]) + "]", group(c),
                     group(inputs_to_eth(public_inputs))])


__all__ = ["read_proof_json", "write_proof_json", "read_public_json", "write_public_json", "read_vk_json",
           "write_vk_json", "inputs_to_eth", "solidity_calldata", "proof_to_json", "proof_from_json", "vk_to_json",
           "vk_from_json", "FQ_MODULUS"]
