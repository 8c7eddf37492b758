"""The ark-serialize containers -- ProvingKey, VerifyingKey, Proof -- against blobs this test assembles itself from
the layout in include/g16_amd.h (points through the Python encoder of test_ark_codec.py), on tiny keys minted by
the oracle: one with CircomReduction's H query, one with LibsnarkReduction's domain - 1 points."""
import pytest

import bn254_ref as o
import circom_compat_amd as cc
import helpers as H
from test_ark_codec import INF, NEG, Q, _le, py_encode

R_ = 3413513218498352040262653353725127729454431939539290118844322056224532443637
S_ = 6077776500692565155461894309070795882353485867345896979329447163197530625403
FIELDS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "ic", "beta_g1", "delta_g1", "a_query", "b_g1_query",
          "b_g2_query", "h_query", "l_query")
G2_FIELDS = ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query")
VECS = ("ic", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
_KEYS = {}


def minted(reduction):
    """(oracle key, circuit, h_len), computed once"""
    if reduction not in _KEYS:
        cons, wit, n_vars, n_pub = H.squaring_chain(3)
        opk = o.trapdoor_setup(cons, n_vars, n_pub, 11, 22, 33, 44, 55, reduction=reduction)
        h_len = opk["domain_size"] - (1 if reduction == "libsnark" else 0)
        if reduction == "libsnark":
            assert opk["h_query"][-1] is None and all(P is not None for P in opk["h_query"][:-1])
        _KEYS[reduction] = (opk, (cons, wit, n_vars, n_pub), h_len)
    return _KEYS[reduction]


def pieces(opk, compressed, h_len, only_vk=False):
    """[(name, bytes)] in file order; a Vec's length prefix is a piece of its own, named 'len(<field>)'"""
    out = []
    for name in FIELDS[:5] if only_vk else FIELDS:
        group = "g2" if name in G2_FIELDS else "g1"
        val = opk[name]
        if name in VECS:
            pts = val[:h_len] if name == "h_query" else val
            out.append((f"len({name})", len(pts).to_bytes(8, "little")))
            out.append((name, b"".join(py_encode(group, P, compressed) for P in pts)))
        else:
            out.append((name, py_encode(group, val, compressed)))
    return out


def blob_of(ps):
    return b"".join(b for _, b in ps)


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_key_write_and_read(lib, reduction, compressed):
    opk, _, h_len = minted(reduction)
    pk = H.pk_from_oracle(opk)
    want = blob_of(pieces(opk, compressed, h_len))
    got = cc.write_ark_key(pk, compressed=compressed, h_len=h_len, lib=lib)
    assert len(got) == len(want) == lib.g16_ark_pk_size(1 if compressed else 0, pk.n_vars, pk.n_public, h_len)
    assert got == want
    back = cc.read_ark_key(want, compressed=compressed, lib=lib)
    assert (back.n_vars, back.n_public, back.domain_size) == (pk.n_vars, pk.n_public, pk.domain_size)
    for name in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query"):
        assert getattr(back, name).tobytes() == getattr(pk, name).tobytes(), name
    assert back.h_query.shape == (pk.domain_size, 64)
    if reduction == "libsnark":
        assert not back.h_query[-1].any() and back.h_query[-2].any()               # padded with infinity
    assert (back.beta_g1, back.delta_g1) == (pk.beta_g1, pk.delta_g1)
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert getattr(back.vk, name) == getattr(pk.vk, name), name
    assert back.vk.gamma_abc_g1.tobytes() == pk.vk.gamma_abc_g1.tobytes()
    assert cc.write_ark_key(back, compressed=compressed, h_len=h_len, lib=lib) == want   # and to the same bytes


@pytest.mark.parametrize("compressed", [True, False])
def test_vk_round_trip(lib, compressed):
    opk, _, _ = minted("circom")
    pk = H.pk_from_oracle(opk)
    want = blob_of(pieces(opk, compressed, 0, only_vk=True))
    assert cc.write_ark_vk(pk.vk, compressed=compressed, lib=lib) == want
    vk = cc.read_ark_vk(want, compressed=compressed, lib=lib)
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert getattr(vk, name) == getattr(pk.vk, name), name
    assert vk.gamma_abc_g1.tobytes() == pk.vk.gamma_abc_g1.tobytes()
    for bad in (want[:-1], want + b"\0", want[:40]):
        with pytest.raises(cc.G16Error) as e:
            cc.read_ark_vk(bad, compressed=compressed, lib=lib)
        assert e.value.status == 5


@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
def test_prover_on_the_reread_key_and_proofs(lib, reduction):
    opk, (cons, wit, n_vars, n_pub), h_len = minted(reduction)
    pk = H.pk_from_oracle(opk)
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    mats = H.matrices_from_rows(a_rows, b_rows, n_pub + 1, n_vars, lib)
    back = cc.read_ark_key(cc.write_ark_key(pk, h_len=h_len, lib=lib), lib=lib)
    p0 = cc.Prover(pk, mats, lib=lib, reduction=reduction).prove(R_, S_, wit)
    p1 = cc.Prover(back, mats, lib=lib, reduction=reduction).prove(R_, S_, wit)
    assert p1.raw == p0.raw
    pub = [wit[1:1 + n_pub]]
    assert cc.verify_batch(pk.vk, [p0], pub, lib=lib) == [True]
    for compressed, size in ((True, 128), (False, 256)):
        ark = p0.to_ark(compressed=compressed, lib=lib)
        assert len(ark) == size
        pr = H.proof_from_bytes(p0.raw)
        assert ark == py_encode("g1", pr["a"], compressed) + py_encode("g2", pr["b"], compressed) + \
            py_encode("g1", pr["c"], compressed)
        assert cc.Proof.from_ark(ark, compressed=compressed, lib=lib) == p0
        got = cc.proofs_from_ark(ark + ark, 2, compressed=compressed, lib=lib)
        assert got == [p0, p0]
        assert cc.verify_batch(back.vk, got, pub + pub, lib=lib) == [True, True]
    # the sign bit of A flipped: still a point of the curve, so it decodes -- and the verifier rejects it
    ark = bytearray(p0.to_ark(lib=lib))
    ark[31] ^= NEG
    flipped = cc.Proof.from_ark(bytes(ark), lib=lib)
    assert flipped != p0 and flipped.raw[64:] == p0.raw[64:] and flipped.raw[:32] == p0.raw[:32]
    assert cc.verify_batch(pk.vk, [flipped], pub, lib=lib) == [False]
    # a proof point that does not decode names itself
    ark = bytearray(p0.to_ark(lib=lib) * 3)
    ark[128 + 32:128 + 96] = _le(Q, 0)
    with pytest.raises(cc.G16Error) as e:
        cc.proofs_from_ark(bytes(ark), 3, lib=lib)
    assert e.value.status == 5 and "proof 1, point b" in e.value.message


def _expect_io(lib, blob, compressed=True, needle=None):
    with pytest.raises(cc.G16Error) as e:
        cc.read_ark_key(blob, compressed=compressed, lib=lib)
    assert e.value.status == 5, e.value
    if needle:
        assert needle in e.value.message, e.value.message


@pytest.mark.parametrize("compressed", [True, False])
def test_malformed_blobs(lib, compressed):
    opk, _, h_len = minted("circom")
    ps = pieces(opk, compressed, h_len)
    blob = blob_of(ps)
    cc.read_ark_key(blob, compressed=compressed, lib=lib)                           # the blob itself is fine
    at = 0
    for name, b in ps:                                                              # truncated at every boundary ...
        _expect_io(lib, blob[:at], compressed)
        if len(b) > 8:
            _expect_io(lib, blob[:at + 5], compressed)                              # ... and in the middle of a point
        at += len(b)
    _expect_io(lib, blob + b"\0", compressed, "trailing")                           # one trailing byte
    names = [n for n, _ in ps]

    def replaced(name, new):
        return blob_of([(n, new if n == name else b) for n, b in ps])

    _expect_io(lib, replaced("len(a_query)", (1 << 63).to_bytes(8, "little")), compressed, "a_query")
    _expect_io(lib, replaced("len(h_query)", (2 ** 64 - 1).to_bytes(8, "little")), compressed, "h_query")
    # len(b_g1_query) != len(a_query), in an otherwise well-formed blob
    b1 = dict(ps)["b_g1_query"]
    rec = len(b1) // opk["n_vars"]
    short = [(n, (opk["n_vars"] - 1).to_bytes(8, "little") if n == "len(b_g1_query)" else
              b[:-rec] if n == "b_g1_query" else b) for n, b in ps]
    _expect_io(lib, blob_of(short), compressed, "b_g1_query")
    assert names.index("h_query") < names.index("l_query")                          # h BEFORE l
    # one corrupted point: the message names the array and the index
    a = bytearray(dict(ps)["a_query"])
    rec = len(a) // opk["n_vars"]
    a[3 * rec:4 * rec] = _le(0) if compressed else _le(0, 5)
    _expect_io(lib, replaced("a_query", bytes(a)), compressed, "a_query[3]")
    b2 = bytearray(dict(ps)["b_g2_query"])
    rec2 = len(b2) // opk["n_vars"]
    b2[5 * rec2 - 1] |= 0xC0
    _expect_io(lib, replaced("b_g2_query", bytes(b2)), compressed, "b_g2_query[4]")
    vk_b = bytearray(dict(ps)["gamma_g2"])
    vk_b[-1] |= INF
    _expect_io(lib, replaced("gamma_g2", bytes(vk_b)), compressed, "vk.gamma_g2[0]")
