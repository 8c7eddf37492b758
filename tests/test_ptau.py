"""snarkjs .ptau files: cc.read_ptau / cc.write_ptau (g16_ptau_*).

The reader is tested against the library's writer AND against a file assembled here with struct from the format
description in include/g16_loaders.h, sections shuffled, with a contribution section and
the Lagrange sections of a "prepared" file present.  No .ptau written by snarkjs was at hand: nothing here pins the
format to one."""
import random
import struct

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

R = o.R_MOD
Q_LE = o.Q_MOD.to_bytes(32, "little")
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
G16_ERR_IO = 5
PAIR_TAU_G1 = 8


def _tox3(seed):
    rng = random.Random(seed)
    return [rng.randrange(2, R) for _ in range(3)]


def _py_srs(cc, k, tox):
    """the string of (tau, alpha, beta) for domain 2^k from the oracle's scalar multiplications"""
    tau, alpha, beta = tox
    n = 1 << k
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    g1 = lambda s: o.g1_to_bytes(o.G1.mul(o.G1_GEN, s % R))
    g2 = lambda s: o.g2_to_bytes(o.G2.mul(o.G2_GEN, s % R))
    arr = lambda bs, w: np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(-1, w).copy()
    return cc.Srs(arr([g1(p) for p in pw], 64), arr([g2(p) for p in pw[:n]], 128),
                  arr([g1(alpha * p) for p in pw[:n]], 64), arr([g1(beta * p) for p in pw[:n]], 64), g2(beta))


_cache = {}


def _srs3(cc):
    if "s" not in _cache:
        _cache["s"] = _py_srs(cc, 3, _tox3(73))
    return _cache["s"]


def _same_srs(a, b):
    for name in ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.beta_g2 == b.beta_g2


def _sections(srs, power, ceremony_power=None, q=Q_LE, n8=32):
    """{id: payload} of sections 1..6 for the first 2^power entries of the arrays"""
    n = 1 << power
    hdr = struct.pack("<I", n8) + q + struct.pack("<II", power, power if ceremony_power is None else ceremony_power)
    return {1: hdr, 2: srs.tau_g1[:2 * n - 1].tobytes(), 3: srs.tau_g2[:n].tobytes(), 4: srs.alpha_tau_g1[:n].tobytes(),
            5: srs.beta_tau_g1[:n].tobytes(), 6: srs.beta_g2}


def _file(sections, order=None, magic=b"ptau", version=1, n_sections=None):
    """the binfile container: magic, version u32, nSections u32, then (id u32, size u64, payload) per section;
    sections: {id: payload} or a list of (id, payload)"""
    items = list(sections.items()) if isinstance(sections, dict) else list(sections)
    if order is not None:
        items = [(i, dict(items)[i]) for i in order]
    out = magic + struct.pack("<II", version, len(items) if n_sections is None else n_sections)
    for sid, payload in items:
        out += struct.pack("<IQ", sid, len(payload)) + payload
    return out


# ---- round trip ---------------------------------------------------------------------------------------------
def test_write_read_round_trip(lib, tmp_path):
    import circom_compat_amd as cc
    srs = _srs3(cc)
    path = tmp_path / "pot3.ptau"
    cc.write_ptau(path, srs, lib=lib)
    got = cc.read_ptau(path, lib=lib)
    _same_srs(got, srs)
    assert (got.power, got.ceremony_power) == (3, 3)
    _same_srs(cc.read_ptau(path.read_bytes(), lib=lib), srs)                  # from memory
    # the writer's bytes are the independent encoding's bytes: sections 1..6 in order, then an empty section 7
    want = _file(list(_sections(srs, 3).items()) + [(7, struct.pack("<I", 0))])
    assert path.read_bytes() == want
    # a longer string is cut to the largest power it covers
    long = cc.Srs(np.vstack([srs.tau_g1, srs.tau_g1[:3]]), np.vstack([srs.tau_g2, srs.tau_g2[:2]]),
                  np.vstack([srs.alpha_tau_g1, srs.alpha_tau_g1[:1]]), np.vstack([srs.beta_tau_g1, srs.beta_tau_g1[:1]]),
                  srs.beta_g2)
    cc.write_ptau(tmp_path / "long.ptau", long, lib=lib)
    assert (tmp_path / "long.ptau").read_bytes() == want
    # a string of a smaller power out of the same arrays
    small = cc.Srs(srs.tau_g1[:7], srs.tau_g2[:4], srs.alpha_tau_g1[:4], srs.beta_tau_g1[:4], srs.beta_g2)
    cc.write_ptau(tmp_path / "pot2.ptau", small, lib=lib)
    got2 = cc.read_ptau(tmp_path / "pot2.ptau", lib=lib)
    assert got2.power == 2
    _same_srs(got2, small)


def test_reader_against_an_independent_encoding(lib, tmp_path):
    """a file assembled with struct: sections shuffled, a contribution section and the sections 12..15 of a prepared
    file present and ignored, a second copy of section 2 behind the first (the first occurrence wins), a ceremony
    power above the file's"""
    import circom_compat_amd as cc
    srs = _srs3(cc)
    sec = _sections(srs, 3, ceremony_power=12)
    rng = random.Random(5)
    junk = lambda n: bytes(rng.randrange(256) for _ in range(n))
    items = [(13, junk(8 * 128)), (5, sec[5]), (7, struct.pack("<I", 2) + junk(300)), (2, sec[2]), (12, junk(8 * 64)),
             (6, sec[6]), (1, sec[1]), (15, junk(8 * 64)), (3, sec[3]), (2, junk(len(sec[2]))), (4, sec[4]),
             (14, junk(8 * 64))]
    data = _file(items)
    got = cc.read_ptau(data, lib=lib)
    _same_srs(got, srs)
    assert (got.power, got.ceremony_power) == (3, 12)
    p = tmp_path / "shuffled.ptau"
    p.write_bytes(data)
    _same_srs(cc.read_ptau(str(p), lib=lib), srs)
    # power 0: one entry per array
    one = cc.Srs(srs.tau_g1[:1], srs.tau_g2[:1], srs.alpha_tau_g1[:1], srs.beta_tau_g1[:1], srs.beta_g2)
    got0 = cc.read_ptau(_file(_sections(one, 0)), lib=lib)
    assert got0.power == 0 and got0.tau_g1.shape == (1, 64)


# ---- rejected files -----------------------------------------------------------------------------------------
def _defects(srs):
    sec = _sections(srs, 3)
    good = _file(sec)
    without = lambda sid: {k: v for k, v in sec.items() if k != sid}
    out = [("magic", _file(sec, magic=b"zkey"), "magic"), ("version", _file(sec, version=2), "version"),
           ("prime", _file({**sec, 1: _sections(srs, 3, q=o.R_MOD.to_bytes(32, "little"))[1]}), "prime"),
           ("n8", _file({**sec, 1: struct.pack("<I", 48) + sec[1][4:]}), "n8"),
           ("power29", _file({**sec, 1: sec[1][:36] + struct.pack("<II", 29, 29)}), "power"),
           ("power_mismatch", _file({**sec, 1: sec[1][:36] + struct.pack("<II", 4, 4)}), "section 2"),
           ("short_tau_g1", _file({**sec, 2: sec[2][:-64]}), "section 2"),
           ("long_tau_g2", _file({**sec, 3: sec[3] + sec[3][:128]}), "section 3"),
           ("short_alpha", _file({**sec, 4: sec[4][:-1]}), "section 4"),
           ("short_beta", _file({**sec, 5: b""}), "section 5"),
           ("beta_g2_as_g1", _file({**sec, 6: sec[6][:64]}), "section 6"),
           ("short_header", _file({**sec, 1: sec[1][:40]}), "header"),
           ("truncated_payload", good[:-40], "past the end"), ("truncated_table", good[:len(good) - len(sec[6]) - 5], "truncated"),
           ("truncated_file_header", good[:9], "truncated"), ("empty", b"", "truncated"),
           ("more_sections_than_present", _file(sec, n_sections=7), "truncated")]
    out += [(f"missing{sid}", _file(without(sid)), f"missing section {sid}") for sid in range(1, 7)]
    return out


def test_rejected_files(lib, tmp_path):
    import circom_compat_amd as cc
    srs = _srs3(cc)
    cc.read_ptau(_file(_sections(srs, 3)), lib=lib)                          # the undamaged file reads
    for name, data, word in _defects(srs):
        with pytest.raises(cc.SerializationError) as e:
            cc.read_ptau(data, lib=lib)
        assert e.value.status == G16_ERR_IO, name
        assert e.value.message and word in e.value.message, (name, e.value.message)
        if data:
            p = tmp_path / (name + ".ptau")
            p.write_bytes(data)
            with pytest.raises(cc.SerializationError) as e:
                cc.read_ptau(str(p), lib=lib)
            assert e.value.status == G16_ERR_IO and word in e.value.message, (name, e.value.message)
    with pytest.raises(cc.SerializationError) as e:
        cc.read_ptau(str(tmp_path / "no_such_file.ptau"), lib=lib)
    assert e.value.status == G16_ERR_IO
    # the writer refuses what it cannot write
    with pytest.raises(cc.SerializationError):
        cc.write_ptau(tmp_path / "no_such_dir" / "x.ptau", srs, lib=lib)


# ---- validation and the whole chain ---------------------------------------------------------------------------
def test_read_ptau_validate(lib, tmp_path):
    import circom_compat_amd as cc
    srs = _srs3(cc)
    path = tmp_path / "pot3.ptau"
    cc.write_ptau(path, srs, lib=lib)
    _same_srs(cc.read_ptau(path, validate=True, lib=lib), srs)
    sec = _sections(srs, 3)
    # a relation fault: one tau_g1 entry is another group element
    other = o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE))
    data = _file({**sec, 2: sec[2][:64 * 9] + other + sec[2][64 * 10:]})
    assert cc.read_ptau(data, lib=lib).tau_g1.shape == (15, 64)               # unchecked: reads
    with pytest.raises(cc.G16Error) as e:
        cc.read_ptau(data, validate=True, lib=lib)
    assert "tau_g1 is not a sequence of powers of tau" in e.value.message
    assert not isinstance(e.value, cc.SerializationError)
    # a structural fault: one flipped bit in tau_g2[2]
    flipped = bytearray(sec[3])
    flipped[128 * 2 + 70] ^= 0x10
    p = tmp_path / "flipped.ptau"
    p.write_bytes(_file({**sec, 3: bytes(flipped)}))
    with pytest.raises(cc.G16Error) as e:
        cc.read_ptau(str(p), validate=True, lib=lib)
    assert "tau_g2[2]" in e.value.message


def test_ptau_to_key_end_to_end(lib, tmp_path):
    """write_ptau -> read_ptau(validate=True) -> setup_from_srs gives the key of the in-memory string, byte for byte;
    a contribution to it is a key of the circuit under the ceremony read from the file"""
    import circom_compat_amd as cc
    cons, _w, n_vars, n_pub = H.squaring_chain(4)
    csrs = tuple(cc.Csr.from_rows([[(cf, idx) for idx, cf in row[j]] for row in cons], lib) for j in range(3))
    mem = cc.trapdoor_srs(4, _tox3(74), lib=lib)
    path = tmp_path / "pot4.ptau"
    cc.write_ptau(path, mem, lib=lib)
    srs = cc.read_ptau(path, validate=True, lib=lib)
    assert srs.power == 4
    _same_srs(srs, mem)
    want = cc.setup_from_srs(*csrs, n_vars, n_pub, mem, lib=lib)
    got = cc.setup_from_srs(*csrs, n_vars, n_pub, srs, lib=lib)
    assert (got.n_vars, got.n_public, got.domain_size) == (want.n_vars, want.n_public, want.domain_size)
    for name in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query"):
        assert np.array_equal(np.asarray(getattr(got, name)), np.asarray(getattr(want, name))), name
    for name in ("beta_g1", "delta_g1"):
        assert bytes(getattr(got, name)) == bytes(getattr(want, name)), name
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert bytes(getattr(got.vk, name)) == bytes(getattr(want.vk, name)), name
    assert np.array_equal(np.asarray(got.vk.gamma_abc_g1), np.asarray(want.vk.gamma_abc_g1))
    key1 = cc.contribute_key(got, 0x5EED0FACADE, lib=lib)
    assert cc.check_key_circuit(key1, *csrs, srs, lib=lib).ok
    assert cc.check_key_circuit(got, *csrs, srs, lib=lib).ok
