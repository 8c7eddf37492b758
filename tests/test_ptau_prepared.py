"""Prepared snarkjs .ptau files: cc.write_ptau(lagrange=) / cc.read_ptau(lagrange=True) (g16_ptau_write_prepared,
g16_ptau_lagrange).

As in tests/test_ptau.py the reader is tested against the library's writer AND against a file assembled here with
struct from the description in include/g16_loaders.h and include/g16_amd.h.  No prepared .ptau written by snarkjs was
at hand: nothing here pins sections 12-15 to one."""
import random
import struct

import numpy as np
import pytest

import bn254_ref as o
from test_ptau import G16_ERR_IO, _file, _same_srs, _sections

R = o.R_MOD
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
POWER = 3
_cache = {}


def _pair(cc, lib):
    """(srs, LagrangeSrs) of power 3, once per library"""
    if id(lib) not in _cache:
        rng = random.Random(91)
        srs = cc.trapdoor_srs(POWER, [rng.randrange(2, R) for _ in range(3)], lib=lib)
        _cache[id(lib)] = (srs, cc.prepare_phase2(srs, lib=lib))
    return _cache[id(lib)]


def _same_set(a, b):
    assert a.power == b.power
    for name in ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def _lag_sections(lag):
    return {12: lag.tau_g1.tobytes(), 13: lag.tau_g2.tobytes(), 14: lag.alpha_tau_g1.tobytes(),
            15: lag.beta_tau_g1.tobytes()}


def test_write_read_round_trip(lib, tmp_path):
    import circom_compat_amd as cc
    srs, lag = _pair(cc, lib)
    path = tmp_path / "pot3_prepared.ptau"
    cc.write_ptau(path, srs, lagrange=lag, lib=lib)
    got = cc.read_ptau(path, lagrange=True, lib=lib)
    _same_srs(got, srs)
    assert (got.power, got.ceremony_power) == (POWER, POWER)
    _same_set(got.lagrange, lag)
    assert got.lagrange.level("tau_g1", POWER + 1).shape == (16, 64)
    _same_set(cc.read_ptau(path.read_bytes(), lagrange=True, lib=lib).lagrange, lag)      # from memory
    plain = cc.read_ptau(path, lib=lib)                                                    # the default reader
    _same_srs(plain, srs)
    assert not hasattr(plain, "lagrange")
    # the writer's bytes are the independent encoding's: sections 1..6, an empty section 7, then 12..15
    want = _file(list(_sections(srs, POWER).items()) + [(7, struct.pack("<I", 0))] + list(_lag_sections(lag).items()))
    assert path.read_bytes() == want
    assert cc.read_ptau(path, validate=True, lagrange=True, lib=lib).lagrange.power == POWER
    # the file has the power of the Lagrange set: a longer string is cut to it, a shorter one refused
    lag2 = cc.prepare_phase2(srs, power=2, lib=lib)
    cc.write_ptau(tmp_path / "pot2.ptau", srs, lagrange=lag2, lib=lib)
    got2 = cc.read_ptau(tmp_path / "pot2.ptau", validate=True, lagrange=True, lib=lib)
    assert got2.power == 2 and got2.tau_g1.shape[0] == 7
    _same_set(got2.lagrange, lag2)
    small = cc.Srs(srs.tau_g1[:7], srs.tau_g2[:4], srs.alpha_tau_g1[:4], srs.beta_tau_g1[:4], srs.beta_g2)
    with pytest.raises(cc.G16Error):
        cc.write_ptau(tmp_path / "no.ptau", small, lagrange=lag, lib=lib)
    # an unprepared file is refused by the reader when the sections are asked for
    cc.write_ptau(tmp_path / "plain.ptau", srs, lib=lib)
    with pytest.raises(cc.G16Error) as e:
        cc.read_ptau(tmp_path / "plain.ptau", lagrange=True, lib=lib)
    assert e.value.status == G16_ERR_IO and "not prepared" in str(e.value)


def test_reader_against_an_independent_encoding(lib):
    """a file assembled with struct, sections shuffled, a second copy of section 13 behind the first"""
    import circom_compat_amd as cc
    srs, lag = _pair(cc, lib)
    sec = dict(_sections(srs, POWER, ceremony_power=12))
    sec.update(_lag_sections(lag))
    rng = random.Random(6)
    junk = lambda n: bytes(rng.randrange(256) for _ in range(n))
    order = [14, 5, 12, 2, 6, 15, 1, 3, 13, 4]
    items = [(i, sec[i]) for i in order] + [(7, struct.pack("<I", 1) + junk(100)), (13, junk(len(sec[13])))]
    got = cc.read_ptau(_file(items), lagrange=True, lib=lib)
    _same_srs(got, srs)
    assert (got.power, got.ceremony_power) == (POWER, 12)
    _same_set(got.lagrange, lag)


@pytest.mark.parametrize("case", ["12_has_13s_size", "12_missing", "13_missing", "14_missing", "15_missing"])
def test_bad_lagrange_sections_matter_only_when_asked_for(lib, case):
    import circom_compat_amd as cc
    srs, lag = _pair(cc, lib)
    sec = dict(_sections(srs, POWER))
    sec.update(_lag_sections(lag))
    if case == "12_has_13s_size":
        sec[12] = sec[12][:len(sec[13])]
        assert len(sec[12]) == len(sec[13]) == 15 * 128
        words = ("section 12", str(15 * 128), str(31 * 64))
    else:
        gone = int(case.split("_")[0])
        del sec[gone]
        words = (f"missing section {gone}", "not prepared")
    data = _file(sec)
    _same_srs(cc.read_ptau(data, lib=lib), srs)                       # accepted by the default reader
    with pytest.raises(cc.G16Error) as e:
        cc.read_ptau(data, lagrange=True, lib=lib)
    assert e.value.status == G16_ERR_IO
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_validate_names_a_flipped_lagrange_byte(lib, tmp_path):
    import circom_compat_amd as cc
    srs, lag = _pair(cc, lib)
    path = tmp_path / "pot3_prepared.ptau"
    cc.write_ptau(path, srs, lagrange=lag, lib=lib)
    raw = bytearray(path.read_bytes())
    at = bytes(raw).index(lag.alpha_tau_g1.tobytes()) + 5 * 64 + 3     # entry 5 of section 14: level 2, entry 2
    raw[at] ^= 0x10
    assert cc.read_ptau(bytes(raw), lagrange=True, lib=lib).lagrange is not None      # not looked at
    assert cc.read_ptau(bytes(raw), validate=True, lib=lib).power == POWER            # nor without lagrange=True
    with pytest.raises(cc.G16Error) as e:
        cc.read_ptau(bytes(raw), validate=True, lagrange=True, lib=lib)
    assert "alpha_tau_g1 level 2 entry 2" in str(e.value) and "off the curve" in str(e.value)
