"""Canonical witness ingestion: k_fr_from_canonical against the host conversion, its range report, and the
*_canonical provers against prove() on the witness read_wtns converts on the host -- byte for byte, on the golden
keys, on the table and bucket paths, batched, resident and on a repeated-ordinal multi-device ctx; open_wtns'
header rules and messages against read_wtns'."""
import ctypes as C
import json
import os
import random
import struct

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

R = o.R_MOD
G16_ERR_INVALID = 1
FIXED_R = 3413513218498352040262653353725127729454431939539290118844322056224532443637
FIXED_S = 6077776500692565155461894309070795882353485867345896979329447163197530625403


def _le(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def _special_values():
    rng = random.Random(4242)
    vals = [0, 1, 2, R - 1, R - 2, 1 << 253, (1 << 64) - 1, (1 << 256) % R, (1 << 512) % R]
    return vals + [rng.randrange(R) for _ in range(58)]


def _convert(lib, le, first_bad=True):
    le = np.ascontiguousarray(le, dtype=np.uint8)
    n = le.size // 32
    out = np.full((max(n, 1), 4), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    bad = C.c_int64(-7)
    st = lib.g16_fr_convert(0, le.ctypes.data, out.ctypes.data, n, C.byref(bad) if first_bad else None)
    return st, out[:n], bad.value


# ---- the kernel ---------------------------------------------------------------------------------------------------
def test_kernel_equals_host_conversion(lib):
    """67 elements -- a full wave and a 3-lane tail -- bit-equal to g16_fr_from_canonical; n = 0 and n = 1"""
    vals = _special_values()
    assert len(vals) == 67
    le = _le(vals)
    want = np.empty((67, 4), dtype=np.uint64)
    assert lib.g16_fr_from_canonical(le.ctypes.data, want.ctypes.data, 67) == 0
    st, got, bad = _convert(lib, le)
    assert st == 0 and bad == -1
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == H.fr_mont_arr(vals).tobytes()          # and to the oracle's Montgomery form
    st, got, bad = _convert(lib, le[:1])
    assert st == 0 and bad == -1 and got.tobytes() == want[:1].tobytes()
    st, got, bad = _convert(lib, le[:0])
    assert st == 0 and bad == -1
    assert lib.g16_fr_convert(0, None, None, 0, None) == 0


def test_range_report(lib):
    """the smallest index of a value >= r comes back, whatever the schedule; NULL first_bad: the same status"""
    vals = _special_values() + [7]
    assert len(vals) == 68
    two = list(vals)
    two[5], two[67] = R, (1 << 256) - 1
    st, _, bad = _convert(lib, _le(two))
    assert st == G16_ERR_INVALID and bad == 5
    assert b"5" in lib.g16_last_error(None)
    last = list(vals)
    last[67] = R + 1
    st, _, bad = _convert(lib, _le(last))
    assert st == G16_ERR_INVALID and bad == 67
    st, _, _ = _convert(lib, _le(last), first_bad=False)
    assert st == G16_ERR_INVALID
    st, _, bad = _convert(lib, _le(vals))
    assert st == 0 and bad == -1


def test_python_fr_from_canonical(lib):
    import circom_compat_amd as cc
    vals = _special_values()
    assert cc.fr_from_canonical(vals, lib=lib).tobytes() == H.fr_mont_arr(vals).tobytes()
    assert cc.fr_from_canonical(_le(vals), lib=lib).tobytes() == H.fr_mont_arr(vals).tobytes()
    with pytest.raises(cc.G16Error) as e:
        cc.fr_from_canonical(vals[:3] + [R] + vals[3:], lib=lib)
    assert e.value.status == G16_ERR_INVALID and e.value.first_bad == 3


# ---- provers ------------------------------------------------------------------------------------------------------
def _chain_key(lib, k, seed):
    import circom_compat_amd as cc
    cons, w, n_vars, n_pub = H.squaring_chain(k)
    rng = random.Random(seed)
    opk = o.trapdoor_setup(cons, n_vars, n_pub, *[rng.randrange(1, R) for _ in range(5)])
    a_rows, b_rows = o.matrices_from_r1cs(cons)
    return H.pk_from_oracle(opk), H.matrices_from_rows(a_rows, b_rows, 2, n_vars, lib), n_vars


def _chain_witness(k, x0):
    return H.squaring_chain(k, x0=x0)[1]


def _check(cc, lib, pk, pr, path, tmp=None):
    """prove_wtns(path) == prove(read_wtns(path)) with fixed (r, s), from every accepted form of the witness, and the
    proof verifies with Witness.public_inputs"""
    want = pr.prove(FIXED_R, FIXED_S, cc.read_wtns(path, lib=lib))
    wt = cc.open_wtns(path, lib=lib)
    for src in (path, open(path, "rb").read(), wt, np.array(wt.canonical)):
        assert pr.prove_wtns(src, FIXED_R, FIXED_S).raw == want.raw
    assert cc.verify_batch(pk.vk, [want], [wt.public_inputs(pk.n_public)], lib=lib) == [True]
    assert pr.prove_wtns(wt).raw != want.raw          # r, s drawn
    return want


def test_prove_wtns_golden_zkey(lib, golden, tmp_path):
    """test.zkey (4 wires): the witness of mycircuit-witness.json through write_wtns"""
    import circom_compat_amd as cc
    pk, mats = cc.read_zkey(os.path.join(golden, "test.zkey"), lib=lib)
    w = [int(x) for x in json.load(open(os.path.join(golden, "mycircuit-witness.json")))]
    path = str(tmp_path / "my.wtns")
    cc.write_wtns(path, w)
    pr = cc.Prover(pk, mats, lib=lib)
    _check(cc, lib, pk, pr, path)
    pr.close()


def test_prove_wtns_circuit2_snarkjs_file(lib, golden):
    """circuit2.r1cs with circuit2.wtns, a file snarkjs wrote (132 wires); key from trapdoor_setup"""
    import circom_compat_amd as cc
    r1cs = cc.R1CS.from_file(os.path.join(golden, "circuit2.r1cs"), lib=lib)
    pk = cc.trapdoor_setup(r1cs.a, r1cs.b, r1cs.c, r1cs.num_variables, r1cs.num_inputs - 1, [11, 22, 33, 44, 55], lib=lib)
    pr = cc.Prover(pk, r1cs.matrices(), lib=lib)
    path = os.path.join(golden, "circuit2.wtns")
    assert cc.open_wtns(path, lib=lib).n == 132
    _check(cc, lib, pk, pr, path)
    pr.close()


# (the emulator builds the fixed-base tables of a 64-wire key in minutes: the table cases carry the slow mark)
TABLES = [pytest.param(1, marks=pytest.mark.slow), -1]


@pytest.mark.parametrize("tables", TABLES)
def test_prove_wtns_chain_tables_and_buckets(lib, tmp_path, tables):
    import circom_compat_amd as cc
    pk, mats, n_vars = _chain_key(lib, 6, 61)
    path = str(tmp_path / "chain.wtns")
    cc.write_wtns(path, _chain_witness(6, 3))
    pr = cc.Prover(pk, mats, lib=lib, tables=tables)
    assert pr.info()["fixed_tables"] == (1 if tables == 1 else 0)
    _check(cc, lib, pk, pr, path)
    # a value >= r: an error naming the element, no proof
    bad = _le(_chain_witness(6, 3))
    bad[9] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
    with pytest.raises(cc.G16Error) as e:
        pr.prove_wtns(bad, FIXED_R, FIXED_S)
    assert e.value.status == G16_ERR_INVALID and "element 9" in str(e.value)
    pr.close()


@pytest.mark.parametrize("tables", TABLES)
def test_prove_wtns_batch(lib, tables):
    """3 distinct chain witnesses (16 wires: the smallest chain with an element 9) on a table ctx and on a bucket ctx
    == the loop of prove(); then witness 1's element 9 set to r: an error naming proof 1 and element 9, first_bad =
    n_vars + 9"""
    import circom_compat_amd as cc
    pk, mats, n_vars = _chain_key(lib, 4, 62)
    pr = cc.Prover(pk, mats, lib=lib, tables=tables)
    assert pr.info()["fixed_tables"] == (1 if tables == 1 else 0) and pr.info()["batched"] == 1
    ws = [_chain_witness(4, x0) for x0 in (3, 4, 5)]
    rng = random.Random(63)
    rs = [(rng.randrange(R), rng.randrange(R)) for _ in ws]
    want = [pr.prove(r, s, w).raw for (r, s), w in zip(rs, ws)]
    les = [_le(w) for w in ws]
    assert [p.raw for p in pr.prove_wtns_batch(les, rs)] == want
    assert pr.prove_wtns_batch([], []) == []
    les[1][9] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
    with pytest.raises(cc.G16Error) as e:
        pr.prove_wtns_batch(les, rs)
    assert e.value.status == G16_ERR_INVALID and e.value.first_bad == n_vars + 9
    assert "proof 1" in str(e.value) and "element 9" in str(e.value)
    # the C call leaves proofs_out alone
    w = np.ascontiguousarray(np.stack(les))
    r, s = pr._batch_rs(rs)
    out = np.full(3 * 256, 0xee, dtype=np.uint8)
    st = lib.g16_prove_batch_canonical(pr.ctx, 3, r.ctypes.data, s.ctypes.data, w.ctypes.data, n_vars, out.ctypes.data, None)
    assert st == G16_ERR_INVALID and (out == 0xee).all()
    pr.close()


def test_resident_canonical_witness(lib):
    """upload_witness_canonical, then prove_dev from the ctx's buffer"""
    import circom_compat_amd as cc
    pk, mats, n_vars = _chain_key(lib, 6, 64)
    pr = cc.Prover(pk, mats, lib=lib)
    w = _chain_witness(6, 7)
    want = pr.prove(FIXED_R, FIXED_S, w).raw
    ptr = pr.upload_witness_canonical(_le(w))
    assert ptr and pr.prove_dev(FIXED_R, FIXED_S, ptr).raw == want
    bad = _le(w)
    bad[n_vars - 1] = 0xff
    with pytest.raises(cc.G16Error) as e:
        pr.upload_witness_canonical(bad)
    assert e.value.first_bad == n_vars - 1
    pr.close()


def test_multi_device_canonical(lib):
    """a devices=[0, 0] ctx converts on its first device and broadcasts: the single-device bytes"""
    import circom_compat_amd as cc
    pk, mats, n_vars = _chain_key(lib, 6, 65)
    w = _chain_witness(6, 5)
    one = cc.Prover(pk, mats, lib=lib)
    want = one.prove(FIXED_R, FIXED_S, w).raw
    one.close()
    multi = cc.Prover(pk, mats, lib=lib, devices=[0, 0])
    assert multi.prove_wtns(_le(w), FIXED_R, FIXED_S).raw == want
    assert multi.prove_dev(FIXED_R, FIXED_S, multi.upload_witness_canonical(_le(w))).raw == want
    assert [p.raw for p in multi.prove_wtns_batch([_le(w), _le(w)], [(FIXED_R, FIXED_S)] * 2)] == [want, want]
    bad = _le(w)
    bad[4] = 0xff
    with pytest.raises(cc.G16Error) as e:
        multi.prove_wtns(bad, FIXED_R, FIXED_S)
    assert "element 4" in str(e.value)
    multi.close()


# ---- the loader ---------------------------------------------------------------------------------------------------
def _wtns(values, magic=b"wtns", n8=32, prime=R, n=None, sec2=None, cut=None):
    body = b"".join(int(v).to_bytes(32, "little") for v in values)
    if sec2 is not None:
        body = body[:sec2]
    hdr = struct.pack("<I", n8) + prime.to_bytes(n8, "little") + struct.pack("<I", len(values) if n is None else n)
    blob = magic + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(hdr)) + hdr + struct.pack("<IQ", 2, len(body)) + body
    return blob if cut is None else blob[:cut]


@pytest.mark.parametrize("kw", [dict(magic=b"wtnz"), dict(n8=64), dict(prime=o.Q_MOD), dict(sec2=32 * 3 - 1), dict(cut=90)],
                         ids=["magic", "n8", "prime", "short-section", "truncated"])
def test_open_wtns_rejections_carry_read_wtns_messages(gpulib, tmp_path, kw):
    import circom_compat_amd as cc
    blob = _wtns([1, 2, 3], **kw)
    with pytest.raises(cc.SerializationError) as want:
        cc.read_wtns(blob, lib=gpulib)
    path = str(tmp_path / "bad.wtns")
    open(path, "wb").write(blob)
    for src in (blob, path):
        with pytest.raises(cc.SerializationError) as got:
            cc.open_wtns(src, lib=gpulib)
        assert got.value.status == want.value.status and got.value.message == want.value.message
    assert want.value.message.startswith("wtns: ")


def test_open_wtns_is_the_files_bytes(gpulib, golden, tmp_path):
    import circom_compat_amd as cc
    path = os.path.join(golden, "circuit2.wtns")
    raw = open(path, "rb").read()
    for src in (path, raw):
        wt = cc.open_wtns(src, lib=gpulib)
        assert wt.n == 132 and wt.canonical.shape == (132, 32)
        assert wt.canonical.tobytes() == raw[-132 * 32:]
        assert not wt.canonical.flags.writeable
        assert wt.public_inputs(1) == o.read_wtns(raw)[1:2]
    with pytest.raises(cc.SerializationError):
        cc.open_wtns(str(tmp_path / "absent.wtns"), lib=gpulib)


def test_write_wtns_round_trips_through_read_wtns(gpulib, tmp_path):
    import circom_compat_amd as cc
    vals = _special_values()
    path = str(tmp_path / "v.wtns")
    cc.write_wtns(path, vals)
    assert H.fr_from_mont_arr(cc.read_wtns(path, lib=gpulib)) == vals
    assert o.read_wtns(open(path, "rb").read()) == vals
    cc.write_wtns(path, _le(vals))
    assert H.fr_from_mont_arr(cc.read_wtns(path, lib=gpulib)) == vals
    assert cc.open_wtns(path, lib=gpulib).canonical.tobytes() == _le(vals).tobytes()
