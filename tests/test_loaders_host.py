"""The four file parsers of csrc/loaders.cpp (.zkey, .r1cs, .wtns, .ptau) and the .zkey writer are pure host code over
bytes the caller does not control.  They are compiled here, together with the stand-alone tests/loaders/loaders_main.cpp,
twice: by g++ with -fsanitize=address,undefined, and plain with an operator new that refuses any single request above
4 x the file under test + 64 KiB (a count believed from a header is then an exception inside the loader, which has to
come back as a status).  The program writes its own minimal files and walks every truncation, section-table and
header-count mutation, duplicate and permuted sections and the edges of the field; see its header comment.  No GPU code
runs and nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "circom_compat_amd", "csrc", "loaders.cpp"),
           os.path.join(ROOT, "tests", "loaders", "loaders_main.cpp")]


def _build_and_run(tmp_path, name, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the library anyway"
    exe = str(tmp_path / name)
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", *flags, *SOURCES, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b", r.stderr):   # the linker's wording only
        pytest.skip("the sanitizer runtime is not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    groups = [ln for ln in r.stdout.splitlines() if ln.startswith("# ")]
    died = re.findall(r"ABORTED in case: (.*)", r.stderr)
    last = died[-1] if died else (groups[-1] if groups else "(nothing printed)")
    assert r.returncode == 0, (f"exit status {r.returncode}; last case: {last}", r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert m, r.stdout[-1000:]
    assert int(m.group(2)) == 0, r.stderr[-4000:]
    assert int(m.group(1)) >= 5000, r.stdout[-1000:]       # the truncations of the zkey alone are about 3000
    return r.stdout


def test_parsers_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "loaders_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_parsers_under_an_allocation_bound(tmp_path):
    out = _build_and_run(tmp_path, "loaders_bound", ["-DLOADERS_ALLOC_BOUND"])
    assert "# allocation bound" in out                      # the replaced operator new is in this build


# ---- the same kinds of file through the Python surface ----------------------------------------------------------------
# Hostile files made from the golden fixtures by patching bytes.  Each must raise SerializationError -- not abort, not
# hand out a view -- and the golden file still loads, in the same process, afterwards.
import struct  # noqa: E402

R_LE = bytes.fromhex("30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001")[::-1]
Q_LE = bytes.fromhex("30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47")[::-1]


def _sections(data):
    """[(id, offset of the (id, size) entry, offset of the payload, size)] of a binfile container"""
    n = struct.unpack_from("<I", data, 8)[0]
    out, at = [], 12
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", data, at)
        out.append((sid, at, at + 12, size))
        at += 12 + size
    assert at == len(data)
    return out


def _payload(data, sid):
    return next(p for s, _e, p, _n in _sections(data) if s == sid)


def _poke(data, at, fmt, *values):
    d = bytearray(data)
    struct.pack_into(fmt, d, at, *values)
    return bytes(d)


def _append_section(data, sid, payload):
    d = bytearray(data) + struct.pack("<IQ", sid, len(payload)) + payload
    struct.pack_into("<I", d, 8, struct.unpack_from("<I", data, 8)[0] + 1)
    return bytes(d)


def _ptau(power=2, header_power=None):
    """a .ptau of arbitrary point bytes (the loader looks at none)"""
    n = 1 << power
    hp = power if header_power is None else header_power
    secs = [(1, struct.pack("<I", 32) + Q_LE + struct.pack("<II", hp, hp)), (2, bytes([2]) * ((2 * n - 1) * 64)),
            (3, bytes([3]) * (n * 128)), (4, bytes([4]) * (n * 64)), (5, bytes([5]) * (n * 64)), (6, bytes([6]) * 128),
            (7, struct.pack("<I", 0))]
    out = b"ptau" + struct.pack("<II", 1, len(secs))
    for sid, p in secs:
        out += struct.pack("<IQ", sid, len(p)) + p
    return out


def _hostile_files(golden):
    rd = lambda name: open(os.path.join(golden, name), "rb").read()
    r1cs, zkey, wtns, ptau = rd("circuit2.r1cs"), rd("test.zkey"), rd("circuit2.wtns"), _ptau()
    h = _payload(r1cs, 1)                       # field_size, prime, n_wires +36, n_pub_out +40, n_pub_in +44, ..., n_constraints +60
    c = next(s for s in _sections(r1cs) if s[0] == 2)
    zh = _payload(zkey, 2)                      # n8q, q, n8r, r, n_vars +72, n_public +76, domain_size +80
    z4 = next(s for s in _sections(zkey) if s[0] == 4)
    w1, w2 = _payload(wtns, 1), _payload(wtns, 2)
    # a second constraint section, behind the first, that ends inside its first coefficient: the last one wins
    short2 = struct.pack("<II", 1, 0) + bytes(16)
    return [
        ("r1cs", "n_constraints = 2^32 - 1", _poke(r1cs, h + 60, "<I", 0xFFFFFFFF)),
        ("r1cs", "n_constraints = 2^31", _poke(r1cs, h + 60, "<I", 1 << 31)),
        ("r1cs", "n_pub_out = 2^31 - 1", _poke(r1cs, h + 40, "<I", 0x7FFFFFFF)),
        ("r1cs", "n_pub_in = 2^32 - 1", _poke(r1cs, h + 44, "<I", 0xFFFFFFFF)),
        ("r1cs", "constraint section of size ~0", _poke(r1cs, c[1] + 4, "<Q", (1 << 64) - 1)),
        ("r1cs", "duplicate section 2", _append_section(r1cs, 2, short2)),
        ("r1cs", "coefficient = r", r1cs[:c[2] + 8] + R_LE + r1cs[c[2] + 40:]),
        ("zkey", "section 4 of size ~0", _poke(zkey, z4[1] + 4, "<Q", (1 << 64) - 1)),
        ("zkey", "n_public = 2^32 - 1", _poke(zkey, zh + 76, "<I", 0xFFFFFFFF)),
        ("zkey", "n_vars = 2^32 - 1", _poke(zkey, zh + 72, "<I", 0xFFFFFFFF)),
        ("zkey", "coefficient count = 2^32 - 1", _poke(zkey, z4[2], "<I", 0xFFFFFFFF)),
        ("wtns", "value = r", wtns[:w2 + 32] + R_LE + wtns[w2 + 64:]),
        ("wtns", "value count = 2^32 - 1", _poke(wtns, w1 + 36, "<I", 0xFFFFFFFF)),
        ("ptau", "power 29", _ptau(header_power=29)),
        ("ptau", "power 2^32 - 1", _ptau(header_power=0xFFFFFFFF)),
        ("ptau", "section 2 of size ~0", _poke(ptau, _sections(ptau)[1][1] + 4, "<Q", (1 << 64) - 1)),
    ]


def test_hostile_files_raise_and_the_golden_files_still_load(gpulib, golden):
    import numpy as np
    import circom_compat_amd as cc
    import bn254_ref as o
    import helpers as H
    assert R_LE == o.R1CS_PRIME_LE and Q_LE == o.Q_MOD.to_bytes(32, "little")
    readers = {"r1cs": lambda d: cc.R1CS(cc.R1CSFile(d, lib=gpulib)), "zkey": lambda d: cc.read_zkey(d, lib=gpulib),
               "wtns": lambda d: cc.read_wtns(d, lib=gpulib), "ptau": lambda d: cc.read_ptau(d, lib=gpulib)}
    rd = lambda name: open(os.path.join(golden, name), "rb").read()
    good = {"r1cs": rd("circuit2.r1cs"), "zkey": rd("test.zkey"), "wtns": rd("circuit2.wtns"), "ptau": _ptau()}
    files = _hostile_files(golden)
    assert len(files) >= 12 and {k for k, _n, _d in files} == set(readers)
    for kind, name, data in files:
        assert data != good[kind], name
        with pytest.raises(cc.SerializationError) as e:
            readers[kind](data)
        assert e.value.status == 5 and e.value.message, (kind, name)       # G16_ERR_IO with a reason
    # still alive, and the undamaged files load to what they held before
    r1 = readers["r1cs"](good["r1cs"])
    ref = o.read_r1cs(good["r1cs"])
    assert (r1.num_inputs, r1.num_variables, r1.num_aux) == (2, ref["n_wires"], ref["n_wires"] - 2)
    assert r1.num_constraints == len(ref["constraints"]) == 131
    assert [int(x) for x in r1.a.col] == [wdx for con in ref["constraints"] for wdx, _cf in con[0]]
    pk, mats = readers["zkey"](good["zkey"])
    assert (pk.n_vars, pk.n_public, pk.domain_size, mats.num_constraints) == (4, 1, 4, 1)
    assert H.fr_from_mont_arr(readers["wtns"](good["wtns"])) == o.read_wtns(good["wtns"])
    srs = readers["ptau"](good["ptau"])
    assert srs.power == 2 and srs.tau_g1.shape == (7, 64) and srs.tau_g2.shape == (4, 128)
    assert np.all(np.asarray(srs.tau_g1) == 2) and srs.beta_g2 == bytes([6]) * 128


def test_r1cs_num_aux_never_wraps(gpulib, golden):
    """every 32-bit value in each of the three counts num_aux is made of: R1CSFile either refuses the header or
    R1CS.num_aux is n_wires - num_inputs >= 0, in the header the library hands out and in Python alike"""
    import circom_compat_amd as cc
    data = open(os.path.join(golden, "mycircuit.r1cs"), "rb").read()
    h = _payload(data, 1)
    n_wires = struct.unpack_from("<I", data, h + 36)[0]
    accepted = 0
    for off in (36, 40, 44):
        was = struct.unpack_from("<I", data, h + off)[0]
        for v in (0, 1, 2, was - 1, was + 1, n_wires, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
            try:
                f = cc.R1CSFile(_poke(data, h + off, "<I", v & 0xFFFFFFFF), lib=gpulib)
            except cc.SerializationError:
                continue
            accepted += 1
            r = cc.R1CS(f)
            hd = f.header
            assert r.num_inputs == 1 + hd.n_pub_in + hd.n_pub_out == hd.num_inputs <= hd.n_wires
            assert 0 <= r.num_aux == hd.n_wires - r.num_inputs == hd.num_aux
    assert accepted >= 3                                    # the unharmful values of n_pub_out / n_pub_in
