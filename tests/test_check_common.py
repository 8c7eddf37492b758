"""The streamed point-check core that g16_key_check, g16_key_contribution_check, g16_srs_check and
g16_srs_lagrange_check share (csrc/keycheck.h): flags, the collect scan, the offsets and the list assembly.

With a caller-supplied rho the four checks are deterministic, so every field of every report and every entry of
every bad-point list is compared with tests/golden/check_reports.json.  That file is the project's own output: it
was recorded (`PYTHONPATH=.:oracle python tests/test_check_common.py`, on the emulator build) at the commit BEFORE the four copies of
the core were merged into one, so the test pins the scan, cap and concatenation logic to what the separate
copies computed.  The expectations of what a report SHOULD say (planted faults, oracle verdicts) live in the
checks' own test files; the inputs here only have to reach every branch of the shared code:

  clean       nothing planted
  seam        a malformed point in the last entry of a chunk and in the first of the next, in two queries
  infinity    one point at infinity
  wrong       a valid point in the wrong place: a relation fails, no structural failure
  many        more bad points than max_listed, over two queries; the cut falls inside the second query's region
              and the second query alone has more than max_listed (the per-query cap of the collect scan)
  many_full   the same input with room for all of them
  many_none   the same input with max_listed = 0

Shapes are those of the neighbours: the 64-wire chain key in chunks of 16 (check) / 24 (contribution), a string
of power 4 in chunks of 5."""
import json
import os
import random

import numpy as np
import pytest

import bn254_ref as o
import test_key_check as TK
import test_key_contribute as TC
from test_verify import _twist_point_outside_g2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "check_reports.json")
CASES = ("clean", "seam", "infinity", "wrong", "many", "many_full", "many_none")
CHECKS = ("key", "contribution", "srs", "lagrange")
ENV = dict(G16_KEYCHECK_CHUNK="16", G16_CONTRIB_CHUNK="24", G16_SRSCHECK_CHUNK="5", G16_LAGCHECK_CHUNK="5")
POWER = 4
MANY_LISTED = 5
R = o.R_MOD


def _rho(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


def _spoil(arr, i, kind):
    """row i of a point array: "noncanon" x + q, "offcurve" y + 1, "cofactor" (G2) on the twist outside G2"""
    raw = bytes(arr[i])
    assert any(raw), i
    half = len(raw) // 2
    if kind == "noncanon":
        v = int.from_bytes(raw[:32], "little") + o.Q_MOD
        assert v < 1 << 256
        raw = v.to_bytes(32, "little") + raw[32:]
    elif kind == "offcurve":
        v = int.from_bytes(raw[half:half + 32], "little") + 1
        assert v < o.Q_MOD
        raw = raw[:half] + v.to_bytes(32, "little") + raw[half + 32:]
    else:
        assert kind == "cofactor" and len(raw) == 128
        raw = o.g2_to_bytes(_twist_point_outside_g2(1 + i))
    arr[i] = np.frombuffer(raw, dtype=np.uint8)


def _other(width, salt):
    """a valid point that belongs nowhere"""
    if width == 128:
        return np.frombuffer(o.g2_to_bytes(o.G2.mul(o.G2_GEN, 0xC0FFEE + salt)), dtype=np.uint8)
    return np.frombuffer(o.g1_to_bytes(o.G1.mul(o.G1_GEN, 0xC0FFEE + salt)), dtype=np.uint8)


def _edit(case, first, second, seam):
    """apply a case to two point arrays of one check (`second` may be G2); seam: the chunk size"""
    if case == "seam":
        for arr, kinds in ((first, ("noncanon", "offcurve")), (second, ("offcurve", "noncanon"))):
            _spoil(arr, seam - 1, kinds[0])
            _spoil(arr, seam, kinds[1])
    elif case == "infinity":
        first[seam + 2] = 0
    elif case == "wrong":
        second[seam + 1] = _other(second.shape[1], seam)
    elif case.startswith("many"):
        for i, kind in ((0, "offcurve"), (seam - 1, "noncanon"), (2 * seam, "offcurve")):
            _spoil(first, i, kind)
        g2 = second.shape[1] == 128
        for n, i in enumerate((2, seam - 1, seam, seam + 1, 2 * seam - 1, 2 * seam, 2 * seam + 3)):
            _spoil(second, i, ("cofactor" if g2 else "offcurve") if n % 2 else "noncanon")
    else:
        assert case == "clean"


def _listed(case):
    return {"many": MANY_LISTED, "many_none": 0}.get(case, 64)


def _plain(rep):
    """every attribute of a report object, as JSON holds it"""
    return json.loads(json.dumps(vars(rep)))


_srs_cache, _pair_cache = {}, {}


def _string(cc, lib):
    """(srs, Lagrange set) of power 4 with writable arrays of their own"""
    if id(lib) not in _srs_cache:
        rng = random.Random(4040)
        srs = cc.trapdoor_srs(POWER, [rng.randrange(2, R) for _ in range(3)], lib=lib)
        _srs_cache[id(lib)] = (srs, cc.prepare_phase2(srs, power=POWER, lib=lib))
    srs, lag = _srs_cache[id(lib)]
    names = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
    return (cc.Srs(*(np.array(getattr(srs, a), dtype=np.uint8, copy=True) for a in names), srs.beta_g2),
            cc.LagrangeSrs(lag.power, *(np.array(getattr(lag, a), dtype=np.uint8, copy=True) for a in names)))


def run_case(cc, lib, check, case):
    """the report of one check on one case, as plain data; the G16_*_CHUNK values of ENV must be set"""
    if check == "key":
        pk = TK._chain_key(cc, lib)
        assert all(any(bytes(pk.b_g2_query[i])) for i in (2, 15, 16, 17, 31, 32, 35))
        _edit(case, pk.a_query, pk.b_g2_query if case != "wrong" else pk.b_g1_query, 16)
        rep = cc.check_key(pk, rho=_rho(11, pk.n_vars), max_listed=_listed(case), lib=lib)
    elif check == "contribution":
        if id(lib) not in _pair_cache:
            _pair_cache[id(lib)] = TC._pair(cc, lib)
        base, new = _pair_cache[id(lib)]
        after = TC._clone(cc, new)
        _edit(case, after.l_query, after.h_query, 24)
        rep = cc.check_contribution(base, after, rho=_rho(12, 62 + 64), max_listed=_listed(case), lib=lib)
    elif check == "srs":
        srs, _ = _string(cc, lib)
        _edit(case, srs.tau_g1, srs.tau_g2, 5)
        rep = cc.check_srs(srs, rho=_rho(13, 30 + 3 * 15), max_listed=_listed(case), lib=lib)
    else:
        srs, lag = _string(cc, lib)
        _edit(case, lag.tau_g1, lag.tau_g2, 5)
        rep = cc.check_lagrange(srs, lag, rho=_rho(14, 63 + 3 * 31), max_listed=_listed(case), lib=lib)
    return _plain(rep)


_golden = []


def _expected(check, case):
    if not _golden:
        _golden.append(json.load(open(GOLDEN)))
    return _golden[0][check][case]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("check", CHECKS)
def test_reports_are_the_recorded_ones(lib, monkeypatch, check, case):
    import circom_compat_amd as cc
    for name, value in ENV.items():
        monkeypatch.setenv(name, value)
    got, want = run_case(cc, lib, check, case), _expected(check, case)
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], (check, case, field)


def test_the_cases_reach_the_cap_and_the_cut():
    """the recorded reports themselves: the inputs do what the module's docstring says of them"""
    for check in CHECKS:
        lists = "bad" if check in ("key", "contribution") else "bad_points"
        want = {case: _expected(check, case) for case in CASES}
        assert want["clean"]["ok"] and want["clean"][lists] == []
        assert len(want["seam"][lists]) == 4 and not want["seam"]["relations_checked"]
        assert want["wrong"]["relations_checked"] and want["wrong"]["relations_failed"] and want["wrong"][lists] == []
        full, cut = want["many_full"][lists], want["many"][lists]
        assert len(full) == 10 and cut == full[:MANY_LISTED] and want["many_none"][lists] == []
        assert len({e[0] for e in cut}) == 2 and len({e[0] for e in full}) == 2
        for case in ("many", "many_none"):
            assert {k: v for k, v in want[case].items() if k != lists} == \
                {k: v for k, v in want["many_full"].items() if k != lists}
        if check != "contribution":
            assert sum(want["infinity"]["n_infinity"].values()) - sum(want["clean"]["n_infinity"].values()) == 1


if __name__ == "__main__":
    # records the golden file from the emulator build of the tree this runs in
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    subprocess.run(["make", "-C", os.path.join(root, "circom_compat_amd", "csrc"), "emu", "-j8"], check=True)
    import circom_compat_amd as cc
    from circom_compat_amd import _binding
    emu = _binding.Library(os.path.join(root, "tests", "emu", "libg16_emu.so"))
    os.environ.update(ENV)
    out = {check: {case: run_case(cc, emu, check, case) for case in CASES} for check in CHECKS}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
