"""python -m circom_compat_amd: main(argv, lib) in-process under both libraries, and once as a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _main(argv, lib):
    from circom_compat_amd.__main__ import main
    return main([str(a) for a in argv], lib)


@pytest.fixture
def wtns(golden, tmp_path):
    import circom_compat_amd as cc
    path = str(tmp_path / "my.wtns")
    cc.write_wtns(path, [int(x) for x in json.load(open(os.path.join(golden, "mycircuit-witness.json")))])
    return path


def test_prove_then_verify(lib, golden, wtns, tmp_path, capsys):
    zkey = os.path.join(golden, "test.zkey")
    pj, uj, vj = tmp_path / "proof.json", tmp_path / "public.json", tmp_path / "vk.json"
    assert _main(["prove", zkey, wtns, pj, uj], lib) == 0
    assert json.load(open(uj)) == ["33"] and set(json.load(open(pj))) == {"pi_a", "pi_b", "pi_c", "protocol", "curve"}
    assert _main(["export-vkey", zkey, vj], lib) == 0
    want = json.load(open(os.path.join(golden, "verification_key.json")))
    del want["vk_alphabeta_12"]
    assert json.load(open(vj)) == want
    capsys.readouterr()
    assert _main(["verify", vj, uj, pj], lib) == 0
    assert capsys.readouterr().out.strip() == "OK"
    assert _main(["verify", os.path.join(golden, "verification_key.json"), uj, pj], lib) == 0
    capsys.readouterr()
    # one digit of public.json changed
    open(uj, "w").write('["34"]')
    assert _main(["verify", vj, uj, pj], lib) == 1
    assert capsys.readouterr().out.strip() == "INVALID"
    # calldata: 8 + 1 words
    open(uj, "w").write('["33"]')
    assert _main(["calldata", uj, pj], lib) == 0
    assert capsys.readouterr().out.count("0x") == 9


def test_wtns_check(lib, golden, tmp_path, capsys):
    import circom_compat_amd as cc
    r1cs, good = os.path.join(golden, "circuit2.r1cs"), os.path.join(golden, "circuit2.wtns")
    assert _main(["wtns-check", r1cs, good], lib) == 0
    vals = o.read_wtns(open(good, "rb").read())
    vals[100] = (vals[100] + 1) % o.R_MOD
    bad = str(tmp_path / "bad.wtns")
    cc.write_wtns(bad, vals)
    want = cc.CircomBuilder(cc.R1CS.from_file(r1cs, lib=lib)).build(vals).first_unsatisfied(lib=lib)
    assert want >= 0
    capsys.readouterr()
    assert _main(["wtns-check", r1cs, bad], lib) == 1
    assert f"constraint {want} " in capsys.readouterr().out
    # a witness of another circuit: bad input, not a crash
    short = str(tmp_path / "short.wtns")
    cc.write_wtns(short, vals[:10])
    assert _main(["wtns-check", r1cs, short], lib) == 2


def test_prove_batch_writes_four_files(lib, golden, wtns, tmp_path):
    import circom_compat_amd as cc
    second = str(tmp_path / "other.wtns")
    cc.write_wtns(second, [1, 33, 3, 11])
    out = tmp_path / "out"
    assert _main(["prove-batch", os.path.join(golden, "test.zkey"), out, wtns, second], lib) == 0
    assert sorted(os.listdir(out)) == ["my.proof.json", "my.public.json", "other.proof.json", "other.public.json"]
    vk = cc.read_vk_json(os.path.join(golden, "verification_key.json"), lib=lib)
    proofs = [cc.read_proof_json(str(out / f"{s}.proof.json"), lib=lib) for s in ("my", "other")]
    pubs = [cc.read_public_json(str(out / f"{s}.public.json")) for s in ("my", "other")]
    assert cc.verify_batch(vk, proofs, pubs, lib=lib) == [True, True]


def test_bad_input_is_one_line_and_status_2(lib, golden, wtns, tmp_path, capsys):
    zkey = os.path.join(golden, "test.zkey")
    capsys.readouterr()
    assert _main(["prove", str(tmp_path / "absent.zkey"), wtns, tmp_path / "p.json", tmp_path / "u.json"], lib) == 2
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "absent.zkey" in err and "Traceback" not in err
    # a witness with a value >= r, a file that is no zkey, no JSON, an unknown command
    import circom_compat_amd as cc
    big = str(tmp_path / "big.wtns")
    cc.write_wtns(big, np.full((4, 32), 0xff, dtype=np.uint8))
    assert _main(["prove", zkey, big, tmp_path / "p.json", tmp_path / "u.json"], lib) == 2
    assert "Traceback" not in capsys.readouterr().err and not os.path.exists(tmp_path / "p.json")
    assert _main(["prove", wtns, wtns, tmp_path / "p.json", tmp_path / "u.json"], lib) == 2
    assert _main(["verify", zkey, zkey, zkey], lib) == 2
    assert _main(["frobnicate"], lib) == 2
    assert "Traceback" not in capsys.readouterr().err


@pytest.mark.gpu
def test_child_process_proves(golden, wtns, tmp_path):
    pj, uj = tmp_path / "proof.json", tmp_path / "public.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "circom_compat_amd", "prove", os.path.join(golden, "test.zkey"), wtns,
                        str(pj), str(uj)], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([sys.executable, "-m", "circom_compat_amd", "verify",
                        os.path.join(golden, "verification_key.json"), str(uj), str(pj)],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
