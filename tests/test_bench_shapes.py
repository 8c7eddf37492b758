"""The driver's N > 1 launch shapes of bench.py, functionally, on ONE GPU (the ranks time-share device 0,
gloo instead of RCCL between the processes): the in-library ctx under torch.distributed.run, the
fallback to one ctx per process when the in-library ctx cannot be built, and the per-process path asked
for directly.  Round 3 shipped with the per-process path dead (two helpers deleted by mistake: NameError)
because nothing in the suites ran it; these do.  Every line must carry a pairing-verified proof that is
byte-identical to the CPU restatement's at the probe size (the `--full` legs).  The plain N = 1 line carries the
headline alone and `--dump-outputs` writes the timed proof."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, port, extra_env, log2=14):
    env = dict(os.environ)
    env.update({"G16_BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "TMPDIR": "/tmp"})
    env.update(extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", str(n), "--log2", str(log2), "--steps", "2", "--warmup", "1", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line), r.stderr


@pytest.mark.parametrize("name,n,env", [("inlib", 2, {}), ("fallback", 2, {"G16_BENCH_FAIL_INLIB": "1"}),
                                        ("ranks", 4, {"G16_BENCH_MODE": "ranks"})])
def test_bench_n_gt_1_shapes_on_one_gpu(gpulib, name, n, env):
    d, err = _run(n, 29531 + n + len(name), env)
    assert d["n_gpus"] == n and d["scaling"] == "strong" and d["value"] > 0
    assert d["parity"]["proof_verifies"] and d["parity"]["wrong_public_input_rejected"]
    assert all(v for k, v in d["parity"].items() if k.startswith("bit_identical_to_cpu")), d["parity"]
    par = d["config"]["parallelism"]
    if name == "inlib":
        # the default under torch.distributed.run (round 5): BOTH launch shapes are timed on the same inputs,
        # their proofs are identical, `value` is the faster; rccl_ranks = 0 here (gloo stands in for RCCL)
        assert "g16_ctx_create_multi" in par and "one process per GPU" in par and not d.get("fallback_reason")
        assert d["value_inlib"] > 0 and d["value_rccl"] > 0 and d["inlib_and_rccl_proofs_identical"]
        assert d["value"] == pytest.approx(max(d["value_inlib"], d["value_rccl"]), rel=1e-6)
        assert d["rccl_ranks"] == 0 and d["value_is"] in ("in-library", "rccl")
    elif name == "fallback":
        assert d.get("fallback_reason") and "one process per GPU" in par and "fallback" in par, (par, d.get("fallback_reason"))
    else:
        assert "one process per GPU" in par and "g16_ctx_create_multi" not in par, par
        assert d["rccl_ranks"] == 0                     # gloo between the processes on this box
    if name == "fallback":
        assert d["value_rccl"] > 0 and d["value_inlib"] is None


def test_bench_plain_line_and_dump_outputs(gpulib, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` times exactly K proofs and prints the headline only; the
    dumped proof (bytes as float64) is the same in two runs on the same arguments and passes the pairing check."""
    import bn254_ref as o
    import helpers as H
    lines, proofs = [], []
    for i in range(2):
        out = tmp_path / f"run{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log2", "12", "--steps", "3",
               "--warmup", "1", "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        parts = [np.load(out / f"proof_{g}.npy") for g in "abc"]
        assert [p.shape for p in parts] == [(2, 32), (4, 32), (2, 32)]
        assert all(p.dtype == np.float64 for p in parts)
        proofs.append(np.concatenate([p.ravel() for p in parts]))
    d = lines[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] == pytest.approx(d["config"]["num_constraints"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("roofline", "alu", "cpu_baseline", "parity", "secondary", "clock", "value_pcie_inclusive", "value_pipelined"):
        assert key not in d, key
    assert np.array_equal(proofs[0], proofs[1])
    raw = bytes(proofs[0].astype(np.uint8))
    assert np.array_equal(proofs[0], np.frombuffer(raw, np.uint8).astype(np.float64))
    # the same key bench.py mints (chain circuit at 2^12, its seeded trapdoor): the oracle checks the proof
    import circom_compat_amd as cc
    import bench
    k = 12
    _mats, (A, B, Cm), w_ints, n_vars = bench.chain_circuit(cc, k)
    rng = random.Random(k)
    tox = [rng.randrange(1, bench.R_MOD) for _ in range(5)]
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, tox, device=0)
    vk = dict(alpha_g1=o.g1_from_bytes(bytes(pk.vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(pk.vk.beta_g2)),
              gamma_g2=o.g2_from_bytes(bytes(pk.vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(pk.vk.delta_g2)),
              ic=[o.g1_from_bytes(bytes(x)) for x in pk.vk.gamma_abc_g1])
    assert o.verify_proof(vk, [w_ints[1]], H.proof_from_bytes(raw))
