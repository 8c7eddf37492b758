"""The large-bucket-set schedule of a single-device proof (api.hip, enqueue_witness_msms): the throughput-bound
head of each bucket reduction stays on the main stream, the latency-bound tail (k_set_sum x 2 + k_horner) of the
A | B1, L and B2 reductions runs on the `red` stream.

A small chain circuit reaches that branch with window_bits = 19 (2^18 buckets, a two-slot G1 workspace).  Several
proofs in a row on one ctx cover the two orderings that events carry: slot 0's `contrib` (the L head must wait for
the A | B1 tail) and the drain of one proof's tails before the next proof's heads.  Every proof is compared byte
for byte with the CPU restatement and pairing-verified."""
import os
import random
import subprocess
import sys
import threading

import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_BITS = 19


def _vk_dict(pk):
    return dict(alpha_g1=o.g1_from_bytes(bytes(pk.vk.alpha_g1)), beta_g2=o.g2_from_bytes(bytes(pk.vk.beta_g2)),
                gamma_g2=o.g2_from_bytes(bytes(pk.vk.gamma_g2)), delta_g2=o.g2_from_bytes(bytes(pk.vk.delta_g2)),
                ic=[o.g1_from_bytes(bytes(x)) for x in pk.vk.gamma_abc_g1])


_cache = {}


def _case(lib, logm):
    """circuit, key, witness, three (r, s) and the CPU restatement's three proofs -- computed once per library"""
    key = (lib.path, logm)
    if key in _cache:
        return _cache[key]
    import circom_compat_amd as cc
    import cpu_ref
    sys.path.insert(0, ROOT)
    import bench
    rng = random.Random(1900 + logm)
    mats, (A, B, Cm), w_ints, n_vars = bench.chain_circuit(cc, logm)
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, [rng.randrange(1, o.R_MOD) for _ in range(5)], lib=lib)
    w = cc.fr_from_ints(w_ints, lib=lib)
    rs = [cc.fr_from_ints([rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)], lib=lib) for _ in range(3)]
    want = [cpu_ref.prove(pk, mats, x[0:1].copy(), x[1:2].copy(), w) for x in rs]
    assert len(set(want)) == 3
    _cache[key] = dict(cc=cc, mats=mats, pk=pk, w=w, w_ints=w_ints, rs=rs, want=want, vk=_vk_dict(pk))
    return _cache[key]


def _logm(lib):
    return 10 if lib.path.endswith("libg16_emu.so") else 12


def _prover(c, lib, **kw):
    pr = c["cc"].Prover(c["pk"], c["mats"], lib=lib, window_bits=WINDOW_BITS, **kw)
    info = pr.info()
    assert info["c_w"] == WINDOW_BITS and info["fixed_tables"] == 0   # 2^18 buckets: the large-bucket-set branch
    return pr


def _three_in_a_row(lib):
    c = _case(lib, _logm(lib))
    pr = _prover(c, lib)
    got = [pr.prove(x[0], x[1], c["w"]).raw for x in c["rs"]]
    assert got == c["want"]
    for raw in got:
        assert o.verify_proof(c["vk"], [c["w_ints"][1]], H.proof_from_bytes(raw))
    assert not o.verify_proof(c["vk"], [(c["w_ints"][1] + 1) % o.R_MOD], H.proof_from_bytes(got[0]))
    pr.close()


@pytest.mark.gpu
def test_three_proofs_in_a_row_on_one_ctx(gpulib):
    _three_in_a_row(gpulib)


@pytest.mark.slow
def test_three_proofs_in_a_row_on_one_ctx_emulator(emu):
    """the same path stepped through on the CPU with the limb / value asserts on (2^10 constraints; 2^18 buckets
    per MSM take the emulator two minutes in all)"""
    _three_in_a_row(emu)


@pytest.mark.gpu
def test_sibling_ctx_two_proofs_in_flight(gpulib):
    """two ctxs over the same planes, one host thread each (the two-in-flight leg of the benchmark)"""
    c = _case(gpulib, 12)
    donor = _prover(c, gpulib)
    sib = _prover(c, gpulib, sibling_of=donor)
    got = [[], []]

    def run(i, p):
        for x in c["rs"]:
            got[i].append(p.prove(x[0], x[1], c["w"]).raw)
    ths = [threading.Thread(target=run, args=(i, p)) for i, p in enumerate((donor, sib))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert got[0] == c["want"] and got[1] == c["want"]
    assert o.verify_proof(c["vk"], [c["w_ints"][1]], H.proof_from_bytes(got[1][-1]))
    sib.close()
    donor.close()


_CHILD = r"""
import os, random, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, "oracle"), os.path.join({root!r}, "tests")]
import circom_compat_amd as cc
cc.DEFAULT_TABLES = -1
import test_reduce_tail_split as T
lib = cc._binding.load()
c = T._case(lib, 12)
pr = T._prover(c, lib)
got = [pr.prove(x[0], x[1], c["w"]).raw for x in c["rs"]]
assert got == c["want"], "proofs differ from the CPU restatement on one stream"
assert T.o.verify_proof(c["vk"], [c["w_ints"][1]], T.H.proof_from_bytes(got[-1]))
print("one-stream ok")
"""


@pytest.mark.gpu
def test_one_stream_mode_in_a_fresh_process(gpulib):
    """G16_NO_OVERLAP=1 is read when a ctx is created and the tail placement once per process: a child process"""
    env = dict(os.environ, G16_NO_OVERLAP="1")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "one-stream ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
