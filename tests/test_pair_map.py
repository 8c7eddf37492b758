"""The A|B1 pair launch (k_bucket_accumulate<Fq, 2, PAIR = true, ..>, msm_curve.inc.h) with the half-wave mapping:
lanes l and l + 32 of a wave walk the SAME segment over the two halves of every 128-byte record, so both halves of a
record are requested by one load instruction.  Whole proofs with the fixed-base tables off (tables = -1: the bucket
path and with it the pair launch), bytes == the oracle's:

  chain 2^12         fewer entries than lanes: most lanes are dead (the `!w.live` exit and the last live lane, in both
                     half-waves of one wave)
  chain 2^16         segments of a few entries that cross bucket boundaries
  dense_skewed 2^14  hot buckets: k_combine_large reads partials of both halves
  fix list           a key whose A and B1 queries repeat points under equal scalars: both half-waves append items to
                     the fix list (slot | half << 31), some sharing a slot, and k_acc_fixup adds them to the right half

and the same legs once more with G16_PAIR_MAP=0 (one wave per half, the mapping before; the knob is read once per
process, so those run in a child)."""
import os
import random
import subprocess
import sys

import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG_LEGS = ("chain12", "chain16", "dense14")


def _big_leg(cc, name):
    """(pk, mats, r, s, w) of a bench circuit under a key minted on the GPU (pinned to the oracle's trapdoor scalars
    by tests/test_gpu_large.py), as packed arrays"""
    sys.path.insert(0, ROOT)
    import bench
    k = int(name[-2:])
    if name.startswith("dense"):
        mats, (A, B, Cm), w_ints, n_vars = bench.dense_skewed_circuit(cc, k)
    else:
        mats, (A, B, Cm), w_ints, n_vars = bench.chain_circuit(cc, k)
    rng = random.Random(8000 + k)
    tox = [rng.randrange(1, o.R_MOD) for _ in range(5)]
    pk = cc.trapdoor_setup(A, B, Cm, n_vars, 1, tox)
    rs = cc.fr_from_ints([rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)])
    return pk, mats, rs, cc.fr_from_ints(w_ints)


def _fix_leg():
    """64 witness scalars over A and B1 queries with repeated points.  Wires 10..13 carry one scalar, so their four
    entries meet in one bucket of every window, next to each other in a segment: A holds P, P, P, X there (inf + P,
    then P + P twice: two fix-list items of the first half on one slot) and B1 holds Y, Q, Q, Q (two items of the
    second half on the slot of the same number); wires 20, 21 and 30, 31 give either half an item of its own.
    (With window_bits = 16 the emulator build's list holds 61 items after the pair launch, 18 of them with the
    second half's bit, a dozen slots listed twice -- well below MSM_FIX_CAP, so k_acc_fixup adds them all.)"""
    rng = random.Random(831)
    n = 64
    N = n + 1
    g1 = H.rand_g1(rng, 3)
    g2 = H.rand_g2(rng, 3)
    A = [o.G1.mul(g1[0], 2 * i + 3) for i in range(N)]
    B1 = [o.G1.mul(g1[1], 2 * i + 5) for i in range(N)]
    A[11] = A[12] = A[10]
    B1[12] = B1[13] = B1[11]
    A[21] = A[20]
    B1[31] = B1[30]
    B2 = [o.G2.mul(g2[0], i + 2) for i in range(N)]
    pk = dict(n_vars=N, n_public=1, domain_size=4, alpha_g1=g1[0], beta_g1=g1[1], beta_g2=g2[0], gamma_g2=g2[1],
              delta_g1=g1[2], delta_g2=g2[2], ic=g1[:2], a_query=A, b_g1_query=B1, b_g2_query=B2,
              l_query=[g1[i % 3] for i in range(N - 2)], h_query=g1 + g1[:1])
    w = [1] + H.rand_fr(rng, n)
    w[11] = w[12] = w[13] = w[10]
    w[21] = w[20]
    w[31] = w[30]
    r, s = rng.randrange(o.R_MOD), rng.randrange(o.R_MOD)
    rows = dict(a=[[(1, 1)]], b=[[(1, 0)]])
    return pk, rows, r, s, w


def _prove_fix_leg(cc, lib):
    pk, rows, r, s, w = _fix_leg()
    mats = H.matrices_from_rows(rows["a"], rows["b"], 2, pk["n_vars"], lib)
    pr = cc.Prover(H.pk_from_oracle(pk), mats, lib=lib, window_bits=16, tables=-1)
    raw = bytes(pr.prove(r, s, w).raw)
    pr.close()
    return raw


def _prove_big_leg(cc, lib, name, leg=None):
    pk, mats, rs, w = leg or _big_leg(cc, name)
    pr = cc.Prover(pk, mats, lib=lib, tables=-1)
    assert pr.info()["fixed_tables"] == 0
    raw = bytes(pr.prove(rs[0], rs[1], w).raw)
    pr.close()
    return raw


def child_main(lib_path, legs):
    """the old-mapping legs: run in a process of their own (G16_PAIR_MAP is read once), one hex line per leg"""
    import circom_compat_amd as cc
    from circom_compat_amd import _binding
    lib = _binding.Library(lib_path)
    for name in legs:
        raw = _prove_fix_leg(cc, lib) if name == "fix" else _prove_big_leg(cc, lib, name)
        print(name, raw.hex(), flush=True)


def _child(lib, legs, pair_map):
    code = "import test_pair_map as t; t.child_main(%r, %r)" % (lib.path, list(legs))
    env = dict(os.environ, G16_PAIR_MAP=pair_map, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests")] + sys.path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return dict(line.split() for line in out.stdout.strip().splitlines() if line.split()[0] in legs)


@pytest.fixture(scope="module")
def fix_want():
    pk, rows, r, s, w = _fix_leg()
    return o.proof_to_bytes(o.create_proof_with_reduction_and_matrices(pk, r, s, rows, 2, 1, w))


def test_fix_list_items_of_both_halves_vs_oracle(lib, fix_want):
    import circom_compat_amd as cc
    assert _prove_fix_leg(cc, lib) == fix_want


def test_fix_list_items_of_both_halves_old_mapping(lib, fix_want):
    assert _child(lib, ["fix"], "0")["fix"] == fix_want.hex()


@pytest.fixture(scope="module")
def big_want(gpulib):
    """the oracle's bytes of the three big legs (the C restatement, pinned to bn254_ref by tests/test_oracle.py),
    computed once"""
    import circom_compat_amd as cc
    import cpu_ref
    want, legs = {}, {}
    for name in BIG_LEGS:
        leg = legs[name] = _big_leg(cc, name)
        pk, mats, rs, w = leg
        want[name] = bytes(cpu_ref.prove(pk, mats, rs[0:1].copy(), rs[1:2].copy(), w))
    return want, legs


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIG_LEGS)
def test_pair_launch_proofs_vs_oracle(gpulib, big_want, name):
    import circom_compat_amd as cc
    want, legs = big_want
    assert _prove_big_leg(cc, gpulib, name, legs[name]) == want[name]


@pytest.mark.gpu
def test_pair_launch_proofs_old_mapping(gpulib, big_want):
    want, _ = big_want
    got = _child(gpulib, BIG_LEGS, "0")
    assert got == {name: want[name].hex() for name in BIG_LEGS}
