"""The accumulation loop without per-iteration infinity handling (msm_curve.inc.h: AccWay::empty, the run-start
block of acc_way_prepare, the commit predicate of acc_way_commit; ec29.h: XYZZ29::madd_core).  What the selects of
madd_select used to decide on every lane-iteration is now decided by control flow: an empty accumulator takes its
first finite point as (x, y, 1, 1), a point at infinity is never committed, a cancelled accumulator (P + (-P) in the
exact kernel) is empty again.  Whole proofs through the public prover on the bucket path (tables = -1), bytes == the
oracle's (the C restatement, pinned to bn254_ref by tests/test_oracle.py), for keys and witnesses that put every one
of those cases into the kernels:

  inf      about a third of the b_g1 / b_g2 points (and a few a points) at infinity; wires in groups of four with
           one scalar meet in one bucket next to each other, and the first one, the first two or all four b points
           of a group are infinite: runs whose first entries never start them, runs that stay empty
  pub3     three public inputs: the entries below idx_min in L's launch are points at infinity by construction
  skew     a witness of mostly 0, 1 and r - 1: runs of empty buckets, and hot buckets that span many lanes
  edge     every bucket holds a multiple of four entries (groups of four equal scalars, wire 0's 1 included); on the
           default grid a segment is MSM_MIN_SEG = 8 entries at these sizes, so segments end exactly on bucket
           boundaries: the next lane starts with the run, the last entry of a lane ends one
  repeat   repeated and negated points under equal scalars: P + P (the exact doubling in G2, fix-list items in the
           optimistic G1 launches) and P - P followed by further points of the same bucket (the accumulator is
           empty again in the middle of a run).  3 pairs x 2 halves x 64 windows stays below MSM_FIX_CAP even in the
           emulator build (512)

each with window widths 4 (a handful of buckets: long runs) and 16 (mostly one entry per bucket: every iteration
starts a run), on the default grid -- most lanes hold 0..2 entries -- and, in a child process (the grid knobs are
read from the environment), with G16_ACC_GRID = 1 / G16_ACC_GRID_G2 = 2: 128 / 256 lanes that cross many buckets.
Keys have 300 wires on the emulator (it steps through every thread of every launch) and 300 .. 4000 on the GPU."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bn254_ref as o
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("inf", "pub3", "skew", "edge", "repeat")
WIDTHS = (4, 16)
R = o.R_MOD


def _neg_g1(rec):
    """packed affine G1 record (Montgomery x | y) -> its negative"""
    p = o.g1_from_bytes(bytes(rec))
    return np.frombuffer(o.g1_to_bytes(o.G1.neg(p)), dtype=np.uint8)


def _neg_g2(rec):
    p = o.g2_from_bytes(bytes(rec))
    return np.frombuffer(o.g2_to_bytes(o.G2.neg(p)), dtype=np.uint8)


# wires per key: the emulator steps through every thread of every launch (about 7 s per 300-wire proof), the GPU does not
SIZES = {False: {"inf": 300, "pub3": 300, "skew": 300, "edge": 300, "repeat": 320},
         True: {"inf": 1500, "pub3": 300, "skew": 4000, "edge": 1200, "repeat": 320}}


def _is_gpu(lib):
    return "emu" not in os.path.basename(lib.path)


def _leg(name, big):
    """-> (pk, rows, num_inputs, r, s, witness ints): a key of distinct multiples of the generators, then the leg's
    infinities / repeats written into the packed arrays"""
    import circom_compat_amd as cc
    import cpu_ref
    rng = random.Random(9000 + LEGS.index(name))
    n_pub = 3 if name == "pub3" else 1
    n = SIZES[big][name]
    dom = 4 if n_pub == 1 else 8
    g1, g2 = o.g1_to_bytes(o.G1_GEN), o.g2_to_bytes(o.G2_GEN)
    ks = lambda k: [rng.randrange(1, R) for _ in range(k)]
    A, B1, B2 = cpu_ref.g1_mul_batch(g1, ks(n)), cpu_ref.g1_mul_batch(g1, ks(n)), cpu_ref.g2_mul_batch(g2, ks(n))
    L, Hq = cpu_ref.g1_mul_batch(g1, ks(n - n_pub - 1)), cpu_ref.g1_mul_batch(g1, ks(dom))
    fixed1, fixed2 = cpu_ref.g1_mul_batch(g1, ks(3 + n_pub + 1)), cpu_ref.g2_mul_batch(g2, ks(3))
    w = [1] + H.rand_fr(rng, n - 1)

    def group4(first, count):                      # wires first .. first + 4 count - 1: four neighbours per scalar
        for g in range(count):
            for j in range(1, 4):
                w[first + 4 * g + j] = w[first + 4 * g]

    if name == "inf":
        groups = 100 if big else 40
        group4(8, groups)
        for g in range(groups):
            dead = (1, 2, 4, 0)[g % 4]
            B1[8 + 4 * g:8 + 4 * g + dead] = 0
            B2[8 + 4 * g:8 + 4 * g + dead] = 0
        for i in range(8 + 4 * groups, n):
            if rng.random() < 0.4:
                B1[i] = 0
                B2[i] = 0
            if rng.random() < 0.05:
                A[i] = 0
        B1[0] = 0
        B2[0] = 0
        B1[n - 3:] = 0                             # the tail of the last segment
        B2[n - 3:] = 0
    elif name == "pub3":
        w[1], w[2], w[3] = 5, R - 1, 0
        for i in range(20, n, 7):
            B1[i] = 0
            B2[i] = 0
    elif name == "skew":
        for i in range(1, n):
            x = rng.random()
            if x < 0.35:
                w[i] = 0
            elif x < 0.7:
                w[i] = 1
            elif x < 0.85:
                w[i] = R - 1
            elif x < 0.9:
                w[i] = rng.randrange(1, 1 << 16)   # one window only: the others' buckets stay empty
    elif name == "edge":
        w[1] = w[2] = w[3] = 1
        group4(4, (n - 4) // 4)
    elif name == "repeat":
        group4(40, 3)
        for first in (40, 44):                     # P, P, X, Y: a doubling, then the run goes on
            A[first + 1] = A[first]
            B1[first + 1] = B1[first]
            B2[first + 1] = B2[first]
        A[49], B1[49], B2[49] = _neg_g1(A[48]), _neg_g1(B1[48]), _neg_g2(B2[48])   # P, -P, X, Y
        L[60] = L[59]                              # l_query[i] belongs to wire i + n_pub + 1: wires 61 and 62 ...
        w[62] = w[61]                              # ... with one scalar
        Hq[2] = Hq[1]                              # (H's scalars are the witness map's: no equal pair, a plain key row)
    vk = cc.VerifyingKey(fixed1[0].tobytes(), fixed2[0].tobytes(), fixed2[1].tobytes(), fixed2[2].tobytes(),
                         fixed1[3:].copy())
    pk = cc.ProvingKey(n, n_pub, dom, vk, fixed1[1].tobytes(), fixed1[2].tobytes(), A, B1, B2, L, Hq)
    rows = dict(a=[[(1, 1)]], b=[[(1, 0)]])
    return pk, rows, n_pub + 1, rng.randrange(R), rng.randrange(R), w


_LEGS = {}


def _cached_leg(name, big):
    if (name, big) not in _LEGS:
        _LEGS[name, big] = _leg(name, big)
    return _LEGS[name, big]


def _prove(cc, lib, name, wb):
    pk, rows, num_inputs, r, s, w = _cached_leg(name, _is_gpu(lib))
    mats = H.matrices_from_rows(rows["a"], rows["b"], num_inputs, pk.n_vars, lib)
    pr = cc.Prover(pk, mats, lib=lib, window_bits=wb, tables=-1)
    rs = H.fr_mont_arr([r, s])
    raw = bytes(pr.prove(rs[0], rs[1], H.fr_mont_arr(w)).raw)
    pr.close()
    return raw


_WANT = {}


def _want(name, lib):
    """the oracle's proof bytes, once per leg and size"""
    big = _is_gpu(lib)
    if (name, big) not in _WANT:
        import cpu_ref
        pk, rows, num_inputs, r, s, w = _cached_leg(name, big)
        mats = H.matrices_from_rows(rows["a"], rows["b"], num_inputs, pk.n_vars, lib)
        rs = H.fr_mont_arr([r, s])
        _WANT[name, big] = bytes(cpu_ref.prove(pk, mats, rs[0:1].copy(), rs[1:2].copy(), H.fr_mont_arr(w)))
    return _WANT[name, big]


@pytest.mark.parametrize("wb", WIDTHS)
@pytest.mark.parametrize("name", LEGS)
def test_default_grid_proofs_vs_oracle(lib, name, wb):
    import circom_compat_amd as cc
    assert _prove(cc, lib, name, wb) == _want(name, lib)


def child_main(lib_path, name):
    """one leg at both widths in a process whose environment holds the small grids; one hex line per proof"""
    import circom_compat_amd as cc
    from circom_compat_amd import _binding
    lib = _binding.Library(lib_path)
    for wb in WIDTHS:
        print("proof", wb, _prove(cc, lib, name, wb).hex(), flush=True)


@pytest.mark.parametrize("name", LEGS)
def test_one_and_two_workgroup_grids_vs_oracle(lib, name):
    code = "import test_acc_diet as t; t.child_main(%r, %r)" % (lib.path, name)
    env = dict(os.environ, G16_ACC_GRID="1", G16_ACC_GRID_G2="2",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests")] + sys.path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {int(f[1]): f[2] for f in (line.split() for line in out.stdout.splitlines()) if len(f) == 3 and f[0] == "proof"}
    assert got == {wb: _want(name, lib).hex() for wb in WIDTHS}
