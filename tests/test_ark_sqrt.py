"""The square roots of the ark-serialize codec alone (csrc/arkser.h: fq_sqrt, fq2_sqrt) through the raw hooks of
tests/arith/sqrt_hooks.hip, on the emulator build and on the gfx950 build of the same file, against Python's pow.

Exact arithmetic, no tolerance: every returned root is squared back, and every "no root" verdict is checked against
Euler's criterion (a^((q-1)/2) in Fq, the norm's in Fq2)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import bn254_ref as o

Q = o.Q_MOD
R = o.MONT_R % Q
R_INV = pow(R, Q - 2, Q)
GPU_HOOKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "arith", "libg16_sqrt_gpu.so")


class Hooks:
    def __init__(self, L):
        for name in ("g16_test_fq_sqrt", "g16_test_fq2_sqrt"):
            fn = getattr(L, name)                          # hook lookup: missing without the feature
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self.L = L

    def run(self, name, rows):
        """rows: n tuples of canonical ints (1 per row in Fq, 2 in Fq2) -> (roots as tuples of ints, ok flags)"""
        n, w = len(rows), len(rows[0])
        raw = b"".join((v * R % Q).to_bytes(32, "little") for row in rows for v in row)
        src = np.frombuffer(raw, dtype=np.uint8)
        out = np.zeros(n * w * 32, dtype=np.uint8)
        ok = np.full(n, 7, dtype=np.uint8)
        st = getattr(self.L, name)(src.ctypes.data, n, out.ctypes.data, ok.ctypes.data)
        assert st == 0, st
        b = out.tobytes()
        vals = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
        assert all(v < Q for v in vals)
        vals = [v * R_INV % Q for v in vals]
        return [tuple(vals[i * w:(i + 1) * w]) for i in range(n)], [int(x) for x in ok]


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def hooks(request):
    if request.param == "emu":
        return Hooks(request.getfixturevalue("emu").L)
    if not os.path.exists(GPU_HOOKS):
        pytest.fail(f"{GPU_HOOKS} is not built (make -C circom_compat_amd/csrc)")
    return Hooks(C.CDLL(GPU_HOOKS))


def _is_residue(a):
    return a == 0 or pow(a, (Q - 1) // 2, Q) == 1


def _fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a else None


def test_fq_sqrt(hooks):
    rng = random.Random(5101)
    cs = [0, 1, Q - 1, 4, 9, 2, 3, Q - 4, (Q - 1) // 2, (Q + 1) // 2]
    cs += [rng.randrange(Q) ** 2 % Q for _ in range(40)]                      # residues
    cs += [rng.randrange(Q) for _ in range(80)]
    assert len(cs) % 64 != 0 and len(cs) > 64                                 # more than one block, a ragged tail
    res = [a for a in cs if _is_residue(a)]
    assert len(res) > 40 and len(cs) - len(res) > 20                          # both verdicts occur
    assert not _is_residue(Q - 1)                                             # q = 3 mod 4: -1 is a non-residue
    roots, ok = hooks.run("g16_test_fq_sqrt", [(a,) for a in cs])
    for a, (r,), good in zip(cs, roots, ok):
        assert good in (0, 1)
        assert bool(good) == _is_residue(a), a                               # Euler's criterion
        if good:
            assert r * r % Q == a, a


def _f2_is_square(a):
    """a is a square in Fq2 iff its norm is a residue in Fq"""
    return _is_residue((a[0] * a[0] + a[1] * a[1]) % Q)


def _t_sign_class(a):
    """which sign of t = (a0 +- s) / 2 is the residue, s = sqrt(norm): '+', '-' (for either root s of the norm the
    two candidates are the same pair; the class is taken for the s the kernel computes, norm^((q+1)/4))"""
    s = _fq_sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
    t = (a[0] + s) * pow(2, Q - 2, Q) % Q
    return "+" if _is_residue(t) else "-"


def test_fq2_sqrt(hooks):
    rng = random.Random(5102)
    rnd = lambda: (rng.randrange(Q), rng.randrange(Q))
    res = next(a for a in iter(lambda: rng.randrange(1, Q), None) if _is_residue(a))
    non = Q - res                                                             # -res: a non-residue
    cs = [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1)]
    cs += [(res, 0), (non, 0)]                                                # a1 = 0: a0 a residue; -a0 a residue
    cs += [(0, rng.randrange(1, Q)) for _ in range(6)]                        # a0 = 0
    cs += [o.f2_sqr(rnd()) for _ in range(60)]                                # squares
    cs += [rnd() for _ in range(60)]
    assert len(cs) % 64 != 0 and len(cs) > 128
    squares = [a for a in cs if _f2_is_square(a)]
    assert len(squares) > 70 and len(cs) - len(squares) > 15
    classes = {_t_sign_class(a) for a in squares if a[1]}
    assert classes == {"+", "-"}                                              # both signs of t are reached
    roots, ok = hooks.run("g16_test_fq2_sqrt", cs)
    for a, y, good in zip(cs, roots, ok):
        assert good in (0, 1)
        assert bool(good) == _f2_is_square(a), a
        if good:
            assert o.f2_sqr(y) == a, a
    # the a1 = 0 branch: a real root for a residue a0, a purely imaginary one otherwise
    by = dict(zip(cs, roots))
    assert by[(res, 0)][1] == 0 and by[(res, 0)][0] != 0
    assert by[(non, 0)][0] == 0 and by[(non, 0)][1] != 0
    assert by[(Q - 1, 0)] in ((0, 1), (0, Q - 1))
    assert by[(0, 0)] == (0, 0)


def test_same_answers_twice(hooks):
    rng = random.Random(5103)
    cs = [(rng.randrange(Q), rng.randrange(Q)) for _ in range(70)]
    assert hooks.run("g16_test_fq2_sqrt", cs) == hooks.run("g16_test_fq2_sqrt", cs)
