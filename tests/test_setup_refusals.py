"""The four setup entry points -- g16_setup_create, g16_setup_create_ex (keygen.hip), g16_setup_from_srs and
g16_setup_from_prepared (setup_srs.hip) -- take transposed CSR matrices from their caller, and their kernels walk
row_ptr[i] .. row_ptr[i + 1] and index the Lagrange basis with col[j] unchecked.  A malformed matrix must be refused on
the host with G16_ERR_INVALID and a NULL handle, before anything is allocated, copied or launched.  The Python wrappers
only ever build well-formed transposes, so the calls go through ctypes here.

squaring_chain(3): 6 constraints, 8 wires, domain 8; `at` carries the n_public + 1 = 2 rows snarkjs appends (constraint
indices 6 and 7), bt and ct stop at 6.  One property is broken per case, in each matrix, on copies; afterwards the
untouched matrices still give the oracle's key through every entry point."""
import ctypes as C

import numpy as np
import pytest

import bn254_ref as o
import helpers as H
import test_setup_srs as S

TOX5 = [0x1234567, 0x89ABCDE, 0xF012345, 0x6789ABC, 0xDEF0123]
SRS_SEED, K = 32, 3          # the oracle-made SRS test_setup_srs.py shares
ENTRY_POINTS = ("g16_setup_create", "g16_setup_create_ex", "g16_setup_from_srs", "g16_setup_from_prepared")
MATRICES = ("at", "bt", "ct")

_circuit = H.squaring_chain(K)
_state = {}


def _setup(cc, lib):
    """per library: the well-formed transposes, the SRS, its Lagrange set"""
    if id(lib) not in _state:
        cons, _w, n_vars, n_pub = _circuit
        csrs = S._csrs(cc, cons, lib)
        at, bt, ct = cc._setup_matrices(*csrs, n_vars, n_pub, lib)
        srs = S._cached_py_srs(cc, K, SRS_SEED)
        _state[id(lib)] = dict(at=at, bt=bt, ct=ct, srs=srs, lag=cc.prepare_phase2(srs, power=K, lib=lib),
                               tox=cc.fr_from_ints(TOX5, lib))
    return _state[id(lib)]


def _call(cc, lib, st, name, mats):
    """one entry point over the three B.Csr in mats -> (status, handle)"""
    _cons, _w, n_vars, n_pub = _circuit
    m = len(_cons)
    h = C.c_void_p(1)                                       # a refusal must leave NULL here
    head = (0, C.byref(mats["at"]), C.byref(mats["bt"]), C.byref(mats["ct"]), n_vars, n_pub, m)
    d, dl = st["srs"].to_c(), st["lag"].to_c()
    circom = cc.REDUCTIONS["circom"]
    if name == "g16_setup_create":
        status = lib.g16_setup_create(*head, st["tox"].ctypes.data, C.byref(h))
    elif name == "g16_setup_create_ex":
        status = lib.g16_setup_create_ex(*head, st["tox"].ctypes.data, circom, C.byref(h))
    elif name == "g16_setup_from_srs":
        status = lib.g16_setup_from_srs(*head, C.byref(d), circom, C.byref(h))
    else:
        status = lib.g16_setup_from_prepared(*head, C.byref(d), C.byref(dl), circom, C.byref(h))
    return status, h


# what is broken -> (row_ptr, col, coeff, nnz) of the broken copy; None for an array stands for a NULL pointer.
# `bound`: the first constraint index the matrix may not name.
def _row_ptr_starts_at_1(rp, col, co, bound):
    rp[0] = 1
    return rp, col, co, len(col)


def _row_ptr_steps_back(rp, col, co, bound):
    rp[1] = rp[2] + 1                                       # still starts at 0 and ends at nnz
    return rp, col, co, len(col)


def _row_ptr_ends_below_nnz(rp, col, co, bound):
    rp[-1] -= 1
    return rp, col, co, len(col)


def _row_ptr_ends_above_nnz(rp, col, co, bound):
    return rp, col, co, len(col) - 1                        # the arrays are longer than nnz says: nothing is read past them


def _null_col(rp, col, co, bound):
    return rp, None, co, len(col)


def _null_coeff(rp, col, co, bound):
    return rp, col, None, len(col)


def _null_row_ptr(rp, col, co, bound):
    return None, col, co, len(col)


def _col_at_the_bound(rp, col, co, bound):
    col[len(col) // 2] = bound                              # inside the domain of 8 for bt and ct, and still refused
    return rp, col, co, len(col)


def _col_last_entry_huge(rp, col, co, bound):
    col[-1] = 0xFFFFFFFF
    return rp, col, co, len(col)


def _col_first_entry_past_the_domain(rp, col, co, bound):
    col[0] = 8
    return rp, col, co, len(col)


DEFECTS = (_row_ptr_starts_at_1, _row_ptr_steps_back, _row_ptr_ends_below_nnz, _row_ptr_ends_above_nnz, _null_col,
           _null_coeff, _null_row_ptr, _col_at_the_bound, _col_last_entry_huge, _col_first_entry_past_the_domain)


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda f: f.__name__.lstrip("_"))
@pytest.mark.parametrize("which", MATRICES)
def test_malformed_matrix_is_refused(lib, which, defect):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    st = _setup(cc, lib)
    cons, _w, n_vars, n_pub = _circuit
    good = st[which]
    assert good.row_ptr.shape == (n_vars + 1,) and good.col.shape[0] == (8 if which == "at" else 6)
    bound = len(cons) + (n_pub + 1 if which == "at" else 0)
    assert int(good.col.max()) == bound - 1                 # the bound is tight: the largest legal index is in use
    rp, col, co, nnz = defect(good.row_ptr.copy(), good.col.copy(), good.coeff.copy(), bound)
    broken = B.Csr()
    broken.row_ptr = rp.ctypes.data_as(C.POINTER(C.c_uint32)) if rp is not None else None
    broken.col = col.ctypes.data_as(C.POINTER(C.c_uint32)) if col is not None else None
    broken.coeff = co.ctypes.data_as(C.POINTER(C.c_uint64)) if co is not None else None
    broken.nnz = nnz
    mats = {k: st[k].to_c() for k in MATRICES}
    mats[which] = broken
    for name in ENTRY_POINTS:
        status, h = _call(cc, lib, st, name, mats)
        assert status == B.G16_ERR_INVALID, (name, status)
        assert h.value is None, name


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_untouched_matrices_still_give_the_key(lib, name):
    import circom_compat_amd as cc
    from circom_compat_amd import _binding as B
    st = _setup(cc, lib)
    cons, _w, n_vars, n_pub = _circuit
    status, h = _call(cc, lib, st, name, {k: st[k].to_c() for k in MATRICES})
    assert status == B.G16_OK and h.value not in (None, 1)
    got = cc._setup_key(lib, h, n_vars, n_pub)
    srs_path = name in ("g16_setup_from_srs", "g16_setup_from_prepared")
    key = "srs" if srs_path else "trapdoor"
    if key not in _state:                                   # the oracle's key: once, whichever library asks first
        tox = S._tox3(SRS_SEED) + [1, 1] if srs_path else TOX5
        _state[key] = H.pk_from_oracle(o.trapdoor_setup(cons, n_vars, n_pub, *tox))
    assert got.domain_size == 8
    S._same_key(got, _state[key])
