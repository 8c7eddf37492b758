"""The eight g16_..._times(float* ms, uint32_t cap) exports share one reader body (hostcall.h, PhaseTimes::read), and
the eight public *_times() functions one wrapper.  On the emulator library and on the product library: NULL is
G16_ERR_INVALID, a buffer longer than the phases gets zeros in its tail, a shorter one is never written at or beyond
cap, and every *_PHASES tuple is what it has always been."""
import ctypes as C

import pytest

import circom_compat_amd as cc
from circom_compat_amd import _binding as B

# export, the Python tuple of its phase names, the tuple's value written out, the public wrapper
EXPORTS = [
    ("g16_fr_convert_times", "FR_CONVERT_PHASES", ("upload", "convert", "download"), "fr_from_canonical_times"),
    ("g16_srs_prepare_times", "SETUP_SRS_PHASES",
     ("upload", "ntt_g1", "ntt_g2", "ntt_h", "affine", "combine", "download"), "prepare_phase2_times"),
    ("g16_srs_contribute_times", "SRS_CONTRIBUTE_PHASES",
     ("upload", "scalars", "mul_g1", "mul_g2", "affine", "download"), "contribute_srs_times"),
    ("g16_setup_from_srs_times", "SETUP_SRS_PHASES",
     ("upload", "ntt_g1", "ntt_g2", "ntt_h", "affine", "combine", "download"), "setup_from_srs_times"),
    ("g16_proofs_rerandomize_times", "RERANDOMIZE_PHASES",
     ("upload", "prepare", "mul_g1", "mul_g2", "affine", "download"), "rerandomize_times"),
    ("g16_gt_times", "GT_PHASES", ("upload", "g2_tests", "kernels", "download"), "gt_times"),
    ("g16_verify_prepared_times", "VERIFY_PREPARED_PHASES",
     ("upload", "inputs", "g2_tests", "pairing", "download", "prepare"), "verify_prepared_times"),
    ("g16_kzg_times", "KZG_PHASES", ("input", "divide_or_scalars", "msm", "output_or_pairing"), "kzg_times"),
]
GUARD = -12345.5


@pytest.mark.parametrize("export,tuple_name,phases,wrapper", EXPORTS, ids=[e[0] for e in EXPORTS])
def test_times_reader(lib, export, tuple_name, phases, wrapper):
    assert getattr(cc, tuple_name) == phases
    fn = getattr(lib, export)
    n = len(phases)
    assert fn(None, n) == B.G16_ERR_INVALID

    long = (C.c_float * (n + 3))(*([GUARD] * (n + 3)))
    assert fn(long, n + 3) == B.G16_OK
    assert list(long[n:]) == [0.0, 0.0, 0.0]
    assert all(t >= 0.0 for t in long[:n])

    short = (C.c_float * n)(*([GUARD] * n))           # cap = n - 1: the last float is the guard behind the buffer
    assert fn(short, n - 1) == B.G16_OK
    assert short[n - 1] == GUARD
    assert list(short[:n - 1]) == list(long[:n - 1])

    times = getattr(cc, wrapper)(lib)
    assert tuple(times) == phases
    assert list(times.values()) == list(long[:n])
