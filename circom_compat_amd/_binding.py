"""ctypes binding of the C ABI in include/g16_amd.h + include/g16_loaders.h.

This is the same stub a Rust maintainer would write as `extern "C"`; Python is
only the harness language of tests/ and bench.py.  There is no CPU fallback: `load()` raises when
the HIP library has not been built, and ctx creation fails with G16_ERR_NO_DEVICE without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libg16_amd.so")

G16_OK, G16_ERR_INVALID, G16_ERR_DOMAIN_TOO_LARGE, G16_ERR_HIP, G16_ERR_NO_DEVICE, G16_ERR_IO, \
    G16_ERR_INTERNAL = range(7)
G16_PROOF_BYTES = 256
G16_PARTIAL_BYTES = 1024
G16_N_STAGES = 10
QUERY_A, QUERY_B1, QUERY_L, QUERY_H = 0, 1, 2, 3

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)


class G16Error(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"g16 status {status}: {message}")
        self.status = status
        self.message = message


class SynthesisError(G16Error):
    """PolynomialDegreeTooLarge (reference src/circom/qap.rs:31,66)."""


class SerializationError(G16Error):
    """ark_serialize::SerializationError stand-in for loader failures."""


class Csr(C.Structure):
    _fields_ = [("row_ptr", _u32p), ("col", _u32p), ("coeff", _u64p), ("nnz", C.c_uint64)]


class KeyDesc(C.Structure):
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain_size", C.c_uint32),
                ("a_query", C.c_void_p), ("b_g1_query", C.c_void_p), ("b_g2_query", C.c_void_p),
                ("l_query", C.c_void_p), ("h_query", C.c_void_p),
                ("alpha_g1", C.c_uint8 * 64), ("beta_g1", C.c_uint8 * 64),
                ("delta_g1", C.c_uint8 * 64), ("beta_g2", C.c_uint8 * 128),
                ("delta_g2", C.c_uint8 * 128)]


class Options(C.Structure):
    _fields_ = [("device", C.c_int), ("rank", C.c_int), ("world", C.c_int),
                ("window_bits", C.c_int), ("planes", C.c_int), ("dist_wm", C.c_int),
                ("reduction", C.c_int), ("shard", C.c_int), ("fixed_tables", C.c_int)]


SHARD_AUTO, SHARD_POINTS, SHARD_BUCKETS = 0, 1, 2


class VkDesc(C.Structure):
    _fields_ = [("alpha_g1", C.c_uint8 * 64), ("beta_g2", C.c_uint8 * 128), ("gamma_g2", C.c_uint8 * 128),
                ("delta_g2", C.c_uint8 * 128), ("ic", C.c_void_p), ("ic_count", C.c_uint32)]


# g16_key_check: query ids, per-point reason bits, relation bits (include/g16_amd.h)
KEY_QUERIES = ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query", "ic", "singles")
KEY_Q_A, KEY_Q_B1, KEY_Q_B2, KEY_Q_L, KEY_Q_H, KEY_Q_IC, KEY_Q_SINGLES = range(7)
KEY_SINGLES = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2")
KEY_BAD_NONCANONICAL, KEY_BAD_OFF_CURVE, KEY_BAD_SUBGROUP = 1, 2, 4
KEY_PAIR_BETA, KEY_PAIR_DELTA, KEY_PAIR_B, KEY_VK_MISMATCH = 1, 2, 4, 8


# arkworks serialization (include/g16_amd.h): the extra reason bit, the groups, the flags
KEY_BAD_ENCODING = 8
POINT_G1, POINT_G2 = 0, 1
ARK_COMPRESSED, ARK_VALIDATE = 1, 2


class ArkLayout(C.Structure):
    _fields_ = [("offset", C.c_uint64 * 12), ("count", C.c_uint64 * 12), ("total", C.c_uint64)]


class KeyBadPoint(C.Structure):
    _fields_ = [("query", C.c_uint32), ("index", C.c_uint32), ("reason", C.c_uint32)]


class KeyReportC(C.Structure):
    _fields_ = [("ok", C.c_uint8), ("relations_checked", C.c_uint8), ("relations_failed", C.c_uint32),
                ("n_points", C.c_uint64 * 7), ("n_bad", C.c_uint64 * 7), ("n_infinity", C.c_uint64 * 7),
                ("n_listed", C.c_uint32)]


# g16_key_contribution_check: report.relations_failed bits
CONTRIB_UNCHANGED_MISMATCH, CONTRIB_PAIR_DELTA, CONTRIB_PAIR_L, CONTRIB_PAIR_H, CONTRIB_DELTA_INFINITE = 1, 2, 4, 8, 16


class ContributionReportC(C.Structure):
    _fields_ = [("ok", C.c_uint8), ("relations_checked", C.c_uint8), ("relations_failed", C.c_uint32),
                ("n_bad_l", C.c_uint64), ("n_bad_h", C.c_uint64), ("n_listed", C.c_uint32)]


class SrsDesc(C.Structure):
    _fields_ = [("n_tau_g1", C.c_uint32), ("n_tau", C.c_uint32), ("tau_g1", C.c_void_p), ("tau_g2", C.c_void_p),
                ("alpha_tau_g1", C.c_void_p), ("beta_tau_g1", C.c_void_p), ("beta_g2", C.c_uint8 * 128)]


# g16_srs_check: query ids and relation bits (include/g16_amd.h); the reason bits are KEY_BAD_*
SRS_QUERIES = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "singles")
SRS_Q_TAU_G1, SRS_Q_TAU_G2, SRS_Q_ALPHA_TAU_G1, SRS_Q_BETA_TAU_G1, SRS_Q_SINGLES = range(5)
SRS_SINGLES = ("beta_g2",)
SRS_BASE, SRS_DEGENERATE, SRS_PAIR_TAU, SRS_PAIR_TAU_G1, SRS_PAIR_TAU_G2, SRS_PAIR_ALPHA, SRS_PAIR_BETA, \
    SRS_PAIR_BETA_G2 = 1, 2, 4, 8, 16, 32, 64, 128


class SrsReportC(C.Structure):
    _fields_ = [("ok", C.c_uint8), ("relations_checked", C.c_uint8), ("relations_failed", C.c_uint32),
                ("n_points", C.c_uint64 * 5), ("n_bad", C.c_uint64 * 5), ("n_infinity", C.c_uint64 * 5),
                ("n_listed", C.c_uint32)]


class SrsLagrangeDesc(C.Structure):
    _fields_ = [("power", C.c_uint32), ("tau_g1", C.c_void_p), ("tau_g2", C.c_void_p),
                ("alpha_tau_g1", C.c_void_p), ("beta_tau_g1", C.c_void_p)]


# g16_srs_lagrange_check: the arrays are SRS_QUERIES[:4]; relations_failed has bit (1 << array)
LAGRANGE_ARRAYS = SRS_QUERIES[:4]


class SrsLagrangeReportC(C.Structure):
    _fields_ = [("ok", C.c_uint8), ("relations_checked", C.c_uint8), ("relations_failed", C.c_uint32),
                ("n_points", C.c_uint64 * 4), ("n_bad", C.c_uint64 * 4), ("n_infinity", C.c_uint64 * 4),
                ("n_listed", C.c_uint32)]


class MsmOptions(C.Structure):
    _fields_ = [("window_bits", C.c_int), ("planes", C.c_int), ("max_batch", C.c_int), ("validate", C.c_int)]


class PtauHeader(C.Structure):
    _fields_ = [("n8q", C.c_uint32), ("q", C.c_uint8 * 32), ("power", C.c_uint32), ("ceremony_power", C.c_uint32)]


class ZkeyHeader(C.Structure):
    _fields_ = [("n8q", C.c_uint32), ("n8r", C.c_uint32), ("q", C.c_uint8 * 32),
                ("r", C.c_uint8 * 32), ("n_vars", C.c_uint32), ("n_public", C.c_uint32),
                ("domain_size", C.c_uint32), ("power", C.c_uint32),
                ("alpha_g1", C.c_uint8 * 64), ("beta_g1", C.c_uint8 * 64),
                ("beta_g2", C.c_uint8 * 128), ("gamma_g2", C.c_uint8 * 128),
                ("delta_g1", C.c_uint8 * 64), ("delta_g2", C.c_uint8 * 128)]


class Matrices(C.Structure):
    _fields_ = [("num_instance_variables", C.c_uint32), ("num_witness_variables", C.c_uint32),
                ("num_constraints", C.c_uint32), ("a_num_non_zero", C.c_uint64),
                ("b_num_non_zero", C.c_uint64), ("a", Csr), ("b", Csr)]


class R1csHeader(C.Structure):
    _fields_ = [("version", C.c_uint32), ("field_size", C.c_uint32), ("prime", C.c_uint8 * 32),
                ("n_wires", C.c_uint32), ("n_pub_out", C.c_uint32), ("n_pub_in", C.c_uint32),
                ("n_prv_in", C.c_uint32), ("n_labels", C.c_uint64), ("n_constraints", C.c_uint32),
                ("num_inputs", C.c_uint32), ("num_aux", C.c_uint32), ("num_variables", C.c_uint32)]


# every symbol include/*.h declares; tests assert the built library exports all of them
ABI_SYMBOLS = [
    "g16_ctx_create", "g16_ctx_create_sibling", "g16_ctx_destroy", "g16_last_error", "g16_witness_map", "g16_msm_g1",
    "g16_msm_g2", "g16_prove", "g16_prove_dev", "g16_prove_partial", "g16_prove_partial_dev",
    "g16_prove_finish", "g16_dist_exchange_bytes", "g16_prove_dist_phase1", "g16_prove_dist_phase2",
    "g16_prove_dist_phase3", "g16_set_profiling", "g16_stage_times", "g16_stage_name", "g16_ctx_info", "g16_multi_links",
    "g16_witness_buffer", "g16_witness_upload", "g16_witness_host_buffer", "g16_ctx_create_multi", "g16_dist_set_exchange_stream",
    "g16_partial_buffer", "g16_gather_buffer", "g16_prove_finish_dev", "g16_witness_map_dev", "g16_msm_g1_dev",
    "g16_msm_g2_dev", "g16_verify_batch", "g16_verify_aggregate", "g16_fft_in_place", "g16_dist_attach_rccl", "g16_dist_rccl_ranks", "g16_prove_dist", "g16_check_satisfied", "g16_zkey_write",
    "g16_setup_create", "g16_setup_create_ex", "g16_setup_destroy", "g16_setup_key",
    "g16_loader_last_error", "g16_zkey_open", "g16_zkey_open_mem", "g16_zkey_close",
    "g16_zkey_header_get", "g16_zkey_key", "g16_zkey_ic", "g16_zkey_matrices", "g16_r1cs_open",
    "g16_r1cs_open_mem", "g16_r1cs_close", "g16_r1cs_header_get", "g16_r1cs_matrices",
    "g16_r1cs_wire_mapping", "g16_wtns_read", "g16_wtns_read_mem", "g16_free",
    "g16_fr_from_canonical", "g16_fr_to_canonical",
    "g16_prove_batch", "g16_prove_batch_dev", "g16_witness_map_batch",
    "g16_key_check", "g16_key_contribute", "g16_key_contribution_check",
    "g16_srs_create", "g16_srs_desc_of", "g16_srs_destroy", "g16_setup_from_srs", "g16_setup_from_srs_times",
    "g16_srs_check", "g16_ptau_open", "g16_ptau_open_mem", "g16_ptau_close", "g16_ptau_header_get", "g16_ptau_srs",
    "g16_ptau_write", "g16_srs_contribute", "g16_srs_contribute_times",
    "g16_srs_prepare", "g16_srs_prepare_times", "g16_srs_lagrange_check", "g16_setup_from_prepared",
    "g16_ptau_lagrange", "g16_ptau_write_prepared",
    "g16_points_from_ark", "g16_points_to_ark", "g16_ark_proofs_read", "g16_ark_proofs_write", "g16_ark_pk_size",
    "g16_ark_pk_read", "g16_ark_pk_key", "g16_ark_pk_close", "g16_ark_pk_write", "g16_ark_vk_size", "g16_ark_vk_read",
    "g16_ark_vk_write", "g16_ark_pk_layout", "g16_ark_vk_layout",
    "g16_verify_aggregate_keys", "g16_verify_batch_keys",
    "g16_proofs_rerandomize", "g16_proofs_rerandomize_keys", "g16_proofs_rerandomize_times",
    "g16_pvk_create", "g16_pvk_destroy", "g16_pvk_alpha_beta", "g16_verify_prepared", "g16_pairing_check",
    "g16_verify_prepared_times",
    "g16_pvk_prepare_inputs", "g16_verify_prepared_inputs",
    "g16_pairing_products", "g16_gt_multiexp", "g16_gt_to_ark", "g16_gt_from_ark", "g16_pvk_alpha_g1_beta_g2",
    "g16_gt_times",
    "g16_fr_convert", "g16_fr_convert_times", "g16_witness_upload_canonical", "g16_prove_canonical", "g16_prove_batch_canonical",
    "g16_wtns_open", "g16_wtns_open_mem", "g16_wtns_count", "g16_wtns_values", "g16_wtns_close",
    "g16_msm_bases_create", "g16_msm_bases_destroy", "g16_msm_bases_info", "g16_msm", "g16_msm_once",
    "g16_poly_divide_linear",
    "g16_kzg_key_create", "g16_kzg_key_destroy", "g16_kzg_key_info", "g16_kzg_commit", "g16_kzg_open", "g16_kzg_verify",
    "g16_kzg_times",
]


class Library:
    """Loaded libg16_amd.so with typed entry points."""

    def __init__(self, path: Optional[str] = None):
        path = path or os.environ.get("G16_AMD_LIB") or DEFAULT_LIB
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C circom_compat_amd/csrc). "
                "There is no CPU fallback.")
        self.path = path
        # PyTorch-ROCm wheels carry their own HIP runtime.  If libg16_amd.so (linked against
        # /opt/rocm's libamdhip64) is loaded first, a later `import torch` ends up with a second
        # runtime and reports "No HIP GPUs are available".  Host frameworks that use torch for
        # device buffers / RCCL therefore get its runtime loaded first; G16_NO_TORCH_PRELOAD=1 skips it.
        if not os.environ.get("G16_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = self.L = C.CDLL(path)
        vp = C.c_void_p
        sig = {
            "g16_ctx_create": (C.c_int, [C.POINTER(KeyDesc), C.POINTER(Csr), C.POINTER(Csr),
                                         C.c_uint32, C.POINTER(Options), C.POINTER(vp)]),
            "g16_ctx_create_sibling": (C.c_int, [vp, C.POINTER(KeyDesc), C.POINTER(Csr), C.POINTER(Csr),
                                                 C.c_uint32, C.POINTER(Options), C.POINTER(vp)]),
            "g16_ctx_destroy": (None, [vp]),
            "g16_last_error": (C.c_char_p, [vp]),
            "g16_witness_map": (C.c_int, [vp, vp, C.c_size_t, vp]),
            "g16_msm_g1": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp]),
            "g16_msm_g2": (C.c_int, [vp, vp, C.c_size_t, vp]),
            "g16_prove": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_dev": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_batch_dev": (C.c_int, [vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]),
            "g16_witness_map_batch": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, vp]),
            "g16_prove_partial": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_partial_dev": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_finish": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
            "g16_dist_exchange_bytes": (C.c_size_t, [vp]),
            "g16_prove_dist_phase1": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_dist_phase2": (C.c_int, [vp, vp, vp]),
            "g16_prove_dist_phase3": (C.c_int, [vp, vp, vp]),
            "g16_set_profiling": (C.c_int, [vp, C.c_int]),
            "g16_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), _u32p]),
            "g16_stage_name": (C.c_char_p, [C.c_int]),
            "g16_multi_links": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_uint64)]),
            "g16_ctx_info": (C.c_int, [vp, _u32p]),
            "g16_witness_buffer": (vp, [vp]),
            "g16_witness_host_buffer": (vp, [vp]),
            "g16_verify_batch": (C.c_int, [C.c_int, C.POINTER(VkDesc), vp, vp, C.c_uint32, vp]),
            "g16_verify_aggregate": (C.c_int, [C.c_int, C.POINTER(VkDesc), vp, vp, C.c_uint32, vp, vp, vp]),
            "g16_verify_aggregate_keys": (C.c_int, [C.c_int, C.POINTER(C.POINTER(VkDesc)), vp, C.c_uint32, vp, vp,
                                                    vp, vp, vp]),
            "g16_verify_batch_keys": (C.c_int, [C.c_int, C.POINTER(C.POINTER(VkDesc)), vp, C.c_uint32, vp, vp, vp]),
            "g16_key_check": (C.c_int, [C.c_int, C.POINTER(KeyDesc), C.POINTER(VkDesc), vp, C.POINTER(KeyBadPoint),
                                        C.c_uint32, C.POINTER(KeyReportC)]),
            "g16_key_contribute": (C.c_int, [C.c_int, C.POINTER(KeyDesc), vp, vp, vp, vp, vp]),
            "g16_key_contribution_check": (C.c_int, [C.c_int, C.POINTER(KeyDesc), C.POINTER(KeyDesc), vp,
                                                     C.POINTER(KeyBadPoint), C.c_uint32,
                                                     C.POINTER(ContributionReportC)]),
            "g16_witness_upload": (C.c_int, [vp, vp, C.c_size_t]),
            "g16_witness_map_dev": (C.c_int, [vp, vp, C.c_size_t, vp]),
            "g16_msm_g1_dev": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp]),
            "g16_msm_g2_dev": (C.c_int, [vp, vp, C.c_size_t, vp]),
            "g16_ctx_create_multi": (C.c_int, [C.POINTER(KeyDesc), C.POINTER(Csr), C.POINTER(Csr), C.c_uint32,
                                               C.POINTER(C.c_int), C.c_int, C.POINTER(Options), C.POINTER(vp)]),
            "g16_dist_set_exchange_stream": (C.c_int, [vp, vp, C.c_int]),
            "g16_partial_buffer": (vp, [vp]),
            "g16_gather_buffer": (vp, [vp]),
            "g16_prove_finish_dev": (C.c_int, [vp, vp, vp, vp]),
            "g16_fft_in_place": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int]),
            "g16_dist_attach_rccl": (C.c_int, [vp, vp]),
            "g16_dist_rccl_ranks": (C.c_int, [vp]),
            "g16_prove_dist": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_check_satisfied": (C.c_int, [C.c_int, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr),
                                              C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_int64)]),
            "g16_zkey_write": (C.c_int, [C.c_char_p, C.POINTER(KeyDesc), vp, vp, C.POINTER(Csr),
                                         C.POINTER(Csr), C.c_uint32]),
            "g16_loader_last_error": (C.c_char_p, []),
            "g16_zkey_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
            "g16_zkey_open_mem": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
            "g16_zkey_close": (None, [vp]),
            "g16_zkey_header_get": (C.c_int, [vp, C.POINTER(ZkeyHeader)]),
            "g16_zkey_key": (C.c_int, [vp, C.POINTER(KeyDesc)]),
            "g16_zkey_ic": (vp, [vp, _u32p]),
            "g16_zkey_matrices": (C.c_int, [vp, C.POINTER(Matrices)]),
            "g16_r1cs_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
            "g16_r1cs_open_mem": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
            "g16_r1cs_close": (None, [vp]),
            "g16_r1cs_header_get": (C.c_int, [vp, C.POINTER(R1csHeader)]),
            "g16_r1cs_matrices": (C.c_int, [vp, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr)]),
            "g16_r1cs_wire_mapping": (vp, [vp, _u32p]),
            "g16_wtns_read": (C.c_int, [C.c_char_p, C.POINTER(vp), _u32p]),
            "g16_wtns_read_mem": (C.c_int, [vp, C.c_size_t, C.POINTER(vp), _u32p]),
            "g16_free": (None, [vp]),
            "g16_fr_from_canonical": (C.c_int, [vp, vp, C.c_size_t]),
            "g16_fr_to_canonical": (C.c_int, [vp, vp, C.c_size_t]),
            "g16_setup_create": (C.c_int, [C.c_int, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr),
                                           C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(vp)]),
            "g16_setup_create_ex": (C.c_int, [C.c_int, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr),
                                           C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, C.POINTER(vp)]),
            "g16_setup_destroy": (None, [vp]),
            "g16_setup_key": (C.c_int, [vp, C.POINTER(KeyDesc), C.POINTER(vp), _u32p, vp]),
            "g16_srs_create": (C.c_int, [C.c_int, C.c_uint32, vp, C.POINTER(vp)]),
            "g16_srs_desc_of": (C.c_int, [vp, C.POINTER(SrsDesc)]),
            "g16_srs_destroy": (None, [vp]),
            "g16_setup_from_srs": (C.c_int, [C.c_int, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr),
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SrsDesc), C.c_int,
                                             C.POINTER(vp)]),
            "g16_setup_from_srs_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_srs_check": (C.c_int, [C.c_int, C.POINTER(SrsDesc), vp, C.POINTER(KeyBadPoint), C.c_uint32,
                                        C.POINTER(SrsReportC)]),
            "g16_srs_contribute": (C.c_int, [C.c_int, C.POINTER(SrsDesc), vp, vp, vp, vp, vp, vp]),
            "g16_srs_contribute_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_ptau_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
            "g16_ptau_open_mem": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
            "g16_ptau_close": (None, [vp]),
            "g16_ptau_header_get": (C.c_int, [vp, C.POINTER(PtauHeader)]),
            "g16_ptau_srs": (C.c_int, [vp, C.POINTER(SrsDesc)]),
            "g16_ptau_write": (C.c_int, [C.c_char_p, C.POINTER(SrsDesc), C.c_uint32]),
            "g16_srs_prepare": (C.c_int, [C.c_int, C.POINTER(SrsDesc), C.c_uint32, vp, vp, vp, vp]),
            "g16_srs_prepare_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_srs_lagrange_check": (C.c_int, [C.c_int, C.POINTER(SrsDesc), C.POINTER(SrsLagrangeDesc), vp,
                                                 C.POINTER(KeyBadPoint), C.c_uint32,
                                                 C.POINTER(SrsLagrangeReportC)]),
            "g16_setup_from_prepared": (C.c_int, [C.c_int, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr),
                                                  C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SrsDesc),
                                                  C.POINTER(SrsLagrangeDesc), C.c_int, C.POINTER(vp)]),
            "g16_ptau_lagrange": (C.c_int, [vp, C.POINTER(SrsLagrangeDesc)]),
            "g16_ptau_write_prepared": (C.c_int, [C.c_char_p, C.POINTER(SrsDesc), C.POINTER(SrsLagrangeDesc),
                                                  C.c_uint32]),
            "g16_points_from_ark": (C.c_int, [C.c_int, C.c_int, C.c_uint32, vp, C.c_size_t, C.c_uint64, vp, C.c_size_t,
                                              vp, _u64p]),
            "g16_points_to_ark": (C.c_int, [C.c_int, C.c_int, C.c_uint32, vp, C.c_size_t, C.c_uint64, vp, C.c_size_t,
                                            _u64p]),
            "g16_ark_proofs_read": (C.c_int, [C.c_int, C.c_uint32, vp, C.c_uint64, vp, vp, _u64p]),
            "g16_ark_proofs_write": (C.c_int, [C.c_int, C.c_uint32, vp, C.c_uint64, vp, _u64p]),
            "g16_ark_pk_size": (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]),
            "g16_ark_pk_read": (C.c_int, [C.c_int, C.c_uint32, vp, C.c_size_t, C.POINTER(vp)]),
            "g16_ark_pk_key": (C.c_int, [vp, C.POINTER(KeyDesc), C.POINTER(VkDesc)]),
            "g16_ark_pk_close": (None, [vp]),
            "g16_ark_pk_write": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(KeyDesc), C.POINTER(VkDesc), C.c_uint64, vp,
                                           C.c_size_t]),
            "g16_ark_vk_size": (C.c_uint64, [C.c_uint32, C.c_uint64]),
            "g16_ark_vk_read": (C.c_int, [C.c_int, C.c_uint32, vp, C.c_size_t, C.POINTER(VkDesc), vp, C.c_uint32]),
            "g16_ark_vk_write": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(VkDesc), vp, C.c_size_t]),
            "g16_ark_pk_layout": (C.c_int, [vp, C.c_size_t, C.c_uint32, C.POINTER(ArkLayout)]),
            "g16_ark_vk_layout": (C.c_int, [vp, C.c_size_t, C.c_uint32, C.POINTER(ArkLayout)]),
            "g16_proofs_rerandomize": (C.c_int, [C.c_int, vp, vp, C.c_uint32, vp, vp, vp]),
            "g16_proofs_rerandomize_keys": (C.c_int, [C.c_int, vp, vp, C.c_uint32, vp, vp, vp, vp]),
            "g16_proofs_rerandomize_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_pvk_create": (C.c_int, [C.c_int, C.POINTER(VkDesc), C.POINTER(vp)]),
            "g16_pvk_destroy": (None, [vp]),
            "g16_pvk_alpha_beta": (C.c_int, [vp, vp]),
            "g16_verify_prepared": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
            "g16_pairing_check": (C.c_int, [C.c_int, vp, vp, C.c_uint32, vp]),
            "g16_verify_prepared_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_pvk_prepare_inputs": (C.c_int, [vp, vp, C.c_uint32, vp]),
            "g16_verify_prepared_inputs": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
            "g16_pairing_products": (C.c_int, [C.c_int, vp, vp, vp, C.c_uint32, vp, vp]),
            "g16_gt_multiexp": (C.c_int, [C.c_int, vp, vp, vp, C.c_uint32, vp]),
            "g16_gt_to_ark": (C.c_int, [C.c_int, vp, C.c_uint32, vp]),
            "g16_gt_from_ark": (C.c_int, [C.c_int, vp, C.c_uint32, C.c_int, vp, vp]),
            "g16_pvk_alpha_g1_beta_g2": (C.c_int, [vp, vp]),
            "g16_gt_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_fr_convert": (C.c_int, [C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_int64)]),
            "g16_fr_convert_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
            "g16_witness_upload_canonical": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_int64)]),
            "g16_prove_canonical": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
            "g16_prove_batch_canonical": (C.c_int, [vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp,
                                                    C.POINTER(C.c_int64)]),
            "g16_wtns_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
            "g16_wtns_open_mem": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
            "g16_wtns_count": (C.c_uint32, [vp]),
            "g16_wtns_values": (vp, [vp]),
            "g16_wtns_close": (None, [vp]),
            "g16_msm_bases_create": (C.c_int, [C.c_int, C.c_int, vp, C.c_size_t, C.c_uint32, C.POINTER(MsmOptions),
                                               C.POINTER(vp)]),
            "g16_msm_bases_destroy": (None, [vp]),
            "g16_msm_bases_info": (C.c_int, [vp, _u32p]),
            "g16_msm": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, vp]),
            "g16_msm_once": (C.c_int, [C.c_int, C.c_int, vp, vp, C.c_size_t, C.c_uint32, vp]),
            "g16_poly_divide_linear": (C.c_int, [C.c_int, vp, C.c_size_t, C.c_size_t, vp, C.c_uint32, vp, vp]),
            "g16_kzg_key_create": (C.c_int, [C.c_int, C.POINTER(SrsDesc), C.c_size_t, C.POINTER(MsmOptions),
                                             C.POINTER(vp)]),
            "g16_kzg_key_destroy": (None, [vp]),
            "g16_kzg_key_info": (C.c_int, [vp, _u32p]),
            "g16_kzg_commit": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, vp]),
            "g16_kzg_open": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_uint32, vp, vp]),
            "g16_kzg_verify": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, C.c_size_t, vp, vp]),
            "g16_kzg_times": (C.c_int, [C.POINTER(C.c_float), C.c_uint32]),
        }
        # measurement builds only (make EXTRA=-DG16_DEBUG_ABI; include/g16_amd.h): not an ABI symbol, never "missing"
        optional = {"g16_debug_alu_bench": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                                      C.POINTER(C.c_double), C.POINTER(C.c_double)])}
        for name, (res, args) in optional.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)
        self.missing = []
        for name, (res, args) in sig.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                self.missing.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def check(self, status, ctx=None, loader=False):
        if status == G16_OK:
            return
        if loader:
            msg = self.g16_loader_last_error().decode()
            raise SerializationError(status, msg)
        msg = self.g16_last_error(ctx).decode()
        if status == G16_ERR_DOMAIN_TOO_LARGE:
            raise SynthesisError(status, msg)
        raise G16Error(status, msg)


_default: Optional[Library] = None


def load(path: Optional[str] = None) -> Library:
    """The product library (cached).  Raises ImportError when it has not been built."""
    global _default
    if path is not None:
        return Library(path)
    if _default is None:
        _default = Library()
    return _default
