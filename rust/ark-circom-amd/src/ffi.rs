//! `extern "C"` declarations of include/g16_amd.h + include/g16_loaders.h, one for one.
//! tests/test_rust_shim.py (repository root) parses this file and asserts that the set of
//! functions and their arities equal the C headers'.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_float, c_int, c_void};

pub type g16_status = c_int;
pub const G16_OK: g16_status = 0;
pub const G16_ERR_INVALID: g16_status = 1;
pub const G16_ERR_DOMAIN_TOO_LARGE: g16_status = 2;
pub const G16_ERR_HIP: g16_status = 3;
pub const G16_ERR_NO_DEVICE: g16_status = 4;
pub const G16_ERR_IO: g16_status = 5;
pub const G16_ERR_INTERNAL: g16_status = 6;

pub const G16_PROOF_BYTES: usize = 256;
pub const G16_PARTIAL_BYTES: usize = 1024;
pub const G16_N_STAGES: usize = 10;
pub const G16_SHARD_AUTO: c_int = 0;
pub const G16_SHARD_POINTS: c_int = 1;
pub const G16_SHARD_BUCKETS: c_int = 2;
pub const G16_REDUCTION_CIRCOM: c_int = 0;
pub const G16_REDUCTION_LIBSNARK: c_int = 1;
pub const G16_QUERY_A: c_int = 0;
pub const G16_QUERY_B1: c_int = 1;
pub const G16_QUERY_L: c_int = 2;
pub const G16_QUERY_H: c_int = 3;
// g16_key_check: query ids, per-point reason bits, report.relations_failed bits
pub const G16_KEY_Q_A: u32 = 0;
pub const G16_KEY_Q_B1: u32 = 1;
pub const G16_KEY_Q_B2: u32 = 2;
pub const G16_KEY_Q_L: u32 = 3;
pub const G16_KEY_Q_H: u32 = 4;
pub const G16_KEY_Q_IC: u32 = 5;
pub const G16_KEY_Q_SINGLES: u32 = 6;
pub const G16_KEY_N_QUERIES: usize = 7;
pub const G16_KEY_BAD_NONCANONICAL: u32 = 1;
pub const G16_KEY_BAD_OFF_CURVE: u32 = 2;
pub const G16_KEY_BAD_SUBGROUP: u32 = 4;
pub const G16_KEY_PAIR_BETA: u32 = 1;
pub const G16_KEY_PAIR_DELTA: u32 = 2;
pub const G16_KEY_PAIR_B: u32 = 4;
pub const G16_KEY_VK_MISMATCH: u32 = 8;
// g16_key_contribution_check: report.relations_failed bits
pub const G16_CONTRIB_UNCHANGED_MISMATCH: u32 = 1;
pub const G16_CONTRIB_PAIR_DELTA: u32 = 2;
pub const G16_CONTRIB_PAIR_L: u32 = 4;
pub const G16_CONTRIB_PAIR_H: u32 = 8;
pub const G16_CONTRIB_DELTA_INFINITE: u32 = 16;

#[repr(C)]
pub struct g16_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_setup {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_srs {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_zkey {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_r1cs {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_ptau {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_wtns {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_ark_pk {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_pvk {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_msm_bases {
    _private: [u8; 0],
}
#[repr(C)]
pub struct g16_kzg_key {
    _private: [u8; 0],
}

pub const G16_GROUP_G1: c_int = 0;
pub const G16_GROUP_G2: c_int = 1;
pub const G16_MSM_SCALARS_CANONICAL: u32 = 1;
pub const G16_MSM_SCALARS_DEVICE: u32 = 2;
pub const G16_MSM_POINTS_DEVICE: u32 = 4;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct g16_msm_options {
    pub window_bits: c_int,
    pub planes: c_int,
    pub max_batch: c_int,
    pub validate: c_int,
}

// arkworks serialization (include/g16_amd.h): the extra per-point reason bit, the groups, the flags
pub const G16_KEY_BAD_ENCODING: u32 = 8;
pub const G16_POINT_G1: c_int = 0;
pub const G16_POINT_G2: c_int = 1;
pub const G16_ARK_COMPRESSED: u32 = 1;
pub const G16_ARK_VALIDATE: u32 = 2;
pub const G16_ARK_N_FIELDS: usize = 12;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_ark_layout {
    pub offset: [u64; G16_ARK_N_FIELDS],
    pub count: [u64; G16_ARK_N_FIELDS],
    pub total: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_csr {
    pub row_ptr: *const u32,
    pub col: *const u32,
    pub coeff: *const u64,
    pub nnz: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_key_desc {
    pub n_vars: u32,
    pub n_public: u32,
    pub domain_size: u32,
    pub a_query: *const u8,
    pub b_g1_query: *const u8,
    pub b_g2_query: *const u8,
    pub l_query: *const u8,
    pub h_query: *const u8,
    pub alpha_g1: [u8; 64],
    pub beta_g1: [u8; 64],
    pub delta_g1: [u8; 64],
    pub beta_g2: [u8; 128],
    pub delta_g2: [u8; 128],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct g16_options {
    pub device: c_int,
    pub rank: c_int,
    pub world: c_int,
    pub window_bits: c_int,
    pub planes: c_int,
    pub dist_wm: c_int,
    pub reduction: c_int,
    /// world > 1 / multi-device: G16_SHARD_AUTO, G16_SHARD_POINTS or G16_SHARD_BUCKETS
    pub shard: c_int,
    /// small keys: 0 = automatic fixed-base tables, > 0 require, < 0 never (include/g16_amd.h)
    pub fixed_tables: c_int,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_vk_desc {
    pub alpha_g1: [u8; 64],
    pub beta_g2: [u8; 128],
    pub gamma_g2: [u8; 128],
    pub delta_g2: [u8; 128],
    pub ic: *const u8,
    pub ic_count: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_srs_desc {
    pub n_tau_g1: u32,
    pub n_tau: u32,
    pub tau_g1: *const u8,
    pub tau_g2: *const u8,
    pub alpha_tau_g1: *const u8,
    pub beta_tau_g1: *const u8,
    pub beta_g2: [u8; 128],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_zkey_header {
    pub n8q: u32,
    pub n8r: u32,
    pub q: [u8; 32],
    pub r: [u8; 32],
    pub n_vars: u32,
    pub n_public: u32,
    pub domain_size: u32,
    pub power: u32,
    pub alpha_g1: [u8; 64],
    pub beta_g1: [u8; 64],
    pub beta_g2: [u8; 128],
    pub gamma_g2: [u8; 128],
    pub delta_g1: [u8; 64],
    pub delta_g2: [u8; 128],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_matrices {
    pub num_instance_variables: u32,
    pub num_witness_variables: u32,
    pub num_constraints: u32,
    pub a_num_non_zero: u64,
    pub b_num_non_zero: u64,
    pub a: g16_csr,
    pub b: g16_csr,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_r1cs_header {
    pub version: u32,
    pub field_size: u32,
    pub prime: [u8; 32],
    pub n_wires: u32,
    pub n_pub_out: u32,
    pub n_pub_in: u32,
    pub n_prv_in: u32,
    pub n_labels: u64,
    pub n_constraints: u32,
    pub num_inputs: u32,
    pub num_aux: u32,
    pub num_variables: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct g16_key_bad_point {
    pub query: u32,
    pub index: u32,
    pub reason: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct g16_key_report {
    pub ok: u8,
    pub relations_checked: u8,
    pub relations_failed: u32,
    pub n_points: [u64; G16_KEY_N_QUERIES],
    pub n_bad: [u64; G16_KEY_N_QUERIES],
    pub n_infinity: [u64; G16_KEY_N_QUERIES],
    pub n_listed: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct g16_contribution_report {
    pub ok: u8,
    pub relations_checked: u8,
    pub relations_failed: u32,
    pub n_bad_l: u64,
    pub n_bad_h: u64,
    pub n_listed: u32,
}

pub const G16_SRS_N_QUERIES: usize = 5;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct g16_srs_report {
    pub ok: u8,
    pub relations_checked: u8,
    pub relations_failed: u32,
    pub n_points: [u64; G16_SRS_N_QUERIES],
    pub n_bad: [u64; G16_SRS_N_QUERIES],
    pub n_infinity: [u64; G16_SRS_N_QUERIES],
    pub n_listed: u32,
}

/// Sections 12-15 of a prepared .ptau: tau_g1 in levels 0..=power+1, the others in levels 0..=power.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_srs_lagrange_desc {
    pub power: u32,
    pub tau_g1: *const u8,
    pub tau_g2: *const u8,
    pub alpha_tau_g1: *const u8,
    pub beta_tau_g1: *const u8,
}

pub const G16_LAGRANGE_N_ARRAYS: usize = 4;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct g16_srs_lagrange_report {
    pub ok: u8,
    pub relations_checked: u8,
    pub relations_failed: u32,
    pub n_points: [u64; G16_LAGRANGE_N_ARRAYS],
    pub n_bad: [u64; G16_LAGRANGE_N_ARRAYS],
    pub n_infinity: [u64; G16_LAGRANGE_N_ARRAYS],
    pub n_listed: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct g16_ptau_header {
    pub n8q: u32,
    pub q: [u8; 32],
    pub power: u32,
    pub ceremony_power: u32,
}

extern "C" {
    // ---- include/g16_amd.h ---------------------------------------------------------------------
    pub fn g16_ctx_create(key: *const g16_key_desc, a: *const g16_csr, b: *const g16_csr, num_constraints: u32, opt: *const g16_options, out: *mut *mut g16_ctx) -> g16_status;
    pub fn g16_ctx_create_sibling(
        donor: *mut g16_ctx,
        key: *const g16_key_desc,
        a: *const g16_csr,
        b: *const g16_csr,
        num_constraints: u32,
        opt: *const g16_options,
        out: *mut *mut g16_ctx,
    ) -> c_int;
    pub fn g16_ctx_destroy(ctx: *mut g16_ctx);
    pub fn g16_last_error(ctx: *const g16_ctx) -> *const c_char;
    pub fn g16_ctx_create_multi(key: *const g16_key_desc, a: *const g16_csr, b: *const g16_csr, num_constraints: u32, device_ids: *const c_int, n_dev: c_int, opt: *const g16_options, out: *mut *mut g16_ctx) -> g16_status;
    pub fn g16_witness_map(ctx: *mut g16_ctx, w: *const u64, n_vars: usize, h_out: *mut u64) -> g16_status;
    pub fn g16_msm_g1(ctx: *mut g16_ctx, which: c_int, scalars: *const u64, len: usize, out: *mut u8) -> g16_status;
    pub fn g16_msm_g2(ctx: *mut g16_ctx, scalars: *const u64, len: usize, out: *mut u8) -> g16_status;
    pub fn g16_witness_map_dev(ctx: *mut g16_ctx, w_dev: *const c_void, n_vars: usize, h_dev_out: *mut c_void) -> g16_status;
    pub fn g16_msm_g1_dev(ctx: *mut g16_ctx, which: c_int, scalars_dev: *const c_void, len: usize, out: *mut u8) -> g16_status;
    pub fn g16_msm_g2_dev(ctx: *mut g16_ctx, scalars_dev: *const c_void, len: usize, out: *mut u8) -> g16_status;
    pub fn g16_prove(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w: *const u64, n_vars: usize, proof_out: *mut u8) -> g16_status;
    pub fn g16_prove_dev(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w_dev: *const c_void, n_vars: usize, proof_out: *mut u8) -> g16_status;
    pub fn g16_prove_batch(ctx: *mut g16_ctx, count: usize, r: *const u64, s: *const u64, w: *const u64, n_vars: usize, proofs_out: *mut u8) -> g16_status;
    pub fn g16_prove_batch_dev(ctx: *mut g16_ctx, count: usize, r: *const u64, s: *const u64, w_dev: *const c_void, n_vars: usize, proofs_out: *mut u8) -> g16_status;
    pub fn g16_witness_map_batch(ctx: *mut g16_ctx, count: usize, w: *const u64, n_vars: usize, h_out: *mut u64) -> g16_status;
    pub fn g16_prove_partial(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w: *const u64, n_vars: usize, partial_out: *mut u8) -> g16_status;
    pub fn g16_prove_partial_dev(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w_dev: *const c_void, n_vars: usize, partial_out: *mut u8) -> g16_status;
    pub fn g16_prove_finish(ctx: *mut g16_ctx, r: *const u64, s: *const u64, partials: *const u8, world: c_int, proof_out: *mut u8) -> g16_status;
    pub fn g16_dist_set_exchange_stream(ctx: *mut g16_ctx, hip_stream: *mut c_void, enabled: c_int) -> g16_status;
    pub fn g16_partial_buffer(ctx: *mut g16_ctx) -> *mut c_void;
    pub fn g16_gather_buffer(ctx: *mut g16_ctx) -> *mut c_void;
    pub fn g16_prove_finish_dev(ctx: *mut g16_ctx, r: *const u64, s: *const u64, proof_out: *mut u8) -> g16_status;
    pub fn g16_dist_exchange_bytes(ctx: *const g16_ctx) -> usize;
    pub fn g16_prove_dist_phase1(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w_dev: *const c_void, n_vars: usize, send_dev: *mut c_void) -> g16_status;
    pub fn g16_prove_dist_phase2(ctx: *mut g16_ctx, recv_dev: *const c_void, send_dev: *mut c_void) -> g16_status;
    pub fn g16_prove_dist_phase3(ctx: *mut g16_ctx, recv_dev: *const c_void, partial_out: *mut u8) -> g16_status;
    pub fn g16_set_profiling(ctx: *mut g16_ctx, enabled: c_int) -> g16_status;
    pub fn g16_stage_times(ctx: *mut g16_ctx, ms: *mut c_float, launches: *mut u32) -> g16_status;
    pub fn g16_stage_name(stage: c_int) -> *const c_char;
    pub fn g16_ctx_info(ctx: *const g16_ctx, out: *mut u32) -> g16_status;
    pub fn g16_multi_links(ctx: *const g16_ctx, gbps: *mut f32, echo_us: *mut f32, cap: c_int, probe_bytes: *mut u64) -> g16_status;
    pub fn g16_witness_buffer(ctx: *mut g16_ctx) -> *mut c_void;
    pub fn g16_witness_upload(ctx: *mut g16_ctx, w: *const u64, n_vars: usize) -> g16_status;
    pub fn g16_fr_convert(device: c_int, in_le: *const u8, out_mont: *mut u64, n: usize, first_bad: *mut i64) -> g16_status;
    pub fn g16_fr_convert_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_witness_upload_canonical(ctx: *mut g16_ctx, w_le: *const u8, n_vars: usize, first_bad: *mut i64) -> g16_status;
    pub fn g16_prove_canonical(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w_le: *const u8, n_vars: usize, proof_out: *mut u8) -> g16_status;
    pub fn g16_prove_batch_canonical(ctx: *mut g16_ctx, count: usize, r: *const u64, s: *const u64, w_le: *const u8, n_vars: usize, proofs_out: *mut u8, first_bad: *mut i64) -> g16_status;
    pub fn g16_witness_host_buffer(ctx: *mut g16_ctx) -> *mut c_void;
    pub fn g16_check_satisfied(device: c_int, a: *const g16_csr, b: *const g16_csr, c: *const g16_csr, num_constraints: u32, w: *const u64, n_vars: usize, first_unsatisfied: *mut i64) -> g16_status;
    pub fn g16_verify_batch(device: c_int, vk: *const g16_vk_desc, proofs: *const u8, public_inputs: *const u64, n_proofs: u32, ok_out: *mut u8) -> g16_status;
    pub fn g16_verify_aggregate(device: c_int, vk: *const g16_vk_desc, proofs: *const u8, public_inputs: *const u64, n_proofs: u32, rho: *const u64, ok_out: *mut u8, structural_out: *mut u8) -> g16_status;
    pub fn g16_verify_aggregate_keys(device: c_int, vks: *const *const g16_vk_desc, counts: *const u32, n_keys: u32, proofs: *const u8, public_inputs: *const u64, rho: *const u64, ok_out: *mut u8, structural_out: *mut u8) -> g16_status;
    pub fn g16_verify_batch_keys(device: c_int, vks: *const *const g16_vk_desc, counts: *const u32, n_keys: u32, proofs: *const u8, public_inputs: *const u64, ok_out: *mut u8) -> g16_status;
    pub fn g16_key_check(device: c_int, key: *const g16_key_desc, vk: *const g16_vk_desc, rho: *const u64, bad_out: *mut g16_key_bad_point, bad_cap: u32, report: *mut g16_key_report) -> g16_status;
    pub fn g16_key_contribute(device: c_int, key: *const g16_key_desc, d: *const u64, l_out: *mut u8, h_out: *mut u8, delta_g1_out: *mut u8, delta_g2_out: *mut u8) -> g16_status;
    pub fn g16_key_contribution_check(device: c_int, before: *const g16_key_desc, after: *const g16_key_desc, rho: *const u64, bad_out: *mut g16_key_bad_point, bad_cap: u32, report: *mut g16_contribution_report) -> g16_status;
    pub fn g16_dist_attach_rccl(ctx: *mut g16_ctx, nccl_comm: *mut c_void) -> g16_status;
    pub fn g16_dist_rccl_ranks(ctx: *const g16_ctx) -> c_int;
    pub fn g16_prove_dist(ctx: *mut g16_ctx, r: *const u64, s: *const u64, w_dev: *const c_void, n_vars: usize, proof_out: *mut u8) -> g16_status;
    pub fn g16_fft_in_place(device: c_int, data: *mut u64, log_n: c_int, inverse: c_int, impl_: c_int) -> g16_status;
    pub fn g16_setup_create(device: c_int, at: *const g16_csr, bt: *const g16_csr, ct: *const g16_csr, n_vars: u32, n_public: u32, num_constraints: u32, toxic: *const u64, out: *mut *mut g16_setup) -> g16_status;
    pub fn g16_setup_create_ex(device: c_int, at: *const g16_csr, bt: *const g16_csr, ct: *const g16_csr, n_vars: u32, n_public: u32, num_constraints: u32, toxic: *const u64, reduction: c_int, out: *mut *mut g16_setup) -> g16_status;
    pub fn g16_setup_key(s: *mut g16_setup, key: *mut g16_key_desc, ic: *mut *const u8, ic_count: *mut u32, gamma_g2: *mut u8) -> g16_status;
    pub fn g16_setup_destroy(s: *mut g16_setup);
    pub fn g16_srs_create(device: c_int, log2_domain: u32, toxic: *const u64, out: *mut *mut g16_srs) -> g16_status;
    pub fn g16_srs_desc_of(s: *mut g16_srs, out: *mut g16_srs_desc) -> g16_status;
    pub fn g16_srs_destroy(s: *mut g16_srs);
    pub fn g16_setup_from_srs(device: c_int, at: *const g16_csr, bt: *const g16_csr, ct: *const g16_csr, n_vars: u32, n_public: u32, num_constraints: u32, srs: *const g16_srs_desc, reduction: c_int, out: *mut *mut g16_setup) -> g16_status;
    pub fn g16_setup_from_srs_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_srs_check(device: c_int, srs: *const g16_srs_desc, rho: *const u64, bad_out: *mut g16_key_bad_point, bad_cap: u32, report: *mut g16_srs_report) -> g16_status;
    pub fn g16_srs_contribute(device: c_int, srs: *const g16_srs_desc, secrets: *const u64, tau_g1_out: *mut u8, tau_g2_out: *mut u8, alpha_tau_g1_out: *mut u8, beta_tau_g1_out: *mut u8, beta_g2_out: *mut u8) -> g16_status;
    pub fn g16_srs_contribute_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_srs_prepare(device: c_int, srs: *const g16_srs_desc, power: u32, tau_g1_out: *mut u8, tau_g2_out: *mut u8, alpha_tau_g1_out: *mut u8, beta_tau_g1_out: *mut u8) -> g16_status;
    pub fn g16_srs_prepare_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_srs_lagrange_check(device: c_int, srs: *const g16_srs_desc, lag: *const g16_srs_lagrange_desc, rho: *const u64, bad_out: *mut g16_key_bad_point, bad_cap: u32, report: *mut g16_srs_lagrange_report) -> g16_status;
    pub fn g16_setup_from_prepared(device: c_int, at: *const g16_csr, bt: *const g16_csr, ct: *const g16_csr, n_vars: u32, n_public: u32, num_constraints: u32, srs: *const g16_srs_desc, lag: *const g16_srs_lagrange_desc, reduction: c_int, out: *mut *mut g16_setup) -> g16_status;
    pub fn g16_points_from_ark(device: c_int, group: c_int, flags: u32, input: *const u8, in_stride: usize, n: u64, out: *mut u8, out_stride: usize, reason_out: *mut u8, n_bad: *mut u64) -> g16_status;
    pub fn g16_points_to_ark(device: c_int, group: c_int, flags: u32, input: *const u8, in_stride: usize, n: u64, out: *mut u8, out_stride: usize, n_bad: *mut u64) -> g16_status;
    pub fn g16_ark_proofs_read(device: c_int, flags: u32, input: *const u8, n: u64, proofs_out: *mut u8, reason_out: *mut u8, n_bad: *mut u64) -> g16_status;
    pub fn g16_ark_proofs_write(device: c_int, flags: u32, proofs: *const u8, n: u64, out: *mut u8, n_bad: *mut u64) -> g16_status;
    pub fn g16_ark_pk_size(flags: u32, n_vars: u64, n_public: u64, h_len: u64) -> u64;
    pub fn g16_ark_pk_read(device: c_int, flags: u32, data: *const u8, len: usize, out: *mut *mut g16_ark_pk) -> g16_status;
    pub fn g16_ark_pk_key(h: *const g16_ark_pk, key: *mut g16_key_desc, vk: *mut g16_vk_desc) -> g16_status;
    pub fn g16_ark_pk_close(h: *mut g16_ark_pk);
    pub fn g16_ark_pk_write(device: c_int, flags: u32, key: *const g16_key_desc, vk: *const g16_vk_desc, h_len: u64, out: *mut u8, cap: usize) -> g16_status;
    pub fn g16_ark_vk_size(flags: u32, n_public: u64) -> u64;
    pub fn g16_ark_vk_read(device: c_int, flags: u32, data: *const u8, len: usize, vk: *mut g16_vk_desc, ic_out: *mut u8, ic_cap: u32) -> g16_status;
    pub fn g16_ark_vk_write(device: c_int, flags: u32, vk: *const g16_vk_desc, out: *mut u8, cap: usize) -> g16_status;
    pub fn g16_proofs_rerandomize(device: c_int, delta_g2: *const u8, proofs: *const u8, n_proofs: u32, scalars: *const u64, proofs_out: *mut u8, ok_out: *mut u8) -> g16_status;
    pub fn g16_proofs_rerandomize_keys(device: c_int, delta_g2s: *const u8, counts: *const u32, n_keys: u32, proofs: *const u8, scalars: *const u64, proofs_out: *mut u8, ok_out: *mut u8) -> g16_status;
    pub fn g16_proofs_rerandomize_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_pvk_create(device: c_int, vk: *const g16_vk_desc, out: *mut *mut g16_pvk) -> g16_status;
    pub fn g16_pvk_destroy(pvk: *mut g16_pvk);
    pub fn g16_pvk_alpha_beta(pvk: *const g16_pvk, out: *mut u8) -> g16_status;
    pub fn g16_verify_prepared(pvk: *mut g16_pvk, proofs: *const u8, public_inputs: *const u64, n_proofs: u32, ok_out: *mut u8) -> g16_status;
    pub fn g16_pairing_check(device: c_int, g1: *const u8, g2: *const u8, n_pairs: u32, ok_out: *mut u8) -> g16_status;
    pub fn g16_verify_prepared_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_pvk_prepare_inputs(pvk: *mut g16_pvk, public_inputs: *const u64, n: u32, out: *mut u8) -> g16_status;
    pub fn g16_verify_prepared_inputs(pvk: *mut g16_pvk, proofs: *const u8, prepared: *const u8, n_proofs: u32, ok_out: *mut u8) -> g16_status;
    pub fn g16_pairing_products(device: c_int, g1: *const u8, g2: *const u8, offsets: *const u32, n_products: u32, gt_out: *mut u8, ok_out: *mut u8) -> g16_status;
    pub fn g16_gt_multiexp(device: c_int, gt: *const u8, scalars: *const u64, offsets: *const u32, n_out: u32, gt_out: *mut u8) -> g16_status;
    pub fn g16_gt_to_ark(device: c_int, gt: *const u8, n: u32, out: *mut u8) -> g16_status;
    pub fn g16_gt_from_ark(device: c_int, input: *const u8, n: u32, validate: c_int, gt_out: *mut u8, reason_out: *mut u8) -> g16_status;
    pub fn g16_pvk_alpha_g1_beta_g2(pvk: *const g16_pvk, out: *mut u8) -> g16_status;
    pub fn g16_gt_times(ms: *mut c_float, cap: u32) -> g16_status;
    pub fn g16_msm_bases_create(device: c_int, group: c_int, points: *const c_void, n: usize, flags: u32, opt: *const g16_msm_options, out: *mut *mut g16_msm_bases) -> g16_status;
    pub fn g16_msm_bases_destroy(h: *mut g16_msm_bases);
    pub fn g16_msm_bases_info(h: *const g16_msm_bases, out: *mut u32) -> g16_status;
    pub fn g16_msm(h: *mut g16_msm_bases, scalars: *const c_void, len: usize, count: usize, stride: usize, flags: u32, out: *mut u8) -> g16_status;
    pub fn g16_msm_once(device: c_int, group: c_int, points: *const c_void, scalars: *const c_void, n: usize, flags: u32, out: *mut u8) -> g16_status;
    pub fn g16_poly_divide_linear(device: c_int, coeffs: *const c_void, n: usize, count: usize, z: *const c_void, flags: u32, quot_out: *mut c_void, rem_out: *mut u64) -> g16_status;
    pub fn g16_kzg_key_create(device: c_int, srs: *const g16_srs_desc, max_len: usize, opt: *const g16_msm_options, out: *mut *mut g16_kzg_key) -> g16_status;
    pub fn g16_kzg_key_destroy(k: *mut g16_kzg_key);
    pub fn g16_kzg_key_info(k: *const g16_kzg_key, out: *mut u32) -> g16_status;
    pub fn g16_kzg_commit(k: *mut g16_kzg_key, coeffs: *const c_void, len: usize, count: usize, stride: usize, flags: u32, out: *mut u8) -> g16_status;
    pub fn g16_kzg_open(k: *mut g16_kzg_key, coeffs: *const c_void, len: usize, count: usize, stride: usize, z: *const c_void, flags: u32, y_out: *mut u64, proof_out: *mut u8) -> g16_status;
    pub fn g16_kzg_verify(device: c_int, tau_g2: *const u8, commitments: *const u8, z: *const u64, y: *const u64, proofs: *const u8, n: usize, rho: *const u64, ok_out: *mut u8) -> g16_status;
    pub fn g16_kzg_times(ms: *mut c_float, cap: u32) -> g16_status;

    // ---- include/g16_loaders.h -----------------------------------------------------------------
    pub fn g16_loader_last_error() -> *const c_char;
    pub fn g16_ark_pk_layout(data: *const u8, len: usize, flags: u32, out: *mut g16_ark_layout) -> g16_status;
    pub fn g16_ark_vk_layout(data: *const u8, len: usize, flags: u32, out: *mut g16_ark_layout) -> g16_status;
    pub fn g16_ptau_open(path: *const c_char, out: *mut *mut g16_ptau) -> g16_status;
    pub fn g16_ptau_open_mem(data: *const u8, len: usize, out: *mut *mut g16_ptau) -> g16_status;
    pub fn g16_ptau_close(p: *mut g16_ptau);
    pub fn g16_ptau_header_get(p: *const g16_ptau, out: *mut g16_ptau_header) -> g16_status;
    pub fn g16_ptau_srs(p: *const g16_ptau, out: *mut g16_srs_desc) -> g16_status;
    pub fn g16_ptau_write(path: *const c_char, srs: *const g16_srs_desc, power: u32) -> g16_status;
    pub fn g16_ptau_lagrange(p: *const g16_ptau, out: *mut g16_srs_lagrange_desc) -> g16_status;
    pub fn g16_ptau_write_prepared(path: *const c_char, srs: *const g16_srs_desc, lag: *const g16_srs_lagrange_desc, power: u32) -> g16_status;
    pub fn g16_zkey_open(path: *const c_char, out: *mut *mut g16_zkey) -> g16_status;
    pub fn g16_zkey_open_mem(data: *const u8, len: usize, out: *mut *mut g16_zkey) -> g16_status;
    pub fn g16_zkey_close(z: *mut g16_zkey);
    pub fn g16_zkey_header_get(z: *const g16_zkey, out: *mut g16_zkey_header) -> g16_status;
    pub fn g16_zkey_key(z: *const g16_zkey, out: *mut g16_key_desc) -> g16_status;
    pub fn g16_zkey_ic(z: *const g16_zkey, count: *mut u32) -> *const u8;
    pub fn g16_zkey_matrices(z: *mut g16_zkey, out: *mut g16_matrices) -> g16_status;
    pub fn g16_zkey_write(path: *const c_char, key: *const g16_key_desc, ic: *const u8, gamma_g2: *const u8, a: *const g16_csr, b: *const g16_csr, num_constraints: u32) -> g16_status;
    pub fn g16_r1cs_open(path: *const c_char, out: *mut *mut g16_r1cs) -> g16_status;
    pub fn g16_r1cs_open_mem(data: *const u8, len: usize, out: *mut *mut g16_r1cs) -> g16_status;
    pub fn g16_r1cs_close(r: *mut g16_r1cs);
    pub fn g16_r1cs_header_get(r: *const g16_r1cs, out: *mut g16_r1cs_header) -> g16_status;
    pub fn g16_r1cs_matrices(r: *const g16_r1cs, a: *mut g16_csr, b: *mut g16_csr, c: *mut g16_csr) -> g16_status;
    pub fn g16_r1cs_wire_mapping(r: *const g16_r1cs, count: *mut u32) -> *const u64;
    pub fn g16_wtns_read(path: *const c_char, out: *mut *mut u64, n: *mut u32) -> g16_status;
    pub fn g16_wtns_read_mem(data: *const u8, len: usize, out: *mut *mut u64, n: *mut u32) -> g16_status;
    pub fn g16_free(p: *mut c_void);
    pub fn g16_wtns_open(path: *const c_char, out: *mut *mut g16_wtns) -> g16_status;
    pub fn g16_wtns_open_mem(data: *const u8, len: usize, out: *mut *mut g16_wtns) -> g16_status;
    pub fn g16_wtns_count(w: *const g16_wtns) -> u32;
    pub fn g16_wtns_values(w: *const g16_wtns) -> *const u8;
    pub fn g16_wtns_close(w: *mut g16_wtns);
    pub fn g16_fr_from_canonical(input: *const u8, out: *mut u64, n: usize) -> g16_status;
    pub fn g16_fr_to_canonical(input: *const u64, out: *mut u8, n: usize) -> g16_status;
}
