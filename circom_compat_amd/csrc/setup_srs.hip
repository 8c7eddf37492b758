// setup_srs.hip -- Groth16 setup from a powers-of-tau string (SRS): the initial key (gamma = delta = 1) of a
// circuit with nobody knowing tau, alpha or beta.  What `snarkjs zkey new <r1cs> <ptau>` computes of the points;
// the math is keygen.hip's header comment with group elements where that file has scalars:
//   Lag1[j]  = L_j(tau) G1       = (inverse size-n transform of tau_g1[0..n))_j        natural order, 1/n included
//   LagA1, LagB1, Lag2           the same transform of alpha_tau_g1, beta_tau_g1, tau_g2 (over G2)
//   a_query[i] = sum_j at[i][j] Lag1[j],  b_g1_query / b_g2_query[i] = sum_j bt[i][j] Lag1[j] / Lag2[j]
//   K_i = sum_j at[i][j] LagB1[j] + bt[i][j] LagA1[j] + ct[i][j] Lag1[j]       IC = K_0..n_public, l_query the rest
//   h_query[i] (circom)   = entry 2i+1 of the inverse size-2n transform of tau_g1[0..2n-1) | infinity.  The odd
//                           entries of a size-2n DIF are the size-n transform of its first stage's lower half:
//                           D[j] = omega_2n^-j / (2n) (tau_g1[j] - tau_g1[j+n]) -- one stage and a size-n transform
//   h_query[i] (libsnark) = tau_g1[i+n] - tau_g1[i], i < n-1; entry n-1 is infinity
// The transform itself (k_naf, k_gntt_stage, k_scale, k_affine) is gtransform.h; the kernels of this file:
//   k_h_first     the first stage of the H transform (or the libsnark differences) straight from the affine SRS
//   k_comb_rows / k_comb_chunk / k_comb_fold   sum_j coeff Base[j] per wire: a lane per short row; long rows
//                 (the constant wire: a term per constraint) in chunks of SS_CHUNK terms, one block each, then
//                 one block per long row over its partial sums.  Coefficient 1 / r-1 is one mixed addition /
//                 subtraction, anything else a double-and-add from the top bit of min(c, r - c).
// g16_srs_create mints an SRS from a known trapdoor with keygen.hip's k_powers / k_fb_mul (tests, synthetic keys).
#include <memory>

#include "gtransform.h"

struct g16_srs {
  uint32_t n_tau_g1 = 0, n_tau = 0;
  std::vector<uint8_t> tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1;
  uint8_t beta_g2[128];
};

namespace g16 {
namespace {

constexpr uint32_t SS_SHORT_MAX = 32;  // terms a single lane walks; longer rows go through the chunk kernels
constexpr uint32_t SS_CHUNK = 1024;    // terms per block of k_comb_chunk

// circom (c != NULL): out[j] = c[j] (tau[j] - tau[j+n]), tau[2n-1] = infinity; libsnark: tau[j+n] - tau[j], j < n-1
__global__ void __launch_bounds__(SS_BLOCK) k_h_first(const G1Affine* tau, uint32_t n, const Naf* c, G1XYZZ29* out) {
  const uint32_t j = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j >= n) return;
  const bool has_hi = j + 1 < n;  // index j + n <= 2n - 2
  const Aff29<Fq29> lo = affine_from_mont256<Fq>(tau[j]);
  Aff29<Fq29> hi{Fq29::zero(), Fq29::zero(), true};
  if (has_hi) hi = affine_from_mont256<Fq>(tau[(size_t)j + n]);
  if (c) {
    G1XYZZ29 D = G1XYZZ29::from_affine(lo);
    D.madd(aff_neg(hi));
    out[j] = mul_naf(D, c + j);
  } else {
    G1XYZZ29 D = G1XYZZ29::from_affine(hi);
    if (has_hi) D.madd(aff_neg(lo));
    out[j] = D;
  }
}

// the zkey encoding (a level of a Lagrange set as it stands) -> the packed internal form the combinations read
template <class F>
__global__ void __launch_bounds__(SS_BLOCK) k_pack_affine(const Affine<F>* in, uint32_t n, Affine<F>* out) {
  const uint32_t i = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = store_packed_affine<F>(affine_from_mont256<F>(in[i]));
}

// ---- sparse point combinations ---------------------------------------------------------------------------
template <class F>
struct CombArgs {
  const uint32_t* rowptr[3];
  const uint32_t* col[3];
  const Fr* val[3];
  const Affine<F>* base[3];  // packed internal form, natural order
  uint32_t nm;
};
struct CombChunk {
  uint32_t q, lo, hi;  // terms [lo, hi) of matrix q
};
struct CombLong {
  uint32_t row, part_lo, part_hi;
};

// acc += c P.  c = 1 / r - 1: one mixed addition of +-P.  Otherwise |c| = min(c, r - c) roughly (c >= 2^253 is
// taken as r - c negated) drives a NAF double-and-add of mixed additions that starts at its top word: a small
// coefficient of either sign costs a few steps, a full-width one the whole ladder.
template <class F>
__device__ __forceinline__ void comb_term(XYZZ29<typename Lazy<F>::type>& acc, const Affine<F>& raw, const Fr& coeff) {
  using LF = typename Lazy<F>::type;
  Aff29<LF> p = load_packed_affine<F>(raw);
  if (p.inf) return;
  U256 k = coeff.to_canonical();
  if ((k.v[7] >> 29) & 1u) {  // k >= 2^253: r - k < 2^253
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t d = (uint64_t)FrParams::MOD[i] - k.v[i] - br;
      k.v[i] = (uint32_t)d;
      br = (d >> 32) & 1;
    }
    p = aff_neg(p);
  }
  uint32_t hi = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i) hi |= k.v[i];
  if (!hi && k.v[0] <= 1u) {
    if (k.v[0]) acc.madd(p);
    return;
  }
  Naf s = naf_of(k);
  const LF ny = p.y.neg().carry();
  XYZZ29<LF> t = XYZZ29<LF>::infinity();
#pragma unroll 1
  for (int w = 0; w < 8; ++w) {
    const uint32_t pw = s.pos[7], nw = s.neg[7];
#pragma unroll
    for (int i = 7; i > 0; --i) {  // the masks move up a word per step: no register array indexed by w
      s.pos[i] = s.pos[i - 1];
      s.neg[i] = s.neg[i - 1];
    }
    if (!(pw | nw) && t.is_inf()) continue;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      t.dbl_in_place();
      const uint32_t m = 1u << b;
      if ((pw | nw) & m) t.madd(Aff29<LF>{p.x, (nw & m) ? ny : p.y, false});
    }
  }
  acc.add(t);
}

template <class F>
__global__ void __launch_bounds__(SS_BLOCK) k_comb_rows(CombArgs<F> A, uint32_t rows,
                                                        XYZZ29<typename Lazy<F>::type>* work) {
  const uint32_t i = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (i >= rows) return;
  uint64_t total = 0;
  for (uint32_t q = 0; q < A.nm; ++q) total += A.rowptr[q][i + 1] - A.rowptr[q][i];
  if (total > SS_SHORT_MAX) return;  // k_comb_fold writes this row
  XYZZ29<typename Lazy<F>::type> acc = XYZZ29<typename Lazy<F>::type>::infinity();
#pragma unroll 1
  for (uint32_t q = 0; q < A.nm; ++q) {
    const uint32_t lo = A.rowptr[q][i], hi = A.rowptr[q][i + 1];
#pragma unroll 1
    for (uint32_t e = lo; e < hi; ++e) comb_term<F>(acc, A.base[q][A.col[q][e]], A.val[q][e]);
  }
  work[i] = acc;
}

// sh[0] <- sum of the block's terms (fixed tree)
template <class T>
__device__ __forceinline__ void ss_block_sum(T* sh, T v) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
#pragma unroll 1
  for (uint32_t s = SS_BLOCK / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      v.add(sh[t + s]);
      sh[t] = v;
    }
  }
  __syncthreads();
}

template <class F>
__global__ void __launch_bounds__(SS_BLOCK) k_comb_chunk(CombArgs<F> A, const CombChunk* chunks,
                                                         XYZZ29<typename Lazy<F>::type>* part) {
  using P = XYZZ29<typename Lazy<F>::type>;
  __shared__ P sh[SS_BLOCK];
  const CombChunk c = chunks[blockIdx.x];
  P acc = P::infinity();
#pragma unroll 1
  for (uint32_t e = c.lo + threadIdx.x; e < c.hi; e += SS_BLOCK)
    comb_term<F>(acc, A.base[c.q][A.col[c.q][e]], A.val[c.q][e]);
  ss_block_sum(sh, acc);
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

template <class LF>
__global__ void __launch_bounds__(SS_BLOCK) k_comb_fold(const CombLong* rows, const XYZZ29<LF>* part,
                                                        XYZZ29<LF>* work) {
  __shared__ XYZZ29<LF> sh[SS_BLOCK];
  const CombLong r = rows[blockIdx.x];
  XYZZ29<LF> acc = XYZZ29<LF>::infinity();
#pragma unroll 1
  for (uint32_t k = r.part_lo + threadIdx.x; k < r.part_hi; k += SS_BLOCK) acc.add(part[k]);
  ss_block_sum(sh, acc);
  if (threadIdx.x == 0) work[r.row] = sh[0];
}

// ---- host side ---------------------------------------------------------------------------------------
enum { T_UPLOAD = 0, T_NTT_G1, T_NTT_G2, T_H, T_AFFINE, T_COMB, T_DOWNLOAD, T_COUNT };

thread_local PhaseTimes<T_COUNT> t_phase;

struct DevCsr {
  DevBuf<uint32_t> rowptr, col;
  DevBuf<Fr> val;
  const g16_csr* host = nullptr;
  void upload(const g16_csr* c, uint32_t rows) {
    host = c;
    rowptr.alloc((size_t)rows + 1);
    col.alloc(c->nnz ? c->nnz : 1);
    val.alloc(c->nnz ? c->nnz : 1);
    G16_HIP(hipMemcpy(rowptr.p, c->row_ptr, ((size_t)rows + 1) * 4, hipMemcpyHostToDevice));
    if (c->nnz) {
      G16_HIP(hipMemcpy(col.p, c->col, c->nnz * 4, hipMemcpyHostToDevice));
      G16_HIP(hipMemcpy(val.p, c->coeff, c->nnz * 32, hipMemcpyHostToDevice));
    }
  }
};

// work[i] = sum over the nm (matrix, base) pairs of row i
template <class F>
void combine(const DevCsr* const* mats, const Affine<F>* const* bases, uint32_t nm, uint32_t rows,
             XYZZ29<typename Lazy<F>::type>* work, hipStream_t s) {
  using P = XYZZ29<typename Lazy<F>::type>;
  if (!rows) return;
  CombArgs<F> A;
  memset(&A, 0, sizeof A);
  A.nm = nm;
  for (uint32_t q = 0; q < nm; ++q) {
    A.rowptr[q] = mats[q]->rowptr.p;
    A.col[q] = mats[q]->col.p;
    A.val[q] = mats[q]->val.p;
    A.base[q] = bases[q];
  }
  std::vector<CombChunk> chunks;
  std::vector<CombLong> longs;
  for (uint32_t i = 0; i < rows; ++i) {
    uint64_t total = 0;
    for (uint32_t q = 0; q < nm; ++q) total += mats[q]->host->row_ptr[i + 1] - mats[q]->host->row_ptr[i];
    if (total <= SS_SHORT_MAX) continue;
    CombLong L{i, (uint32_t)chunks.size(), 0};
    for (uint32_t q = 0; q < nm; ++q) {
      const uint32_t lo = mats[q]->host->row_ptr[i], hi = mats[q]->host->row_ptr[i + 1];
      for (uint64_t at = lo; at < hi; at += SS_CHUNK)
        chunks.push_back(CombChunk{q, (uint32_t)at, (uint32_t)(hi - at < SS_CHUNK ? hi : at + SS_CHUNK)});
    }
    L.part_hi = (uint32_t)chunks.size();
    longs.push_back(L);
  }
  G16_LAUNCH((k_comb_rows<F>), ceil_div(rows, SS_BLOCK), SS_BLOCK, 0, s, A, rows, work);
  if (!longs.empty()) {
    DevBuf<CombChunk> dch;
    DevBuf<CombLong> dlo;
    DevBuf<P> part;
    dch.alloc(chunks.size());
    dlo.alloc(longs.size());
    part.alloc(chunks.size());
    G16_HIP(hipMemcpy(dch.p, chunks.data(), chunks.size() * sizeof(CombChunk), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dlo.p, longs.data(), longs.size() * sizeof(CombLong), hipMemcpyHostToDevice));
    G16_LAUNCH((k_comb_chunk<F>), (uint32_t)chunks.size(), SS_BLOCK, 0, s, A, (const CombChunk*)dch.p, part.p);
    G16_LAUNCH((k_comb_fold<typename Lazy<F>::type>), (uint32_t)longs.size(), SS_BLOCK, 0, s,
               (const CombLong*)dlo.p, (const P*)part.p, work);
    G16_HIP(hipStreamSynchronize(s));  // the buffers above are released at the end of this scope
  }
}

Fr fr_of_limbs(const uint64_t* p) {
  Fr a;
  memcpy(a.v, p, 32);
  return a;
}

}  // namespace
}  // namespace g16

using namespace g16;

// lag == NULL: the Lagrange bases and the circom H by the group transform; else read from the prepared set
static g16_status setup_impl(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct, uint32_t n_vars,
                             uint32_t n_public, uint32_t num_constraints, const g16_srs_desc* srs,
                             const g16_srs_lagrange_desc* lag, int reduction, g16_setup** out);

extern "C" {

g16_status g16_srs_create(int device, uint32_t log2_domain, const uint64_t* toxic, g16_srs** out) {
  if (!toxic || !out) return G16_ERR_INVALID;
  *out = nullptr;
  if (log2_domain > 27) return G16_ERR_DOMAIN_TOO_LARGE;
  if (const g16_status ds = device_ok(device)) return ds;
  std::unique_ptr<g16_srs> owned(new g16_srs());  // freed on every way out but the last
  g16_srs* S = owned.get();
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    const uint32_t n = 1u << log2_domain, n1 = 2 * n - 1;
    const Fr tau = fr_of_limbs(toxic), alpha = fr_of_limbs(toxic + 4), beta = fr_of_limbs(toxic + 8);
    FixedBase fb;
    fb.build(s);
    DevBuf<Fr> sc;
    DevBuf<G1Affine> o1;
    DevBuf<G2Affine> o2;
    sc.alloc(n1);
    o1.alloc(n1);
    o2.alloc(n);
    auto g1_powers = [&](const Fr& scale, uint32_t count, std::vector<uint8_t>& dst) {
      fr_powers(tau, scale, sc.p, count, count, s);
      fb.mul_g1(sc.p, count, o1.p, s);
      G16_HIP(hipStreamSynchronize(s));
      fetch(dst, o1.p, count);
    };
    g1_powers(Fr::one(), n1, S->tau_g1);
    g1_powers(alpha, n, S->alpha_tau_g1);
    g1_powers(beta, n, S->beta_tau_g1);
    fr_powers(tau, Fr::one(), sc.p, n, n, s);
    fb.mul_g2(sc.p, n, o2.p, s);
    G16_HIP(hipStreamSynchronize(s));
    fetch(S->tau_g2, o2.p, n);
    G16_HIP(hipMemcpy(sc.p, &beta, sizeof beta, hipMemcpyHostToDevice));
    fb.mul_g2(sc.p, 1, o2.p, s);
    G16_HIP(hipStreamSynchronize(s));
    G16_HIP(hipMemcpy(S->beta_g2, o2.p, 128, hipMemcpyDeviceToHost));
    G16_HIP(hipMemset(sc.p, 0, sc.bytes()));  // the powers of the trapdoor do not outlive the call
    S->n_tau_g1 = n1;
    S->n_tau = n;
    *out = owned.release();
    return G16_OK;
  });
}

g16_status g16_srs_desc_of(g16_srs* s, g16_srs_desc* out) {
  if (!s || !out) return G16_ERR_INVALID;
  memset(out, 0, sizeof *out);
  out->n_tau_g1 = s->n_tau_g1;
  out->n_tau = s->n_tau;
  out->tau_g1 = s->tau_g1.data();
  out->tau_g2 = s->tau_g2.data();
  out->alpha_tau_g1 = s->alpha_tau_g1.data();
  out->beta_tau_g1 = s->beta_tau_g1.data();
  memcpy(out->beta_g2, s->beta_g2, 128);
  return G16_OK;
}

void g16_srs_destroy(g16_srs* s) { delete s; }

g16_status g16_setup_from_srs(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct, uint32_t n_vars,
                              uint32_t n_public, uint32_t num_constraints, const g16_srs_desc* srs, int reduction,
                              g16_setup** out) {
  return setup_impl(device, at, bt, ct, n_vars, n_public, num_constraints, srs, nullptr, reduction, out);
}

g16_status g16_setup_from_prepared(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct,
                                   uint32_t n_vars, uint32_t n_public, uint32_t num_constraints,
                                   const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag, int reduction,
                                   g16_setup** out) {
  if (!lag) return G16_ERR_INVALID;
  return setup_impl(device, at, bt, ct, n_vars, n_public, num_constraints, srs, lag, reduction, out);
}

}  // extern "C"

static g16_status setup_impl(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct, uint32_t n_vars,
                             uint32_t n_public, uint32_t num_constraints, const g16_srs_desc* srs,
                             const g16_srs_lagrange_desc* lag, int reduction, g16_setup** out) {
  if (!at || !bt || !ct || !srs || !out) return G16_ERR_INVALID;
  if (reduction != G16_REDUCTION_CIRCOM && reduction != G16_REDUCTION_LIBSNARK) return G16_ERR_INVALID;
  *out = nullptr;
  const uint32_t num_inputs = n_public + 1, N = n_vars;
  int k = 0;
  while (((uint64_t)1 << k) < (uint64_t)num_constraints + num_inputs) ++k;
  if (k + 1 > 28) return G16_ERR_DOMAIN_TOO_LARGE;  // g16_setup_create's limit: n <= 2^27
  const uint32_t n = 1u << k;
  if ((uint64_t)srs->n_tau_g1 < 2 * (uint64_t)n - 1 || srs->n_tau < n) return G16_ERR_INVALID;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  if (lag) {
    if (lag->power > 27) return G16_ERR_DOMAIN_TOO_LARGE;
    if (lag->power < (uint32_t)k) return G16_ERR_INVALID;
    if (!lag->tau_g1 || !lag->tau_g2 || !lag->alpha_tau_g1 || !lag->beta_tau_g1) return G16_ERR_INVALID;
  }
  if (setup_matrices_check(at, bt, ct, N, n_public, num_constraints)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  std::unique_ptr<g16_setup> owned(new g16_setup());  // freed on every way out but the last
  g16_setup* S = owned.get();
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    t_phase.clear();
    PhaseClock clk(t_phase.ms, s);
    S->n_vars = N;
    S->n_public = n_public;
    S->domain = n;
    const uint32_t n1 = 2 * n - 1;
    const size_t maxn = N > n ? N : n;

    // ---- SRS, matrices, twiddle schedules
    DevBuf<G1Affine> tau1, o1, lag1, lagA, lagB;
    DevBuf<G2Affine> o2, lag2;
    DevBuf<G1XYZZ29> w1;
    DevBuf<G2XYZZ29> w2;
    tau1.alloc(n1);
    o1.alloc(maxn);
    o2.alloc(maxn);
    lag1.alloc(n);
    lagA.alloc(n);
    lagB.alloc(n);
    lag2.alloc(n);
    w1.alloc(maxn);
    w2.alloc(maxn);
    const bool need_tau = !lag || reduction == G16_REDUCTION_LIBSNARK;
    if (need_tau) G16_HIP(hipMemcpy(tau1.p, srs->tau_g1, (size_t)n1 * 64, hipMemcpyHostToDevice));
    DevCsr dA, dB, dC;
    dA.upload(at, N);
    dB.upload(bt, N);
    dC.upload(ct, N);
    Twiddles T;
    if (!lag) {
      DevBuf<Fr> tmp;
      tmp.alloc(n);
      build_twiddles(T, k, reduction == G16_REDUCTION_CIRCOM, tmp.p, s);
    }
    clk.lap(T_UPLOAD);

    // ---- Lagrange bases: G1 three times, G2 once; natural order, packed internal affine
    const uint8_t* g1_src[3] = {nullptr, srs->alpha_tau_g1, srs->beta_tau_g1};
    G1Affine* g1_dst[3] = {lag1.p, lagA.p, lagB.p};
    const size_t lvl = (size_t)n - 1;  // level k of a Lagrange array starts at point 2^k - 1
    if (lag) {  // level k as it stands: no transform, only the packed form
      const uint8_t* g1_lag[3] = {lag->tau_g1, lag->alpha_tau_g1, lag->beta_tau_g1};
      for (int q = 0; q < 3; ++q) {
        G16_HIP(hipMemcpy(o1.p, g1_lag[q] + lvl * 64, (size_t)n * 64, hipMemcpyHostToDevice));
        G16_LAUNCH((k_pack_affine<Fq>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G1Affine*)o1.p, n, g1_dst[q]);
      }
      G16_HIP(hipMemcpy(o2.p, lag->tau_g2 + lvl * 128, (size_t)n * 128, hipMemcpyHostToDevice));
      G16_LAUNCH((k_pack_affine<Fq2>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G2Affine*)o2.p, n, lag2.p);
      clk.lap(T_UPLOAD);
    }
    for (int q = 0; q < 3 && !lag; ++q) {
      const G1Affine* in = tau1.p;
      if (g1_src[q]) {
        G16_HIP(hipMemcpy(o1.p, g1_src[q], (size_t)n * 64, hipMemcpyHostToDevice));
        in = o1.p;
      }
      G16_LAUNCH((k_load_affine<Fq>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, in, n, w1.p);
      group_intt<Fq29>(w1.p, k, T, true, s);
      clk.lap(T_NTT_G1);
      to_affine<Fq, true>(w1.p, n, k, g1_dst[q], s);
      clk.lap(T_AFFINE);
    }
    if (!lag) {
      G16_HIP(hipMemcpy(o2.p, srs->tau_g2, (size_t)n * 128, hipMemcpyHostToDevice));
      G16_LAUNCH((k_load_affine<Fq2>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G2Affine*)o2.p, n, w2.p);
      group_intt<Fq2x29>(w2.p, k, T, true, s);
      clk.lap(T_NTT_G2);
      to_affine<Fq2, true>(w2.p, n, k, lag2.p, s);
      clk.lap(T_AFFINE);
    }

    // ---- H
    if (lag && reduction == G16_REDUCTION_CIRCOM) {
      // the odd entries of level k + 1 of tau_g1 AS IT STANDS.  For k == power that level is the transform of
      // tau^0 .. tau^(2n-2) | infinity, the h_query of g16_setup_from_srs; below the power it is the transform of
      // all 2n powers, and the two queries differ point by point by multiples of tau^(2n-1) G -- the same proofs,
      // since the quotient has no coefficient at x^(2n-1) (include/g16_amd.h).
      const uint8_t* top = lag->tau_g1 + (2 * (size_t)n - 1) * 64;
      S->h.resize((size_t)n * 64);
      for (size_t i = 0; i < n; ++i) memcpy(S->h.data() + i * 64, top + (2 * i + 1) * 64, 64);
      clk.lap(T_H);
    } else if (reduction == G16_REDUCTION_CIRCOM) {
      G16_LAUNCH(k_h_first, ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G1Affine*)tau1.p, n, (const Naf*)T.h.p, w1.p);
      group_intt<Fq29>(w1.p, k, T, false, s);
      clk.lap(T_H);
      to_affine<Fq, false>(w1.p, n, k, o1.p, s);
    } else {
      G16_LAUNCH(k_h_first, ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G1Affine*)tau1.p, n, (const Naf*)nullptr, w1.p);
      clk.lap(T_H);
      to_affine<Fq, false>(w1.p, n, -1, o1.p, s);
    }
    if (!(lag && reduction == G16_REDUCTION_CIRCOM)) {
      clk.lap(T_AFFINE);
      fetch(S->h, o1.p, n);
    }
    clk.lap(T_DOWNLOAD);

    // ---- queries
    auto g1_query = [&](const DevCsr* const* mats, const G1Affine* const* bases, uint32_t nm) {
      combine<Fq>(mats, bases, nm, N, w1.p, s);
      clk.lap(T_COMB);
      to_affine<Fq, false>(w1.p, N, -1, o1.p, s);
      clk.lap(T_AFFINE);
    };
    {
      const DevCsr* m[1] = {&dA};
      const G1Affine* b[1] = {lag1.p};
      g1_query(m, b, 1);
      fetch(S->a, o1.p, N);
      clk.lap(T_DOWNLOAD);
    }
    {
      const DevCsr* m[1] = {&dB};
      const G1Affine* b[1] = {lag1.p};
      g1_query(m, b, 1);
      fetch(S->b1, o1.p, N);
      clk.lap(T_DOWNLOAD);
    }
    {
      const DevCsr* m[1] = {&dB};
      const G2Affine* b[1] = {lag2.p};
      combine<Fq2>(m, b, 1, N, w2.p, s);
      clk.lap(T_COMB);
      to_affine<Fq2, false>(w2.p, N, -1, o2.p, s);
      clk.lap(T_AFFINE);
      fetch(S->b2, o2.p, N);
      clk.lap(T_DOWNLOAD);
    }
    {
      const DevCsr* m[3] = {&dA, &dB, &dC};
      const G1Affine* b[3] = {lagB.p, lagA.p, lag1.p};
      g1_query(m, b, 3);
      std::vector<uint8_t> all;
      fetch(all, o1.p, N);
      S->ic.assign(all.begin(), all.begin() + (size_t)num_inputs * 64);
      S->l.assign(all.begin() + (size_t)num_inputs * 64, all.begin() + (size_t)N * 64);
      if (S->l.empty()) S->l.resize(1);
      clk.lap(T_DOWNLOAD);
    }
    // ---- single points: alpha, beta from the SRS; gamma = delta = 1
    const G1Affine g1 = g1_generator();
    const G2Affine g2 = g2_generator();
    memcpy(S->alpha1, srs->alpha_tau_g1, 64);
    memcpy(S->beta1, srs->beta_tau_g1, 64);
    memcpy(S->beta2, srs->beta_g2, 128);
    memcpy(S->delta1, &g1, 64);
    memcpy(S->delta2, &g2, 128);
    memcpy(S->gamma2, &g2, 128);
    *out = owned.release();
    return G16_OK;
  });
}

extern "C" {

g16_status g16_setup_from_srs_times(float* ms, uint32_t cap) {
  return t_phase.read(ms, cap);
}

}  // extern "C"
