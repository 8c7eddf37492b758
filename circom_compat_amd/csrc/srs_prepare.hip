// srs_prepare.hip -- prepared powers of tau (`snarkjs powersoftau prepare phase2`): the Lagrange sections 12-15 of a
// .ptau built (g16_srs_prepare) and checked against the monomial arrays (g16_srs_lagrange_check).  The layout of a
// Lagrange set, the algebra of the check and its soundness are in include/g16_amd.h; g16_setup_from_prepared, which
// USES a set, is setup_srs.hip's body with the transforms skipped.
//
// g16_srs_prepare: level by level (p = 0 .. P+1), the twiddle schedules of size 2^p once, then the group transform
// of gtransform.h on the first 2^p points of each array, the affine pass with the bit reversal folded in, and the
// download of the level.  Nothing but one level is resident.
//
// g16_srs_lagrange_check, per array (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1):
//   k_lc_rho_fr + ntt29_dif + k_lc_accum   C = sum_p iNTT_{2^p}(rho^(p)): the level's 128-bit coefficients as Fr,
//                                the inverse Fr transform of the witness map (ntt29.h, 1/2^p fused), and the
//                                bit-reversed result added into C[0 .. 2^p)
//   k_lc_flags_g1 / _g2          one reason byte per point: the predicates of keycheck.h (monomial G2 points: canonical
//                                and on the curve only -- the string is expected to have passed g16_srs_check)
//   k_lc_rho                     Lagrange side: one lane per point, rho P by a 128-step double-and-add of mixed
//                                additions on the lazy limbs of ec29.h, then the block's sum (kc_block_sum)
//   k_lc_coeff                   monomial side: one lane per point, C_i P by a NAF ladder over the full width
//   k_lc_fold                    one block: the chunk's block sums into the running sum of the side
//   k_lc_collect                 one block: counts the flags, appends the bad points in index order (a scan)
// and once at the end k_lc_final: the two sums of every array compared as group elements (their difference is the
// point at infinity), the report and the bad-point list assembled on the device.  The arrays are STREAMED as in
// srs_check.hip: two page-locked host slots and two device slots of `chunk` points, the copy of chunk k + 1 under
// the kernels of chunk k.  One synchronisation precedes the download of the report.  No atomics anywhere.
#include <stdlib.h>

#include <memory>

#include "gtransform.h"
#include "keycheck.h"
#include "ntt29.h"

namespace g16 {
namespace {

constexpr uint32_t LC_DEFAULT_CHUNK = 1u << 18;
constexpr uint32_t LC_N = G16_LAGRANGE_N_ARRAYS;

thread_local float t_prepare_ms[7];  // the phases of g16_setup_from_srs_times

struct LcState {  // device-resident for the whole call
  uint64_t n_points[LC_N], n_bad[LC_N], n_infinity[LC_N];
  uint32_t n_list[LC_N];
  G1XYZZ29 sum1[3][2];  // [tau_g1, alpha_tau_g1, beta_tau_g1][Lagrange side, monomial side]
  G2XYZZ29 sum2[2];
  g16_srs_lagrange_report report;
};

__global__ void __launch_bounds__(KC_BLOCK) k_lc_flags_g1(const G1Affine* pts, uint32_t n, uint8_t* flags) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  flags[i] = g1_flag(pts[i]);
}

// subgroup = 0 (monomial points): canonical words and the curve equation only
__global__ void __launch_bounds__(KC_BLOCK) k_lc_flags_g2(const VkDev* vk, const G2Affine* pts, uint32_t n,
                                                          uint32_t subgroup, uint8_t* flags) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G2Affine p = pts[i];
  uint8_t f;
  if (subgroup) {
    f = g2_flag(p, vk);
  } else if (!(fq2_words_canonical(p.x) && fq2_words_canonical(p.y))) {
    f = G16_KEY_BAD_NONCANONICAL;
  } else if (p.is_inf()) {
    f = KC_INF;
  } else {
    f = on_curve_g2(p, vk) ? 0 : G16_KEY_BAD_OFF_CURVE;
  }
  flags[i] = f;
}

// part[block] = sum over the block of rho_i P_i, rho_i = rho[2i] + 2^64 rho[2i + 1].  A malformed or infinite
// point is left out (the relations are not reported when a point is malformed).
template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_lc_rho(const Affine<F>* pts, const uint64_t* rho, const uint8_t* flags,
                                                     uint32_t n, XYZZ29<typename Lazy<F>::type>* part) {
  using P = XYZZ29<typename Lazy<F>::type>;
  __shared__ P sh[KC_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  P acc = P::infinity();
  if (i < n && !flags[i]) {
    const uint64_t lo = rho[2 * (size_t)i], hi = rho[2 * (size_t)i + 1];
    const Aff29<typename Lazy<F>::type> p = affine_from_mont256<F>(pts[i]);
#pragma unroll 1
    for (int b = 127; b >= 0; --b) {
      acc.dbl_in_place();
      const uint64_t w = b >= 64 ? hi : lo;
      if ((w >> (b & 63)) & 1) acc.madd(p);
    }
  }
  kc_block_sum(sh, acc);
  if (t == 0) part[blockIdx.x] = sh[0];
}

// part[block] = sum over the block of coeff[i] P_i, coeff full-width Montgomery Fr: the NAF ladder of comb_term
// (setup_srs.hip), mixed additions of +-P from the top word down
template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_lc_coeff(const Affine<F>* pts, const Fr* coeff, const uint8_t* flags,
                                                       uint32_t n, XYZZ29<typename Lazy<F>::type>* part) {
  using LF = typename Lazy<F>::type;
  using P = XYZZ29<LF>;
  __shared__ P sh[KC_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  P acc = P::infinity();
  if (i < n && !flags[i]) {
    const Aff29<LF> p = affine_from_mont256<F>(pts[i]);
    const Naf s = naf_of(coeff[i].to_canonical());
    const LF ny = p.y.neg().carry();
#pragma unroll 1
    for (int w = 7; w >= 0; --w) {
      const uint32_t pw = s.pos[w], nw = s.neg[w];
      if (!(pw | nw) && acc.is_inf()) continue;
#pragma unroll 1
      for (int b = 31; b >= 0; --b) {
        acc.dbl_in_place();
        const uint32_t m = 1u << b;
        if ((pw | nw) & m) acc.madd(Aff29<LF>{p.x, (nw & m) ? ny : p.y, false});
      }
    }
  }
  kc_block_sum(sh, acc);
  if (t == 0) part[blockIdx.x] = sh[0];
}

// one block: *sum += the chunk's nb block sums
template <class LF>
__global__ void __launch_bounds__(KC_BLOCK) k_lc_fold(const XYZZ29<LF>* part, uint32_t nb, XYZZ29<LF>* sum) {
  __shared__ XYZZ29<LF> sh[KC_BLOCK];
  const uint32_t t = threadIdx.x;
  XYZZ29<LF> a = XYZZ29<LF>::infinity();
#pragma unroll 1
  for (uint32_t k = t; k < nb; k += KC_BLOCK) a.add(part[k]);
  kc_block_sum(sh, a);
  if (t == 0) {
    XYZZ29<LF> s = *sum;
    s.add(sh[0]);
    *sum = s;
  }
}

// k_sc_collect of srs_check.hip on this call's state
__global__ void __launch_bounds__(KC_SCAN) k_lc_collect(const uint8_t* flags, uint32_t n, uint32_t query, uint32_t base,
                                                        LcState* st, g16_key_bad_point* lists, uint32_t cap) {
  __shared__ uint32_t sh_bad[KC_SCAN], sh_inf[KC_SCAN];
  __shared__ uint32_t sh_start;
  const uint32_t t = threadIdx.x;
  const uint32_t seg = (n + KC_SCAN - 1) / KC_SCAN;
  const uint32_t lo = t * seg < n ? t * seg : n, hi = lo + seg < n ? lo + seg : n;
  uint32_t bad = 0, inf = 0;
#pragma unroll 1
  for (uint32_t i = lo; i < hi; ++i) {
    const uint8_t f = flags[i];
    bad += (f & ~KC_INF) ? 1 : 0;
    inf += (f == KC_INF) ? 1 : 0;
  }
  sh_bad[t] = bad;
  sh_inf[t] = inf;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0, infs = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < KC_SCAN; ++k) {
      const uint32_t c = sh_bad[k];
      sh_bad[k] = run;
      run += c;
      infs += sh_inf[k];
    }
    const uint32_t start = st->n_list[query];
    sh_start = start;
    st->n_bad[query] += run;
    st->n_infinity[query] += infs;
    st->n_list[query] = (uint64_t)start + run < cap ? start + run : cap;
  }
  __syncthreads();
  uint64_t at = (uint64_t)sh_start + sh_bad[t];
  g16_key_bad_point* list = lists + (size_t)query * cap;
#pragma unroll 1
  for (uint32_t i = lo; i < hi && bad && at < cap; ++i) {
    const uint8_t f = flags[i] & ~KC_INF;
    if (!f) continue;
    list[at].query = query;
    list[at].index = base + i;
    list[at].reason = f;
    ++at;
  }
}

// rho (2 x u64, a plain integer < 2^128) -> Montgomery Fr
__global__ void __launch_bounds__(256) k_lc_rho_fr(const uint64_t* rho, uint32_t n, Fr* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = Fr::from_canonical(rho_u256(rho, i));
}

// c[bitrev_k(i)] += v[i]: the transform's output is bit-reversed; one lane per entry, every entry touched once
__global__ void __launch_bounds__(256) k_lc_accum(const Fr* v, uint32_t n, int k, Fr* c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = k > 0 ? __brev(i) >> (32 - k) : i;
  c[d] = c[d] + v[i];
}

// the sums of each array compared (their difference is the point at infinity), then the report and the list
__global__ void __launch_bounds__(KC_BLOCK) k_lc_final(LcState* st, const g16_key_bad_point* lists, uint32_t cap,
                                                       g16_key_bad_point* out_list) {
  __shared__ uint32_t sh_off[LC_N + 1];
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    uint64_t bad = 0;
    uint32_t off = 0;
    for (uint32_t q = 0; q < LC_N; ++q) {
      bad += st->n_bad[q];
      sh_off[q] = off;
      const uint32_t room = cap - off;
      off += st->n_list[q] < room ? st->n_list[q] : room;
    }
    sh_off[LC_N] = off;
    g16_srs_lagrange_report r;
    memset(&r, 0, sizeof r);
    r.relations_checked = bad ? 0 : 1;
    if (!bad) {
      for (uint32_t a = 0; a < 3; ++a) {
        G1XYZZ29 d = st->sum1[a][0];
        d.add(st->sum1[a][1].neg());
        const uint32_t q = a == 0 ? G16_SRS_Q_TAU_G1 : a == 1 ? G16_SRS_Q_ALPHA_TAU_G1 : G16_SRS_Q_BETA_TAU_G1;
        if (!d.is_inf()) r.relations_failed |= 1u << q;
      }
      G2XYZZ29 d2 = st->sum2[0];
      d2.add(st->sum2[1].neg());
      if (!d2.is_inf()) r.relations_failed |= 1u << G16_SRS_Q_TAU_G2;
    }
    r.ok = (!bad && !r.relations_failed) ? 1 : 0;
    for (uint32_t q = 0; q < LC_N; ++q) {
      r.n_points[q] = st->n_points[q];
      r.n_bad[q] = st->n_bad[q];
      r.n_infinity[q] = st->n_infinity[q];
    }
    r.n_listed = off;
    st->report = r;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t q = 0; q < LC_N; ++q) {
    const uint32_t cnt = sh_off[q + 1] - sh_off[q];
#pragma unroll 1
    for (uint32_t k = t; k < cnt; k += KC_BLOCK) out_list[sh_off[q] + k] = lists[(size_t)q * cap + k];
  }
}

struct LcArray {
  bool g2;
  uint32_t query, which;  // which: index into LcState::sum1
  int top;                // highest level
  const uint8_t* lag;     // the Lagrange section: 2^(top+1) - 1 points
  const uint8_t* mono;    // the monomial array
  uint64_t n_mono;        // monomial points that enter (the pad of tau_g1's top level does not)
};

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" {

g16_status g16_srs_prepare(int device, const g16_srs_desc* srs, uint32_t power, uint8_t* tau_g1_out,
                           uint8_t* tau_g2_out, uint8_t* alpha_tau_g1_out, uint8_t* beta_tau_g1_out) {
  if (!srs || !tau_g1_out || !tau_g2_out || !alpha_tau_g1_out || !beta_tau_g1_out) return G16_ERR_INVALID;
  if (power > 27) return G16_ERR_DOMAIN_TOO_LARGE;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  const uint32_t nP = 1u << power, n_top = 2 * nP;
  if ((uint64_t)srs->n_tau_g1 < (uint64_t)n_top - 1 || srs->n_tau < nP) return G16_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G16_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return G16_ERR_INVALID;
  try {
    G16_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    memset(t_prepare_ms, 0, sizeof t_prepare_ms);
    PhaseClock clk(t_prepare_ms, s);
    DevBuf<G1Affine> in1, o1;
    DevBuf<G2Affine> in2, o2;
    DevBuf<G1XYZZ29> w1;
    DevBuf<G2XYZZ29> w2;
    DevBuf<Fr> tmp;
    in1.alloc(n_top);
    o1.alloc(n_top);
    w1.alloc(n_top);
    in2.alloc(nP);
    o2.alloc(nP);
    w2.alloc(nP);
    tmp.alloc(nP);  // n / 2 scalars of the largest level
    const uint8_t* g1_src[3] = {srs->tau_g1, srs->alpha_tau_g1, srs->beta_tau_g1};
    uint8_t* g1_dst[3] = {tau_g1_out, alpha_tau_g1_out, beta_tau_g1_out};
    for (uint32_t p = 0; p <= power + 1; ++p) {
      const uint32_t n = 1u << p;
      const size_t at = (size_t)n - 1;  // the level's offset in points
      Twiddles T;
      build_twiddles(T, (int)p, false, tmp.p, s);
      clk.lap(0);
      for (int q = 0; q < 3; ++q) {
        if (q && p > power) break;  // only tau_g1 has level P+1
        const uint32_t have = p > power ? n - 1 : n;  // level P+1 reads M[2^(P+1) - 1] as infinity
        G16_HIP(hipMemcpyAsync(in1.p, g1_src[q], (size_t)have * 64, hipMemcpyHostToDevice, s));
        if (have < n) G16_HIP(hipMemsetAsync(in1.p + have, 0, 64, s));
        G16_LAUNCH((k_load_affine<Fq>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G1Affine*)in1.p, n, w1.p);
        clk.lap(0);
        group_intt<Fq29>(w1.p, (int)p, T, true, s);
        clk.lap(1);
        to_affine<Fq, false>(w1.p, n, (int)p, o1.p, s);
        clk.lap(4);
        G16_HIP(hipMemcpy(g1_dst[q] + at * 64, o1.p, (size_t)n * 64, hipMemcpyDeviceToHost));
        clk.lap(6);
      }
      if (p <= power) {
        G16_HIP(hipMemcpyAsync(in2.p, srs->tau_g2, (size_t)n * 128, hipMemcpyHostToDevice, s));
        G16_LAUNCH((k_load_affine<Fq2>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G2Affine*)in2.p, n, w2.p);
        clk.lap(0);
        group_intt<Fq2x29>(w2.p, (int)p, T, true, s);
        clk.lap(2);
        to_affine<Fq2, false>(w2.p, n, (int)p, o2.p, s);
        clk.lap(4);
        G16_HIP(hipMemcpy(tau_g2_out + at * 128, o2.p, (size_t)n * 128, hipMemcpyDeviceToHost));
        clk.lap(6);
      }
    }
    return G16_OK;
  } catch (const HipError&) {
    return G16_ERR_HIP;
  } catch (const std::exception&) {
    return G16_ERR_INTERNAL;
  }
}

g16_status g16_srs_prepare_times(float* ms, uint32_t cap) {
  if (!ms) return G16_ERR_INVALID;
  for (uint32_t i = 0; i < cap; ++i) ms[i] = i < 7 ? t_prepare_ms[i] : 0.f;
  return G16_OK;
}

g16_status g16_srs_lagrange_check(int device, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                  const uint64_t* rho, g16_key_bad_point* bad_out, uint32_t bad_cap,
                                  g16_srs_lagrange_report* report) {
  if (!srs || !lag || !report || (bad_cap && !bad_out)) return G16_ERR_INVALID;
  if (lag->power > 27) return G16_ERR_DOMAIN_TOO_LARGE;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  if (!lag->tau_g1 || !lag->tau_g2 || !lag->alpha_tau_g1 || !lag->beta_tau_g1) return G16_ERR_INVALID;
  const uint32_t P = lag->power;
  const uint64_t nP = (uint64_t)1 << P, n_top = 2 * nP;
  if ((uint64_t)srs->n_tau_g1 < n_top - 1 || srs->n_tau < nP) return G16_ERR_INVALID;
  const uint64_t m1 = 2 * n_top - 1, m2 = n_top - 1;  // points of section 12 / of sections 13-15
  const uint64_t n_rho = m1 + 3 * m2;
  if (rho)
    for (uint64_t i = 0; i < n_rho; ++i)
      if (!(rho[2 * i] | rho[2 * i + 1])) return G16_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G16_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return G16_ERR_INVALID;
  try {
    // G16_LAGCHECK_CHUNK=<points> (tests): points per staged chunk; never more than the longest array needs
    uint32_t chunk = LC_DEFAULT_CHUNK;
    if (const char* e = getenv("G16_LAGCHECK_CHUNK")) {
      const unsigned long long v = strtoull(e, nullptr, 0);
      if (v >= 1 && v <= (1ull << 24)) chunk = (uint32_t)v;
    }
    if (chunk > m1) chunk = (uint32_t)m1;
    const uint32_t nb_max = ceil_div(chunk, KC_BLOCK);
    const uint32_t cap = bad_cap < KC_MAX_LISTED ? bad_cap : KC_MAX_LISTED;

    const LcArray arrays[LC_N] = {
        {false, G16_SRS_Q_TAU_G1, 0, (int)P + 1, lag->tau_g1, srs->tau_g1, n_top - 1},
        {true, G16_SRS_Q_TAU_G2, 0, (int)P, lag->tau_g2, srs->tau_g2, nP},
        {false, G16_SRS_Q_ALPHA_TAU_G1, 1, (int)P, lag->alpha_tau_g1, srs->alpha_tau_g1, nP},
        {false, G16_SRS_Q_BETA_TAU_G1, 2, (int)P, lag->beta_tau_g1, srs->beta_tau_g1, nP}};

    G16_HIP(hipSetDevice(device));
    const HostConsts& H = host_consts();
    std::unique_ptr<VkDev> hv(new VkDev());
    memset(hv.get(), 0, sizeof(VkDev));
    hv->frob_x = H.frob_x;
    hv->frob_y = H.frob_y;
    hv->b_twist = H.b_twist;
    memcpy(hv->frob, H.frob, sizeof H.frob);
    std::unique_ptr<LcState> hs(new LcState());
    memset(hs.get(), 0, sizeof(LcState));
    hs->n_points[G16_SRS_Q_TAU_G1] = m1;
    hs->n_points[G16_SRS_Q_TAU_G2] = hs->n_points[G16_SRS_Q_ALPHA_TAU_G1] = hs->n_points[G16_SRS_Q_BETA_TAU_G1] = m2;

    // every allocation of the call but the transform plans: nothing else is allocated inside the loops
    const size_t off_rho = (size_t)chunk * 128;  // a slot: points | chunk coefficients
    const size_t slot_bytes = off_rho + (size_t)chunk * 16;
    PinnedBuf pin[2];
    DevBuf<uint8_t> dslot[2], dflags;
    DevBuf<VkDev> dvk;
    DevBuf<LcState> dst;
    DevBuf<G1XYZZ29> dpart1;
    DevBuf<G2XYZZ29> dpart2;
    DevBuf<g16_key_bad_point> dlists, dout;
    DevBuf<Fr> dC, dv;
    DevBuf<uint64_t> drho_lvl;
    DevBuf<int32_t> dplanes;
    StreamBox copy, comp;
    EventBox copied[2], done[2];
    for (int s = 0; s < 2; ++s) {
      pin[s].alloc(slot_bytes);
      dslot[s].alloc(slot_bytes);
      copied[s].create();
      done[s].create();
    }
    dflags.alloc(chunk);
    dvk.alloc(1);
    dst.alloc(1);
    dpart1.alloc(nb_max);
    dpart2.alloc(nb_max);
    dlists.alloc((size_t)LC_N * (cap ? cap : 1));
    dout.alloc(cap ? cap : 1);
    dC.alloc(n_top);
    dv.alloc(n_top);
    drho_lvl.alloc(2 * n_top);
    dplanes.alloc((size_t)NTT29_LIMBS * n_top);
    copy.create();
    comp.create();
    G16_HIP(hipMemcpy(dvk.p, hv.get(), sizeof(VkDev), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dst.p, hs.get(), sizeof(LcState), hipMemcpyHostToDevice));

    std::vector<uint64_t> drawn;  // the array's rho when the caller gave none
    const uint64_t* rho_at = rho;
    size_t k = 0;                 // chunks staged so far: the slot is k & 1
    for (uint32_t a = 0; a < LC_N; ++a) {
      const LcArray& A = arrays[a];
      const uint64_t m = ((uint64_t)2 << A.top) - 1;
      const uint64_t* r = rho_at;
      if (!rho) {
        // the slots in flight do not read `drawn`, but the level uploads below do: they are synchronous
        drawn.resize(2 * m);
        bool ok = os_random(drawn.data(), (size_t)m * 16);
        for (uint64_t i = 0; ok && i < m; ++i)
          while (ok && !(drawn[2 * i] | drawn[2 * i + 1])) ok = os_random(&drawn[2 * i], 16);  // probability 2^-128
        if (!ok) {  // never a fixed fallback; the chunks in flight still read the slots
          (void)hipStreamSynchronize(copy.s);
          (void)hipStreamSynchronize(comp.s);
          return G16_ERR_INTERNAL;
        }
        r = drawn.data();
      } else {
        rho_at += 2 * m;
      }

      // ---- C = sum_p iNTT_{2^p}(rho^(p)), on the compute stream behind the array before
      G16_HIP(hipMemsetAsync(dC.p, 0, ((size_t)1 << A.top) * sizeof(Fr), comp.s));
      for (int p = 0; p <= A.top; ++p) {
        const uint32_t n = 1u << p;
        Ntt29Plan plan;
        plan.build(p, comp.s);
        G16_HIP(hipMemcpyAsync(drho_lvl.p, r + 2 * ((size_t)n - 1), (size_t)n * 16, hipMemcpyHostToDevice, comp.s));
        G16_LAUNCH(k_lc_rho_fr, ceil_div(n, 256), 256, 0, comp.s, (const uint64_t*)drho_lvl.p, n, dv.p);
        ntt29_to_planes(dv.p, dplanes.p, n, comp.s);
        ntt29_dif(plan, dplanes.p, (size_t)NTT29_LIMBS * n, 1, true, NTT_FUSE_SCALE, comp.s);
        ntt29_from_planes(dplanes.p, dv.p, n, comp.s);
        G16_LAUNCH(k_lc_accum, ceil_div(n, 256), 256, 0, comp.s, (const Fr*)dv.p, n, p, dC.p);
        G16_HIP(hipStreamSynchronize(comp.s));  // the plan's tables are released at the end of this scope
      }

      // ---- the two sides: the Lagrange section under rho, then the monomial array under C
      for (int side = 0; side < 2; ++side) {
        const uint64_t total = side ? A.n_mono : m;
        const uint8_t* src = side ? A.mono : A.lag;
        const size_t w = A.g2 ? 128 : 64;
        for (uint64_t base = 0; base < total; base += chunk, ++k) {
          const uint32_t n = (uint32_t)(total - base < chunk ? total - base : chunk);
          const int s = (int)(k & 1);
          if (k >= 2) G16_HIP(hipEventSynchronize(done[s].e));  // the kernels that read this slot two chunks ago
          uint8_t* h = pin[s].p;
          uint8_t* d = dslot[s].p;
          memcpy(h, src + base * w, (size_t)n * w);
          G16_HIP(hipMemcpyAsync(d, h, (size_t)n * w, hipMemcpyHostToDevice, copy.s));
          if (!side) {
            memcpy(h + off_rho, r + 2 * base, (size_t)n * 16);
            G16_HIP(hipMemcpyAsync(d + off_rho, h + off_rho, (size_t)n * 16, hipMemcpyHostToDevice, copy.s));
          }
          G16_HIP(hipEventRecord(copied[s].e, copy.s));
          G16_HIP(hipStreamWaitEvent(comp.s, copied[s].e, 0));
          const uint32_t nb = ceil_div(n, KC_BLOCK);
          const uint64_t* drho = (const uint64_t*)(d + off_rho);
          const uint8_t* fl = dflags.p;
          if (A.g2) {
            G16_LAUNCH(k_lc_flags_g2, nb, KC_BLOCK, 0, comp.s, (const VkDev*)dvk.p, (const G2Affine*)d, n,
                       (uint32_t)(side ? 0 : 1), dflags.p);
            if (side)
              G16_LAUNCH((k_lc_coeff<Fq2>), nb, KC_BLOCK, 0, comp.s, (const G2Affine*)d, (const Fr*)(dC.p + base), fl,
                         n, dpart2.p);
            else
              G16_LAUNCH((k_lc_rho<Fq2>), nb, KC_BLOCK, 0, comp.s, (const G2Affine*)d, drho, fl, n, dpart2.p);
            G16_LAUNCH((k_lc_fold<Fq2x29>), 1, KC_BLOCK, 0, comp.s, (const G2XYZZ29*)dpart2.p, nb,
                       &dst.p->sum2[side]);
          } else {
            G16_LAUNCH(k_lc_flags_g1, nb, KC_BLOCK, 0, comp.s, (const G1Affine*)d, n, dflags.p);
            if (side)
              G16_LAUNCH((k_lc_coeff<Fq>), nb, KC_BLOCK, 0, comp.s, (const G1Affine*)d, (const Fr*)(dC.p + base), fl,
                         n, dpart1.p);
            else
              G16_LAUNCH((k_lc_rho<Fq>), nb, KC_BLOCK, 0, comp.s, (const G1Affine*)d, drho, fl, n, dpart1.p);
            G16_LAUNCH((k_lc_fold<Fq29>), 1, KC_BLOCK, 0, comp.s, (const G1XYZZ29*)dpart1.p, nb,
                       &dst.p->sum1[A.which][side]);
          }
          if (!side)  // only the Lagrange points are counted and listed
            G16_LAUNCH(k_lc_collect, 1, KC_SCAN, 0, comp.s, fl, n, A.query, (uint32_t)base, dst.p, dlists.p, cap);
          G16_HIP(hipEventRecord(done[s].e, comp.s));
        }
      }
      // `drawn` is overwritten for the next array: every copy out of it (pinned slots, level uploads) is done
    }
    G16_LAUNCH(k_lc_final, 1, KC_BLOCK, 0, comp.s, dst.p, (const g16_key_bad_point*)dlists.p, cap, dout.p);
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(comp.s));  // the one synchronisation before the download
    G16_HIP(hipMemcpy(hs.get(), dst.p, sizeof(LcState), hipMemcpyDeviceToHost));
    *report = hs->report;
    if (report->n_listed)
      G16_HIP(hipMemcpy(bad_out, dout.p, (size_t)report->n_listed * sizeof(g16_key_bad_point), hipMemcpyDeviceToHost));
    return G16_OK;
  } catch (const HipError&) {
    return G16_ERR_HIP;
  } catch (const std::exception&) {
    return G16_ERR_INTERNAL;
  }
}

}  // extern "C"
