// srs_check.hip -- validation of a powers-of-tau string on the GPU before keys are built from it
// (g16_srs_check): the point arithmetic of `snarkjs powersoftau verify`.  The section-7 contribution transcript
// is NOT handled (include/g16_amd.h).
//
// keycheck.hip's structure on the five arrays of a g16_srs_desc:
//   structural   every entry handed over, one lane per point: canonical words, on the curve, a G2 point in the
//                r-torsion of the twist -- the predicates and the flag byte of keycheck.h.
//   relations    every array is a geometric sequence in the ONE ratio tau that tau_g2[1] (tau_g1[1]) holds:
//                with 128-bit coefficients rho_i and, for an array P of m points,
//                    Lo(P) = sum_{i<m-1} rho_i P[i]      Hi(P) = sum_{i<m-1} rho_i P[i+1]
//                e(Hi(P), g2) = e(Lo(P), tau_g2[1]) for the three G1 arrays and e(tau_g1[1], Lo(P)) = e(g1, Hi(P))
//                for tau_g2; the two bases and beta_g2 are tied by three single pairings.
//
// The arrays are STREAMED through the CheckStage of keycheck.h: two page-locked host slots and two device slots of
// `chunk` points, the copy of chunk k + 1 under the kernels of chunk k.  Per chunk:
//   k_chk_flags_g1 / _g2         one reason byte per point
//   k_sc_pair_g1 / k_sc_pair_g2  the shifted sums.  Point P[j] enters Lo with rho_j and Hi with rho_{j-1}: one
//                                lane per point, the point fetched ONCE, both products from one LSB-first chain
//                                (the running double 2^b P is added into either accumulator: 128 doublings and
//                                ~128 full additions, against 2 x (128 doublings + ~64 mixed additions) for two
//                                MSB-first ladders), then two per-block sums through the LDS tree of
//                                kc_block_sum.  The slot carries chunk + 1 coefficients: entry k is
//                                rho_{base - 1 + k}, so a chunk seam needs nothing but the overlap of one
//                                coefficient, and the zero entries in front of the first and behind the last point
//                                of an array keep those two points out of Hi / Lo.
//   k_chk_fold                   one block: the chunk's block sums into the running sums of the call
//   k_chk_collect                one block: counts the flags and appends the bad points in index order (a scan)
// and once at the end
//   k_sc_final                   twelve Miller loops in twelve lanes, six final exponentiations in six, then the
//                                report and the bad-point list assembled on the device.
// One synchronisation precedes the download of the report and the list.  No atomics anywhere.
#include "keycheck.h"

namespace g16 {
namespace {

constexpr uint32_t SC_DEFAULT_CHUNK = 1u << 18;
constexpr uint32_t SC_N_G1 = 3;  // the G1 arrays: tau_g1, alpha_tau_g1, beta_tau_g1

struct ScKey {  // the fixed points of the six pairs
  G1Affine tau1, beta1, g1_neg;  // tau_g1[1], beta_tau_g1[0], -G1
  G2Affine tau2, beta2, g2;      // tau_g2[1], beta_g2, G2
};

struct ScState {  // device-resident for the whole call
  CheckTally tally;
  G1XYZZ sum1[SC_N_G1][2];  // [tau_g1, alpha_tau_g1, beta_tau_g1][Lo, Hi] so far
  G2XYZZ sum2[2];           // tau_g2: Lo, Hi so far
  g16_srs_report report;
};

// part[block] = sum over the block of rho[i + 1] P_i (the chunk's share of Lo), part[nb + block] = the same with
// rho[i] (of Hi); rho has n + 1 entries of 2 x u64, a zero entry contributes nothing.  D runs through P, 2P, 4P,
// ...: bit b of either coefficient adds 2^b P into that coefficient's accumulator.  The loop ends with the highest
// set bit of the two coefficients.  A malformed point is left out: the relations are not reported then anyway.
template <class F>
__device__ __forceinline__ void sc_pair(const Affine<F>* pts, const uint64_t* rho, const uint8_t* flags, uint32_t n,
                                        XYZZ<F>* part, XYZZ<F>* sh) {
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  XYZZ<F> lo = XYZZ<F>::infinity(), hi = XYZZ<F>::infinity();
  if (i < n && !flags[i]) {  // neither malformed nor infinity
    uint64_t h0 = rho[2 * (size_t)i], h1 = rho[2 * (size_t)i + 1];
    uint64_t l0 = rho[2 * (size_t)i + 2], l1 = rho[2 * (size_t)i + 3];
    XYZZ<F> D = XYZZ<F>::from_affine(pts[i]);
#pragma unroll 1
    while (h0 | h1 | l0 | l1) {
      if (l0 & 1) lo.add(D);
      if (h0 & 1) hi.add(D);
      l0 = (l0 >> 1) | (l1 << 63);
      l1 >>= 1;
      h0 = (h0 >> 1) | (h1 << 63);
      h1 >>= 1;
      D.dbl_in_place();
    }
  }
  kc_block_sum(sh, lo);
  if (t == 0) part[blockIdx.x] = sh[0];
  __syncthreads();
  kc_block_sum(sh, hi);
  if (t == 0) part[gridDim.x + blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(KC_BLOCK) k_sc_pair_g1(const G1Affine* pts, const uint64_t* rho, const uint8_t* flags,
                                                         uint32_t n, G1XYZZ* part) {
  __shared__ G1XYZZ sh[KC_BLOCK];
  sc_pair<Fq>(pts, rho, flags, n, part, sh);
}

__global__ void __launch_bounds__(KC_BLOCK) k_sc_pair_g2(const G2Affine* pts, const uint64_t* rho, const uint8_t* flags,
                                                         uint32_t n, G2XYZZ* part) {
  __shared__ G2XYZZ sh[KC_BLOCK];
  sc_pair<Fq2>(pts, rho, flags, n, part, sh);
}

// The same two sums the way k_kc_rho would make them (G16_SRSCHECK_SLICED=1, the yardstick of the fused chain):
// blockIdx.y = 0 is Lo, 1 is Hi, each one MSB-first ladder of mul_rho -- every point fetched twice, every
// doubling chain run twice, two live values instead of three.
template <class F>
__device__ __forceinline__ void sc_pair_sliced(const Affine<F>* pts, const uint64_t* rho, const uint8_t* flags,
                                               uint32_t n, XYZZ<F>* part, XYZZ<F>* sh) {
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  XYZZ<F> acc = XYZZ<F>::infinity();
  if (i < n && !flags[i]) {
    const size_t e = (size_t)i + (blockIdx.y ? 0 : 1);
    const uint64_t c0 = rho[2 * e], c1 = rho[2 * e + 1];
    if (c0 | c1) acc = mul_rho(pts[i], c0, c1);
  }
  kc_block_sum(sh, acc);
  if (t == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(KC_BLOCK) k_sc_pair_g1_sliced(const G1Affine* pts, const uint64_t* rho,
                                                                const uint8_t* flags, uint32_t n, G1XYZZ* part) {
  __shared__ G1XYZZ sh[KC_BLOCK];
  sc_pair_sliced<Fq>(pts, rho, flags, n, part, sh);
}

__global__ void __launch_bounds__(KC_BLOCK) k_sc_pair_g2_sliced(const G2Affine* pts, const uint64_t* rho,
                                                                const uint8_t* flags, uint32_t n, G2XYZZ* part) {
  __shared__ G2XYZZ sh[KC_BLOCK];
  sc_pair_sliced<Fq2>(pts, rho, flags, n, part, sh);
}

// lanes 2k, 2k + 1: the two Miller loops of pair k; lanes 0..5: product and final exponentiation of pair k
//   0 PAIR_TAU      ML(g2, tau_g1[1])        ML(tau_g2[1], -g1)
//   1 PAIR_TAU_G1   ML(g2, Hi(tau_g1))       ML(tau_g2[1], -Lo(tau_g1))
//   2 PAIR_TAU_G2   ML(Lo(tau_g2), tau_g1[1]) ML(Hi(tau_g2), -g1)
//   3 PAIR_ALPHA    ML(g2, Hi(alpha))        ML(tau_g2[1], -Lo(alpha))
//   4 PAIR_BETA     the same for beta_tau_g1
//   5 PAIR_BETA_G2  ML(g2, beta_tau_g1[0])   ML(beta_g2, -g1)
// then the report and the list.  Nothing is paired when a structural check failed.
__global__ void __launch_bounds__(KC_BLOCK) k_sc_final(const VkDev* vk, const ScKey* key, ScState* st,
                                                       const g16_key_bad_point* lists, uint32_t cap, uint32_t host_bits,
                                                       g16_key_bad_point* out_list) {
  __shared__ F12 sh[12];
  __shared__ uint32_t sh_fail[6];
  __shared__ uint32_t sh_off[G16_SRS_N_QUERIES + 2];
  const uint32_t t = threadIdx.x;
  const bool pair = !chk_offsets(&st->tally, G16_SRS_N_QUERIES, cap, sh_off);
  G2Affine Q = G2Affine::infinity();
  G1Affine P = G1Affine::infinity();
  if (pair && t < 12) {
    const uint32_t k = t >> 1, second = t & 1;
    if (k == 0) {
      Q = second ? key->tau2 : key->g2;
      P = second ? key->g1_neg : key->tau1;
    } else if (k == 2) {
      Q = st->sum2[second].to_affine();
      P = second ? key->g1_neg : key->tau1;
    } else if (k == 5) {
      Q = second ? key->beta2 : key->g2;
      P = second ? key->g1_neg : key->beta1;
    } else {  // 1, 3, 4: the G1 arrays 0, 1, 2
      const uint32_t a = k == 1 ? 0 : k - 2;
      Q = second ? key->tau2 : key->g2;
      P = st->sum1[a][second ? 0 : 1].to_affine();
      if (second) P = P.neg();
    }
  }
  const uint32_t failed = chk_pairs(Q, P, 6, pair, vk, sh, sh_fail);
  if (t == 0) {
    g16_srs_report r;
    memset(&r, 0, sizeof r);
    r.relations_checked = pair ? 1 : 0;
    // pairs 0 .. 5: G16_SRS_PAIR_TAU, _TAU_G1, _TAU_G2, _ALPHA, _BETA, _BETA_G2
    if (pair) r.relations_failed = host_bits | failed * G16_SRS_PAIR_TAU;
    r.ok = (pair && !r.relations_failed) ? 1 : 0;
    chk_counts(&r, &st->tally, G16_SRS_N_QUERIES);
    r.n_listed = sh_off[G16_SRS_N_QUERIES];
    st->report = r;
  }
  chk_emit_lists(sh_off, G16_SRS_N_QUERIES, lists, cap, out_list);
}

// ---- host side -------------------------------------------------------------------------------------

struct Item {
  bool g2, sums;         // sums: the array has a rho segment (everything but beta_g2)
  uint32_t query, which; // which: index into ScState::sum1 (G1 arrays)
  uint32_t base, count;  // points [base, base + count) of an array of `total`
  uint64_t total;
  const uint8_t* src;
  const uint64_t* rho;   // the array's segment of the caller's rho (total - 1 entries), or NULL
};

void add_items(std::vector<Item>& items, bool g2, bool sums, uint32_t query, uint32_t which, const uint8_t* src,
               uint64_t total, const uint64_t* rho, uint32_t chunk) {
  const size_t w = g2 ? 128 : 64;
  for (uint64_t at = 0; at < total; at += chunk) {
    const uint32_t c = (uint32_t)(total - at < chunk ? total - at : chunk);
    items.push_back(Item{g2, sums, query, which, (uint32_t)at, c, total, src + at * w, rho});
  }
}

bool all_zero(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i]) return false;
  return true;
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" g16_status g16_srs_check(int device, const g16_srs_desc* srs, const uint64_t* rho,
                                    g16_key_bad_point* bad_out, uint32_t bad_cap, g16_srs_report* report) {
  if (!srs || !report || (bad_cap && !bad_out)) return G16_ERR_INVALID;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  const uint64_t n1 = srs->n_tau_g1, n2 = srs->n_tau;
  if (n1 < 2 || n2 < 2) return G16_ERR_INVALID;
  const uint64_t n_rho = (n1 - 1) + 3 * (n2 - 1);
  if (!rho_all_nonzero(rho, n_rho)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&]() -> g16_status {
    const uint32_t chunk = chunk_from_env("G16_SRSCHECK_CHUNK", SC_DEFAULT_CHUNK, n1 > n2 ? n1 : n2);
    // G16_SRSCHECK_SLICED=1 (measurements): the shifted sums as two ladders in two blockIdx.y slices
    const char* sl = getenv("G16_SRSCHECK_SLICED");
    const bool sliced = sl && sl[0] == '1';
    const uint32_t nb_max = ceil_div(chunk, KC_BLOCK);

    // what needs no arithmetic: compared as bytes on the host, reported with the relations
    const G1Affine g1{Fq::one(), Fq::from_u32(2)};
    uint32_t host_bits = 0;
    if (memcmp(srs->tau_g1, &g1, 64) || memcmp(srs->tau_g2, G2_GEN_WORDS, 128)) host_bits |= G16_SRS_BASE;
    if (all_zero(srs->tau_g1 + 64, 64) || all_zero(srs->tau_g2 + 128, 128) || all_zero(srs->alpha_tau_g1, 64) ||
        all_zero(srs->beta_tau_g1, 64) || all_zero(srs->beta_g2, 128))
      host_bits |= G16_SRS_DEGENERATE;

    // rho segments in the order tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1
    const uint64_t* r_tau1 = rho;
    const uint64_t* r_tau2 = rho ? rho + 2 * (n1 - 1) : nullptr;
    const uint64_t* r_alpha = rho ? r_tau2 + 2 * (n2 - 1) : nullptr;
    const uint64_t* r_beta = rho ? r_alpha + 2 * (n2 - 1) : nullptr;
    std::vector<Item> items;
    add_items(items, false, true, G16_SRS_Q_TAU_G1, 0, srs->tau_g1, n1, r_tau1, chunk);
    add_items(items, true, true, G16_SRS_Q_TAU_G2, 0, srs->tau_g2, n2, r_tau2, chunk);
    add_items(items, false, true, G16_SRS_Q_ALPHA_TAU_G1, 1, srs->alpha_tau_g1, n2, r_alpha, chunk);
    add_items(items, false, true, G16_SRS_Q_BETA_TAU_G1, 2, srs->beta_tau_g1, n2, r_beta, chunk);
    add_items(items, true, false, G16_SRS_Q_SINGLES, 0, srs->beta_g2, 1, nullptr, chunk);

    G16_HIP(hipSetDevice(device));
    ScKey hk;
    memcpy(&hk.tau1, srs->tau_g1 + 64, 64);
    memcpy(&hk.beta1, srs->beta_tau_g1, 64);
    memcpy(&hk.tau2, srs->tau_g2 + 128, 128);
    memcpy(&hk.beta2, srs->beta_g2, 128);
    hk.g1_neg = g1.neg();
    memcpy(&hk.g2, G2_GEN_WORDS, 128);
    std::unique_ptr<ScState> hs(new ScState());
    memset(hs.get(), 0, sizeof(ScState));
    uint64_t* n_points = hs->tally.n_points;
    n_points[G16_SRS_Q_TAU_G1] = n1;
    n_points[G16_SRS_Q_TAU_G2] = n_points[G16_SRS_Q_ALPHA_TAU_G1] = n_points[G16_SRS_Q_BETA_TAU_G1] = n2;
    n_points[G16_SRS_Q_SINGLES] = 1;

    const size_t off_rho = (size_t)chunk * 128;  // a slot: points | chunk + 1 coefficients
    CheckStage stage(off_rho + ((size_t)chunk + 1) * 16, chunk, G16_SRS_N_QUERIES, bad_cap);
    DevBuf<ScKey> dkey;
    DevBuf<ScState> dst;
    DevBuf<G1XYZZ> dpart1;
    DevBuf<G2XYZZ> dpart2;
    dkey.alloc(1);
    dst.alloc(1);
    dpart1.alloc(2 * (size_t)nb_max);
    dpart2.alloc(2 * (size_t)nb_max);
    G16_HIP(hipMemcpy(dkey.p, &hk, sizeof hk, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dst.p, hs.get(), sizeof(ScState), hipMemcpyHostToDevice));
    const hipStream_t copy = stage.copy.s, comp = stage.comp.s;
    uint8_t* flags = stage.dflags.p;

    uint64_t carry[2] = {0, 0};  // drawn rho: the last coefficient of the chunk before, the first of this one's
    for (const Item& it : items) {
      const auto [h, d] = stage.begin();
      const uint32_t n = it.count;
      const size_t bytes = (size_t)n * (it.g2 ? 128 : 64);
      memcpy(h, it.src, bytes);
      G16_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, copy));
      if (it.sums) {
        // entry e of the slot = rho_{base - 1 + e}, e <= n; rho_{-1} = rho_{total - 1} = 0
        uint64_t* hr = (uint64_t*)(h + off_rho);
        const uint64_t first = it.base ? 0 : 1;                                        // entries that are rho_{-1}
        const uint64_t last = (uint64_t)it.base + n == it.total ? n - 1 : n;           // last entry that is a rho
        if (first) hr[0] = hr[1] = 0;
        if (last < n) hr[2 * (size_t)n] = hr[2 * (size_t)n + 1] = 0;
        if (it.rho) {
          if (last >= first)
            memcpy(hr + 2 * first, it.rho + 2 * ((size_t)it.base + first - 1), (size_t)(last - first + 1) * 16);
        } else {  // drawn chunk by chunk, straight into the staging slot; the seam coefficient is carried
          uint64_t from = first;
          if (!first) {
            hr[0] = carry[0];
            hr[1] = carry[1];
            from = 1;
          }
          if (last >= from && !draw_rho(hr + 2 * from, (size_t)(last - from + 1))) {
            stage.drain();
            return G16_ERR_INTERNAL;
          }
          carry[0] = hr[2 * (size_t)n];
          carry[1] = hr[2 * (size_t)n + 1];
        }
        G16_HIP(hipMemcpyAsync(d + off_rho, h + off_rho, ((size_t)n + 1) * 16, hipMemcpyHostToDevice, copy));
      }
      stage.staged();
      const uint32_t nb = ceil_div(n, KC_BLOCK);
      const uint64_t* drho = (const uint64_t*)(d + off_rho);
      if (it.g2) {
        G16_LAUNCH(k_chk_flags_g2, nb, KC_BLOCK, 0, comp, (const VkDev*)stage.dvk.p, (const G2Affine*)d, n, 1u, flags);
        if (it.sums) {
          if (sliced)
            G16_LAUNCH(k_sc_pair_g2_sliced, dim3(nb, 2), KC_BLOCK, 0, comp, (const G2Affine*)d, drho,
                       (const uint8_t*)flags, n, dpart2.p);
          else
            G16_LAUNCH(k_sc_pair_g2, nb, KC_BLOCK, 0, comp, (const G2Affine*)d, drho, (const uint8_t*)flags, n,
                       dpart2.p);
          G16_LAUNCH(k_chk_fold<G2XYZZ>, 1, KC_BLOCK, 0, comp, (const G2XYZZ*)dpart2.p, nb, 2u, dst.p->sum2);
        }
      } else {
        G16_LAUNCH(k_chk_flags_g1, nb, KC_BLOCK, 0, comp, (const G1Affine*)d, n, flags);
        if (sliced)
          G16_LAUNCH(k_sc_pair_g1_sliced, dim3(nb, 2), KC_BLOCK, 0, comp, (const G1Affine*)d, drho,
                     (const uint8_t*)flags, n, dpart1.p);
        else
          G16_LAUNCH(k_sc_pair_g1, nb, KC_BLOCK, 0, comp, (const G1Affine*)d, drho, (const uint8_t*)flags, n,
                     dpart1.p);
        G16_LAUNCH(k_chk_fold<G1XYZZ>, 1, KC_BLOCK, 0, comp, (const G1XYZZ*)dpart1.p, nb, 2u, dst.p->sum1[it.which]);
      }
      stage.collect(flags, n, it.query, it.query, it.base, &dst.p->tally);
      stage.end();
    }
    G16_LAUNCH(k_sc_final, 1, KC_BLOCK, 0, comp, (const VkDev*)stage.dvk.p, (const ScKey*)dkey.p, dst.p,
               (const g16_key_bad_point*)stage.dlists.p, stage.cap, host_bits, stage.dout.p);
    stage.finish(hs.get(), dst.p, report, bad_out);
    return G16_OK;
  });
}
