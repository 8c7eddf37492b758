// keycheck.h -- the streamed point-check core of the four validators: g16_key_check (keycheck.hip),
// g16_key_contribution_check (contribute.hip), g16_srs_check (srs_check.hip) and g16_srs_lagrange_check
// (srs_prepare.hip).  One copy of everything they have in common; each including file gets its own instance of the
// kernels (anonymous namespace, as in gtransform.h).
//   device   the per-point predicates and their flag byte, k_chk_flags_g1 / _g2 (one reason byte per point),
//            k_chk_collect (one block: counts the flags and appends the bad points, in index order, to the
//            slot's list -- a scan, no atomics: the list does not depend on scheduling), the 128-bit
//            multiplication, the per-block LDS sum and chk_fold / k_chk_fold (block sums into a running sum) of the
//            small-exponent tests, and the halves every final kernel shares: chk_offsets, chk_pairs, chk_counts,
//            chk_emit_lists.  What is left to a check is its table of pairs and its own relation bits.
//   host     CheckStage, the streamed staging of one call (two page-locked host slots, two device slots, the copy
//            of chunk k + 1 under the kernels of chunk k, one synchronisation before the download), rho_all_nonzero
//            and vk_consts.  The RAII boxes, device_ok and chunk_from_env are hostcall.h's, draw_rho is secret.h's.
#pragma once
#include <memory>

#include "hostcall.h"
#include "pairing.h"
#include "secret.h"

namespace g16 {

constexpr uint32_t KC_BLOCK = 64;           // lanes per block of the per-point kernels
constexpr uint32_t KC_SCAN = 256;           // lanes of the one-block flag scan
constexpr uint32_t KC_MAX_LISTED = 1u << 16;  // bad points listed per call (all are counted)
constexpr uint8_t KC_INF = 0x80;            // flag byte: the point at infinity (bits 0..2: G16_KEY_BAD_*)

// the standard generators (EIP-197), Montgomery form
constexpr uint32_t G2_GEN_WORDS[4][8] = {
    {0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u},
    {0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u},
    {0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu},
    {0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u}};

G16_HD bool fq2_words_canonical(const Fq2& a) { return fq_words_canonical(a.c0) && fq_words_canonical(a.c1); }

// the first test that fails, in the order k_verify_batch applies them: arithmetic on a value >= q, or the
// group law on a point off the curve, would mean nothing
G16_HD uint8_t g1_flag(const G1Affine& p) {
  if (!(fq_words_canonical(p.x) && fq_words_canonical(p.y))) return G16_KEY_BAD_NONCANONICAL;
  if (p.is_inf()) return KC_INF;
  return on_curve_g1(p) ? 0 : G16_KEY_BAD_OFF_CURVE;
}

// [r] P = infinity, the predicate of g2_in_subgroup (pairing.h), as one loop over the bits of r with a mixed
// addition of the affine P (8M + 2S in Fq2 instead of the 12M + 2S of XYZZ + XYZZ)
G16_HD bool g2_r_torsion(const G2Affine& p) {
  G2XYZZ acc = G2XYZZ::from_affine(p);  // bit 253, the top bit of r
#pragma unroll 1
  for (int i = 252; i >= 0; --i) {
    acc.dbl_in_place();
    if ((FrParams::MOD[i >> 5] >> (i & 31)) & 1) acc.madd(p);
  }
  return acc.is_inf();
}

// subgroup = false: canonical words and the curve equation only
G16_HD uint8_t g2_flag(const G2Affine& p, const VkDev* vk, bool subgroup = true) {
  if (!(fq2_words_canonical(p.x) && fq2_words_canonical(p.y))) return G16_KEY_BAD_NONCANONICAL;
  if (p.is_inf()) return KC_INF;
  if (!on_curve_g2(p, vk)) return G16_KEY_BAD_OFF_CURVE;
  return (!subgroup || g2_r_torsion(p)) ? 0 : G16_KEY_BAD_SUBGROUP;
}

// rho * p for a 128-bit rho = hi : lo, MSB first
template <class F>
G16_HD XYZZ<F> mul_rho(const Affine<F>& p, uint64_t lo, uint64_t hi) {
  XYZZ<F> acc = XYZZ<F>::infinity();
  if (p.is_inf()) return acc;
#pragma unroll 1
  for (int i = 127; i >= 0; --i) {
    acc.dbl_in_place();
    const uint64_t w = i >= 64 ? hi : lo;
    if ((w >> (i & 63)) & 1) acc.madd(p);
  }
  return acc;
}

// sh[0] <- sum of sh[0 .. KC_BLOCK): every lane of the block calls it, v = the lane's own term (fixed tree)
template <class T>
__device__ __forceinline__ void kc_block_sum(T* sh, T v) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
#pragma unroll 1
  for (uint32_t s = KC_BLOCK / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      v.add(sh[t + s]);
      sh[t] = v;
    }
  }
  __syncthreads();
}


// ---- the shared kernels ------------------------------------------------------------------------------
// what a call counts per slot (a query or an array): device-resident, embedded in the call's state
constexpr uint32_t CHK_SLOTS = G16_KEY_N_QUERIES;  // the largest query count in use
static_assert(CHK_SLOTS >= (uint32_t)G16_SRS_N_QUERIES && CHK_SLOTS >= (uint32_t)G16_LAGRANGE_N_ARRAYS, "tally slots");
struct CheckTally {
  uint64_t n_points[CHK_SLOTS], n_bad[CHK_SLOTS], n_infinity[CHK_SLOTS];
  uint32_t n_list[CHK_SLOTS];  // entries in the slot's list (<= cap)
};

// *sum += the nb block sums of a chunk: every lane of the one block calls it
template <class P>
__device__ __forceinline__ void chk_fold(const P* part, uint32_t nb, P* sum, P* sh) {
  const uint32_t t = threadIdx.x;
  P a = P::infinity();
#pragma unroll 1
  for (uint32_t k = t; k < nb; k += KC_BLOCK) a.add(part[k]);
  kc_block_sum(sh, a);
  if (t == 0) {
    P s = *sum;
    s.add(sh[0]);
    *sum = s;
  }
}

// the list offsets of the final kernel: sh_off[q] = where slot q starts in the output (the lists concatenated in
// slot order, cut at bad_cap), sh_off[nq] = entries in all; every lane calls it, returns "any bad point"
__device__ __forceinline__ bool chk_offsets(const CheckTally* tally, uint32_t nq, uint32_t bad_cap, uint32_t* sh_off) {
  if (threadIdx.x == 0) {
    uint64_t bad = 0;
    uint32_t off = 0;
    for (uint32_t q = 0; q < nq; ++q) {
      bad += tally->n_bad[q];
      sh_off[q] = off;
      const uint32_t room = bad_cap - off;
      off += tally->n_list[q] < room ? tally->n_list[q] : room;
    }
    sh_off[nq] = off;
    sh_off[nq + 1] = bad ? 1 : 0;
  }
  __syncthreads();
  return sh_off[nq + 1] != 0;
}

// lanes 2k, 2k + 1 hold the two sides (Q, P) of pair k < n_pairs and run its Miller loops, lanes 0 .. n_pairs - 1
// its product and final exponentiation; every lane calls it, every other lane with Q = P = infinity.  Returns
// bit k = pair k is not one.  !pair (a structural check failed): Q = P = infinity everywhere, nothing is computed.
__device__ __forceinline__ uint32_t chk_pairs(const G2Affine& Q, const G1Affine& P, uint32_t n_pairs, bool pair,
                                              const VkDev* vk, F12* sh, uint32_t* sh_fail) {
  const uint32_t t = threadIdx.x;
  F12 f = f12_one();
  miller_mul(&f, &Q, &P, vk);  // one call site: infinity on either side (every idle lane) returns at once
  if (t < 2 * n_pairs) sh[t] = f;
  __syncthreads();
  if (t < n_pairs) {
    bool one = true;
    if (pair) {
      F12 g;
      f12_mul(&g, &sh[2 * t], &sh[2 * t + 1]);
      one = final_exp_is_one(&g, vk);
    }
    sh_fail[t] = one ? 0 : (1u << t);
  }
  __syncthreads();
  uint32_t failed = 0;
  for (uint32_t k = 0; k < n_pairs; ++k) failed |= sh_fail[k];
  return failed;
}

// the per-slot counts of a report with n_points / n_bad / n_infinity arrays
template <class R>
__device__ __forceinline__ void chk_counts(R* r, const CheckTally* tally, uint32_t nq) {
  for (uint32_t q = 0; q < nq; ++q) {
    r->n_points[q] = tally->n_points[q];
    r->n_bad[q] = tally->n_bad[q];
    r->n_infinity[q] = tally->n_infinity[q];
  }
}

// the slots' lists, concatenated in (slot, index) order at the offsets of chk_offsets; every lane calls it
__device__ __forceinline__ void chk_emit_lists(const uint32_t* sh_off, uint32_t nq, const g16_key_bad_point* lists,
                                               uint32_t cap, g16_key_bad_point* out_list) {
#pragma unroll 1
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t cnt = sh_off[q + 1] - sh_off[q];
#pragma unroll 1
    for (uint32_t k = threadIdx.x; k < cnt; k += KC_BLOCK) out_list[sh_off[q] + k] = lists[(size_t)q * cap + k];
  }
}

namespace {

__global__ void __launch_bounds__(KC_BLOCK) k_chk_flags_g1(const G1Affine* pts, uint32_t n, uint8_t* flags) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  flags[i] = g1_flag(pts[i]);
}

__global__ void __launch_bounds__(KC_BLOCK) k_chk_flags_g2(const VkDev* vk, const G2Affine* pts, uint32_t n,
                                                           uint32_t subgroup, uint8_t* flags) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  flags[i] = g2_flag(pts[i], vk, subgroup != 0);
}

// one block: part holds `sides` runs of nb block sums; run s goes into sum[s]
template <class P>
__global__ void __launch_bounds__(KC_BLOCK) k_chk_fold(const P* part, uint32_t nb, uint32_t sides, P* sum) {
  __shared__ P sh[KC_BLOCK];
#pragma unroll 1
  for (uint32_t side = 0; side < sides; ++side) {
    chk_fold(part + (size_t)side * nb, nb, sum + side, sh);
    __syncthreads();
  }
}

// one block: lane t owns the contiguous run [t * seg, (t + 1) * seg) of the chunk's flags; counts, an exclusive
// scan of the counts, then every lane appends its bad points behind those of the lanes before it.  slot: the
// tally entry and the list region; query_id: what the list entries name; base: the chunk's first index.
__global__ void __launch_bounds__(KC_SCAN) k_chk_collect(const uint8_t* flags, uint32_t n, uint32_t slot,
                                                         uint32_t query_id, uint32_t base, CheckTally* tally,
                                                         g16_key_bad_point* lists, uint32_t cap) {
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
    const uint32_t start = tally->n_list[slot];
    sh_start = start;
    tally->n_bad[slot] += run;
    tally->n_infinity[slot] += infs;
    tally->n_list[slot] = (uint64_t)start + run < cap ? start + run : cap;
  }
  __syncthreads();
  uint64_t at = (uint64_t)sh_start + sh_bad[t];
  g16_key_bad_point* list = lists + (size_t)slot * cap;
#pragma unroll 1
  for (uint32_t i = lo; i < hi && bad && at < cap; ++i) {
    const uint8_t f = flags[i] & ~KC_INF;
    if (!f) continue;
    list[at].query = query_id;
    list[at].index = base + i;
    list[at].reason = f;
    ++at;
  }
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------
// a caller's n coefficients of 2 x u64 (NULL: the library draws them)
inline bool rho_all_nonzero(const uint64_t* rho, uint64_t n) {
  if (rho)
    for (uint64_t i = 0; i < n; ++i)
      if (!(rho[2 * i] | rho[2 * i + 1])) return false;
  return true;
}

// the curve and Frobenius constants of a VkDev; the key's own fields are the caller's
inline void vk_consts(VkDev* hv) {
  const HostConsts& H = host_consts();
  hv->frob_x = H.frob_x;
  hv->frob_y = H.frob_y;
  hv->b_twist = H.b_twist;
  memcpy(hv->frob, H.frob, sizeof H.frob);
}

// The streamed staging of one check call and every allocation the four checks have in common: nothing is allocated
// inside the chunk loop, device memory is fixed by the chunk and not by the input.  Per chunk
//     auto [h, d] = begin();  fill h, hipMemcpyAsync h -> d on copy.s;  staged();  launches on comp.s;  end();
// the host fills slot k + 1 and its copy runs while the kernels of slot k do.
namespace {  // it launches this file's k_chk_collect

struct CheckStage {
  PinnedBuf pin[2];
  DevBuf<uint8_t> dslot[2], dflags;
  DevBuf<VkDev> dvk;  // the constants of vk_consts, everything else zero
  DevBuf<g16_key_bad_point> dlists, dout;
  StreamBox copy, comp;
  EventBox copied[2], done[2];
  uint32_t cap;  // entries per list region and in the output: min(bad_cap, KC_MAX_LISTED)
  size_t k = 0;  // chunks begun so far: the slot is (k - 1) & 1

  struct Slot {
    uint8_t* h;
    uint8_t* d;
  };

  CheckStage(size_t slot_bytes, size_t n_flags, uint32_t n_regions, uint32_t bad_cap)
      : cap(bad_cap < KC_MAX_LISTED ? bad_cap : KC_MAX_LISTED) {
    for (int s = 0; s < 2; ++s) {
      pin[s].alloc(slot_bytes);
      dslot[s].alloc(slot_bytes);
      copied[s].create();
      done[s].create();
    }
    dflags.alloc(n_flags);
    dvk.alloc(1);
    dlists.alloc((size_t)n_regions * (cap ? cap : 1));
    dout.alloc(cap ? cap : 1);
    copy.create();
    comp.create();
    std::unique_ptr<VkDev> hv(new VkDev());
    memset(hv.get(), 0, sizeof(VkDev));
    vk_consts(hv.get());
    G16_HIP(hipMemcpy(dvk.p, hv.get(), sizeof(VkDev), hipMemcpyHostToDevice));
  }

  Slot begin() {
    const int s = (int)(k++ & 1);
    if (k > 2) G16_HIP(hipEventSynchronize(done[s].e));  // the kernels that read this slot two chunks ago
    return Slot{pin[s].p, dslot[s].p};
  }
  void staged() {
    const int s = (int)((k - 1) & 1);
    G16_HIP(hipEventRecord(copied[s].e, copy.s));
    G16_HIP(hipStreamWaitEvent(comp.s, copied[s].e, 0));
  }
  // counts the chunk's flags into tally slot `slot` and lists its bad points under query_id (k_chk_collect)
  void collect(const uint8_t* flags, uint32_t n, uint32_t slot, uint32_t query_id, uint32_t base, CheckTally* tally) {
    G16_LAUNCH(k_chk_collect, 1, KC_SCAN, 0, comp.s, flags, n, slot, query_id, base, tally, dlists.p, cap);
  }
  void end() { G16_HIP(hipEventRecord(done[(k - 1) & 1].e, comp.s)); }
  // a draw failed: the chunks in flight still read the slots
  void drain() {
    (void)hipStreamSynchronize(copy.s);
    (void)hipStreamSynchronize(comp.s);
  }
  // after the final kernel: the one synchronisation, then the state (with its report) and the list come down
  template <class S, class R>
  void finish(S* hs, const S* ds, R* report, g16_key_bad_point* bad_out) {
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(comp.s));
    G16_HIP(hipMemcpy(hs, ds, sizeof(S), hipMemcpyDeviceToHost));
    *report = hs->report;
    if (report->n_listed)
      G16_HIP(hipMemcpy(bad_out, dout.p, (size_t)report->n_listed * sizeof(g16_key_bad_point), hipMemcpyDeviceToHost));
  }
};

}  // namespace

}  // namespace g16
