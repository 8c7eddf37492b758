// keycheck.h -- what g16_key_check (keycheck.hip) and the phase-2 calls (contribute.hip) share: the per-point
// predicates and their flag byte, the 128-bit multiplication and the per-block LDS sum of the small-exponent
// tests, and the RAII boxes of the streamed staging (two page-locked host slots, two device slots).
#pragma once
#include "../../include/g16_amd.h"

#include "pairing.h"

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

G16_HD uint8_t g2_flag(const G2Affine& p, const VkDev* vk) {
  if (!(fq2_words_canonical(p.x) && fq2_words_canonical(p.y))) return G16_KEY_BAD_NONCANONICAL;
  if (p.is_inf()) return KC_INF;
  if (!on_curve_g2(p, vk)) return G16_KEY_BAD_OFF_CURVE;
  return g2_r_torsion(p) ? 0 : G16_KEY_BAD_SUBGROUP;
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

struct PinnedBuf {
  uint8_t* p = nullptr;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  void alloc(size_t bytes) { G16_HIP(hipHostMalloc((void**)&p, bytes, hipHostMallocPortable)); }
};
struct StreamBox {
  hipStream_t s = nullptr;
  bool made = false;
  ~StreamBox() {
    if (made) (void)hipStreamDestroy(s);
  }
  void create() {
    G16_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    made = true;
  }
};
struct EventBox {
  hipEvent_t e = nullptr;
  bool made = false;
  ~EventBox() {
    if (made) (void)hipEventDestroy(e);
  }
  void create() {
    G16_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    made = true;
  }
};

}  // namespace g16
