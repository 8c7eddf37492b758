// gt.h -- pairing VALUES (elements of GT, the order-r subgroup of Fq12*) on the wave-cooperative arithmetic of
// pairing_coop.h: the power of an element held in LDS, and the change of basis between the library's flat form and
// the tower form every other BN254 software uses.  gt.hip has the kernels and the entry points.
//
// Convention.  A pairing value here is  ML(Q, P)^((q^12 - 1) / r * m),  m = 2 x (6 x^2 + 3 x + 1),  x = 4965661367192848881:
// coop_final_exp's chain is ark-ec's bn::final_exponentiation, whose Fuentes-Castaneda hard part computes the m-th
// power of the "plain" reduced pairing f^((q^12 - 1) / r).  gcd(m, r) = 1, so it is a pairing all the same, and it is
// the one snarkjs and arkworks hand out: tests/golden/verification_key.json's vk_alphabeta_12 pins it.
//
// Flat form (the library's): Fq12 = Fq[w] / (w^12 - 18 w^6 + 82), a = sum a_i w^i, 12 x 32 bytes, a_i Montgomery.
// Tower form (ark-ff Fq12::serialize, snarkjs' [2][3][2] nesting): Fq2 = Fq[u] / (u^2 + 1), Fq6 = Fq2[v] / (v^3 - xi),
// Fq12 = Fq6[w] / (w^2 - v), xi = 9 + u.  With w^6 = xi:  a = sum_{i < 6} (a_i + a_{i+6} xi) w^i, and w^i =
// v^(i >> 1) w^(i & 1), so the Fq2 coefficient (a_i + 9 a_{i+6}, a_{i+6}) sits at Fq12.c_{i & 1}, Fq6.c_{i >> 1}: slot
// 3 (i & 1) + (i >> 1) of the six Fq2 slots, 64 bytes each, c0 first, every Fq canonical little-endian.
#pragma once
#include "pairing_coop.h"

namespace g16 {
namespace {

constexpr uint32_t GT_BYTES = 384;
constexpr uint32_t GT_CODEC_BLOCK = 256;

G16_HD uint32_t gt_slot(int i) { return 3u * (uint32_t)(i & 1) + (uint32_t)(i >> 1); }

// flat Montgomery -> tower canonical
G16_HD void gt_flat_to_tower(const F12& a, uint8_t* out) {
#pragma unroll 1
  for (int i = 0; i < 6; ++i) {
    const Fq b = a.c[i + 6];
    const U256 c0 = (a.c[i] + (b.dbl().dbl().dbl() + b)).to_canonical();
    const U256 c1 = b.to_canonical();
    uint8_t* o = out + 64 * gt_slot(i);
    memcpy(o, c0.v, 32);
    memcpy(o + 32, c1.v, 32);
  }
}

// tower canonical -> flat Montgomery; G16_KEY_BAD_NONCANONICAL (and a zero element) if one of the 12 words is >= q
G16_HD uint8_t gt_tower_to_flat(const uint8_t* in, F12* a) {
  bool good = true;
#pragma unroll 1
  for (int i = 0; i < 6; ++i) {
    const uint8_t* p = in + 64 * gt_slot(i);
    Fq w0, w1;
    memcpy(w0.v, p, 32);
    memcpy(w1.v, p + 32, 32);
    good = good && fq_words_canonical(w0) && fq_words_canonical(w1);
    const Fq c0 = w0 * Fq::r2(), c1 = w1 * Fq::r2();
    a->c[i] = c0 - (c1.dbl().dbl().dbl() + c1);
    a->c[i + 6] = c1;
  }
  if (good) return 0;
#pragma unroll 1
  for (int i = 0; i < 12; ++i) a->c[i] = Fq::zero();
  return G16_KEY_BAD_NONCANONICAL;
}

__device__ __forceinline__ void coop_set_one(F12* out) {
  const uint32_t t = threadIdx.x;
  if (t < 12) out->c[t] = t == 0 ? Fq::one() : Fq::zero();
  __syncthreads();
}

// out = a^e for the 256-bit integer e = 4 x u64 little-endian, the same for every lane of the block: plain
// square-and-multiply from the top set bit on coop_mul_dense, so the result depends on (a, e) alone.  out != a.
__device__ __attribute__((noinline)) void coop_pow(CoopLds& L, F12* out, const F12* a, const uint64_t* e) {
  int top = -1;
#pragma unroll 1
  for (int k = 255; k >= 0; --k)
    if ((e[k >> 6] >> (k & 63)) & 1) {
      top = k;
      break;
    }
  if (top < 0) {
    coop_set_one(out);
    return;
  }
  coop_copy(out, a);
#pragma unroll 1
  for (int bit = top - 1; bit >= 0; --bit) {
    coop_mul_dense(L, out, out, out);
    if ((e[bit >> 6] >> (bit & 63)) & 1) coop_mul_dense(L, out, out, a);
  }
}

}  // namespace
}  // namespace g16
