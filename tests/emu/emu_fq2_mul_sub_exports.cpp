// emu_fq2_mul_sub_exports.cpp -- TEST INFRASTRUCTURE ONLY: the host compilation of field29.h's F29x2::mul_sub
// (a b - c d, the Y3 of the G2 additions) on raw limb patterns, F29_CHECK asserts active: the merged form (one
// reduction per component) and the split form (a * b - c * d).carry().  Linked only into tests/emu/libg16_emu.so.
#include <string.h>

#include "field29.h"

using namespace g16;

namespace {
void pack2(const Fq2x29& a, uint32_t* out) {
  uint32_t w[8];
  a.c0.pack(w);
  memcpy(out, w, 32);
  a.c1.pack(w);
  memcpy(out + 8, w, 32);
}
Fq2x29 load2(const int32_t* limbs) {
  Fq2x29 a;
  memcpy(a.c0.l, limbs, 36);
  memcpy(a.c1.l, limbs + 9, 36);
  return a;
}
}  // namespace

extern "C" {
// limbs: n x (a | b | c | d), each 9 limbs of c0 | 9 limbs of c1.
// out: canonical mul_sub_merged(a, b, c, d), 16 words; raw: its limbs before canonicalisation (18 per case), so that the
// test can hold the result to its documented class.  split != 0: the two-product form instead.
void emu_fq2x29_mul_sub(const int32_t* limbs, uint32_t* out, int32_t* raw, size_t n, int split) {
  for (size_t i = 0; i < n; ++i) {
    const int32_t* p = limbs + 72 * i;
    const Fq2x29 a = load2(p), b = load2(p + 18), c = load2(p + 36), d = load2(p + 54);
    const Fq2x29 r = split ? Fq2x29::mul_sub_split(a, b, c, d) : Fq2x29::mul_sub_merged(a, b, c, d);
    memcpy(raw + 18 * i, r.c0.l, 36);
    memcpy(raw + 18 * i + 9, r.c1.l, 36);
    pack2(r.canonical(), out + 16 * i);
  }
}
}
