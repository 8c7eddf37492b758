// emu_y3_exports.cpp -- TEST INFRASTRUCTURE ONLY: the host compilation of field29.h's mul_sub_y3 (a b - c d under the
// name ec29.h forms every Y3 with) on raw limb patterns, F29_CHECK asserts active, next to the split form
// (a * b - c * d).carry() of the same operands.  Linked only into tests/emu/libg16_emu.so.
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
// out: canonical Fq2x29::mul_sub_y3(a, b, c, d), 16 words; raw: its limbs before canonicalisation (18 per case);
// split_out: canonical Fq2x29::mul_sub_split of the same operands.
void emu_fq2x29_mul_sub_y3(const int32_t* limbs, uint32_t* out, int32_t* raw, uint32_t* split_out, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const int32_t* p = limbs + 72 * i;
    const Fq2x29 a = load2(p), b = load2(p + 18), c = load2(p + 36), d = load2(p + 54);
    const Fq2x29 r = Fq2x29::mul_sub_y3(a, b, c, d);
    memcpy(raw + 18 * i, r.c0.l, 36);
    memcpy(raw + 18 * i + 9, r.c1.l, 36);
    pack2(r.canonical(), out + 16 * i);
    pack2(Fq2x29::mul_sub_split(a, b, c, d).canonical(), split_out + 16 * i);
  }
}
// the G1 field: mul_sub_y3 is mul_sub.  limbs: n x (a | b | c | d), 9 limbs each; out / sub_out: 8 words per case
void emu_fq29_mul_sub_y3(const int32_t* limbs, uint32_t* out, int32_t* raw, uint32_t* sub_out, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    Fq29 v[4];
    for (int k = 0; k < 4; ++k) memcpy(v[k].l, limbs + 36 * i + 9 * k, 36);
    const Fq29 r = Fq29::mul_sub_y3(v[0], v[1], v[2], v[3]);
    memcpy(raw + 9 * i, r.l, 36);
    uint32_t w[8];
    r.canonical().pack(w);
    memcpy(out + 8 * i, w, 32);
    Fq29::mul_sub(v[0], v[1], v[2], v[3]).canonical().pack(w);
    memcpy(sub_out + 8 * i, w, 32);
  }
}
}
