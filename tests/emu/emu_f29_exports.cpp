// emu_f29_exports.cpp -- TEST INFRASTRUCTURE ONLY: the host compilation of field29.h's Fq2 squaring on raw limb
// patterns (F29_CHECK asserts active), so pytest can drive it to the limb / value extremes of its call sites.
// Linked only into tests/emu/libg16_emu.so.
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
}  // namespace

extern "C" {
// limbs: n x (9 limbs of c0 | 9 limbs of c1).  out_sqr: canonical a.sqr(), out_mul: canonical a * a; 16 words each
void emu_fq2x29_sqr(const int32_t* limbs, uint32_t* out_sqr, uint32_t* out_mul, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    Fq2x29 a;
    memcpy(a.c0.l, limbs + 18 * i, 36);
    memcpy(a.c1.l, limbs + 18 * i + 9, 36);
    pack2(a.sqr().canonical(), out_sqr + 16 * i);
    pack2((a * a).canonical(), out_mul + 16 * i);
  }
}
}
