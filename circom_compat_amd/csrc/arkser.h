// arkser.h -- what the ark-serialize codec (arkser.hip) and the tests' square-root hooks (tests/arith/sqrt_hooks.hip)
// share: square roots in Fq and Fq2, the `y > -y` order of ark-serialize's sign flag, and the layout walk of the
// containers (loaders.cpp).
//
// q = 3 (mod 4).  With E = (q - 3) / 4 and w = a^E:  r = w a = a^((q+1)/4) is a root of a when a is a residue, and
// r w = a^((q-1)/2) is Euler's symbol, so w = 1 / r for a residue and -1 / r for a non-residue (then r^2 = -a).
// One 252-bit exponentiation gives the root AND its inverse.
//
// Fq2 = Fq[i] / (i^2 + 1), a = a0 + a1 i, the norm method with two Fq exponentiations and no inversion:
//   s = sqrt(a0^2 + a1^2)                      first exponentiation
//   t = (a0 + s) / 2,  w = t^E,  c = t w       second: c^2 = t (t a residue) or c^2 = -t (t a non-residue)
//   d = a1 w / 2
//   t a residue:      y = c + d i   (d = a1 / (2 c))
//   t a non-residue:  y = -d + c i  (w = -1 / c, so -d = a1 / (2 c); then d^2 = (a0 - s) / 2, the other sign of t)
// Both signs of t = (a0 +- s) / 2 are thus reached by ONE exponentiation: (a0 + s)(a0 - s) / 4 = -a1^2 / 4, so the
// root of the other candidate is a1 / (2 sqrt(-t)).  a1 = 0 is its own branch (t would be 0 or a0): y = sqrt(a0)
// or sqrt(-a0) i, one exponentiation.  The VERDICT is always the final check y^2 == a, never a residue test on the
// way: a non-residue norm or a wrong guess just fails it.
#pragma once
#include "../../include/g16_loaders.h"
#include "ec.h"

#include <string>

namespace g16 {

struct AkParams {
  // E = (q - 3) / 4, 252 bits
  static constexpr uint32_t E[8] = {0xb61f3f51u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u,
                                    0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
  static constexpr int E_TOP = 251;
  // (q - 1) / 2: a canonical y above it is "negative"
  static constexpr uint32_t HALF[8] = {0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u,
                                       0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
  // 1 / 2, Montgomery
  static constexpr uint32_t INV2[8] = {0x4f060572u, 0x87bee7d2u, 0x2f1c6ae5u, 0xd0fd2addu,
                                       0xfcfd4f44u, 0x8f5f7492u, 0x3d9cbfacu, 0x1f37631au};
};

// a^((q-3)/4): the words of the exponent are constants read one per 32 positions, nothing is indexed per lane
G16_HD Fq fq_pow_e(const Fq& a) {
  Fq r = a;  // bit E_TOP
#pragma unroll 1
  for (int i = AkParams::E_TOP - 1; i >= 0; --i) {
    r = r.sqr();
    if ((AkParams::E[i >> 5] >> (i & 31)) & 1) r = r * a;
  }
  return r;
}

// *root = a root of a when there is one; returns root^2 == a
G16_HD bool fq_sqrt(const Fq& a, Fq* root) {
  const Fq r = fq_pow_e(a) * a;
  *root = r;
  return r.sqr() == a;
}

G16_HD bool fq2_sqrt(const Fq2& a, Fq2* root) {
  Fq2 y;
  if (a.c1.is_zero()) {
    const Fq r = fq_pow_e(a.c0) * a.c0;  // r^2 = a0 or -a0
    y = r.sqr() == a.c0 ? Fq2{r, Fq::zero()} : Fq2{Fq::zero(), r};
  } else {
    Fq inv2;
#pragma unroll
    for (int i = 0; i < 8; ++i) inv2.v[i] = AkParams::INV2[i];
    const Fq n = a.c0.sqr() + a.c1.sqr();
    const Fq s = fq_pow_e(n) * n;
    const Fq t = (a.c0 + s) * inv2;
    const Fq w = fq_pow_e(t);
    const Fq c = t * w, d = a.c1 * w * inv2;
    y = c.sqr() == t ? Fq2{c, d} : Fq2{d.neg(), c};
  }
  *root = y;
  return y.sqr() == a;
}

// canonical integer > (q - 1) / 2
G16_HD bool ak_above_half(const uint32_t (&v)[8]) {
  for (int i = 7; i >= 0; --i) {
    if (v[i] > AkParams::HALF[i]) return true;
    if (v[i] < AkParams::HALF[i]) return false;
  }
  return false;
}
// ark-serialize's sign flag: y > -y on canonical integers; in Fq2 lexicographic with c1 FIRST.  The order is
// stated once, on the canonical words; a Montgomery value is converted and asked the same question.
G16_HD bool ak_canon_negative(const Fq& c) { return ak_above_half(c.v); }
G16_HD bool ak_canon_negative(const Fq2& c) { return c.c1.is_zero() ? ak_above_half(c.c0.v) : ak_above_half(c.c1.v); }
G16_HD Fq ak_from_mont(const Fq& a) {  // the canonical integer, in the words of an Fq
  Fq r;
  const U256 u = a.to_canonical();
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = u.v[i];
  return r;
}
G16_HD Fq2 ak_from_mont(const Fq2& a) { return Fq2{ak_from_mont(a.c0), ak_from_mont(a.c1)}; }
template <class F>
G16_HD bool ak_is_negative(const F& y) {
  return ak_canon_negative(ak_from_mont(y));
}

// loaders.cpp: the message behind g16_loader_last_error and the names of the containers' fields (G16_ARK_F_*), for
// the container calls of arkser.hip
g16_status loader_fail(g16_status code, const std::string& message);
const char* ark_field_name(int field);

}  // namespace g16
