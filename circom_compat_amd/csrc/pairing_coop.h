// pairing_coop.h -- the WAVE-COOPERATIVE optimal-ate pairing of verify_prepared.hip: one workgroup of 64 lanes per
// pairing product, the Fq12 operands in LDS, the 144 coefficient products of an Fq12 multiplication spread over the
// lanes.  It stands beside pairing.h (one lane per pairing, the throughput form) and computes the same predicate
// "product of pairings == 1" in the same basis: Fq12 = Fq[w] / (w^12 - 18 w^6 + 82), c[i] = coefficient of w^i.
//
//   coop_mul      out = a * b.  Phase 1: product p = s * 12 + j is a.c[idx[s]] * b.c[j], lane p % 64 computes it
//                 (a dense a has 144 products: three per lane at most; a line has 3, 5 or 6 non-zero coefficients).
//                 Phase 2: lane m < 12 sums the products of w^m, w^(m+6), w^(m+12), w^(m+18) in a FIXED order and
//                 folds w^12 = 18 w^6 - 82 in:   m < 6:  t[m] - 82 t[m+12] - 1476 t[m+18]
//                                                m >= 6: t[m] + 18 t[m+6] + 242 t[m+12]
//                 No atomics: the result does not depend on scheduling.  Saturated field.h arithmetic (the gfx950
//                 compile decides: DESIGN.md section 9j).
//   coop_miller   ONE f for all pairs: per step f <- f^2, then one line per pair.  A pair is either ON THE FLY
//                 (G2 point given; inversion-free homogeneous projective doubling / addition steps, the formulation
//                 of ark-ec's BN doubling_step / addition_step, their independent Fq2 products in different lanes)
//                 or PREPARED (the line coefficients of every step come from a table built once per key: ark-ec's
//                 G2Prepared).  The loop is pairing.h's: 6x + 2 from the second-highest bit, then the two Frobenius
//                 steps.  Projective lines differ from pairing.h's affine ones by factors in Fq2, and a projective
//                 G1 side scales a line by a factor in Fq: the final exponentiation removes both.
//   coop_final_exp   the easy part with ONE inversion through the norms Fq12 -> Fq6 -> Fq2 -> Fq (one Fermat
//                 inversion in Fq, in one lane), then the Fuentes-Castaneda hard part of pairing.h; the value stays
//                 in LDS.  coop_final_exp_is_one compares it with 1.
// Everything here uses only __syncthreads and LDS, so the same source runs under the CPU emulator of the tests.
#pragma once
#include "keycheck.h"

namespace g16 {
namespace {

constexpr uint32_t COOP_LANES = 64;
constexpr uint32_t COOP_MAX_PAIRS = 16;
constexpr uint64_t COOP_ATE_LO = 0x9d797039be763ba8ull;  // 6x + 2 = 2^64 + this
constexpr uint32_t COOP_STEPS = 64 + 36 + 2;             // doublings + additions + the two Frobenius steps
static_assert(__builtin_popcountll(COOP_ATE_LO) == 36, "COOP_STEPS counts the set bits of 6x + 2 below the top one");

enum : uint8_t { LINE_ONE = 0, LINE_CHORD = 1, LINE_VERTICAL = 2 };

// one step of a prepared G2 point.  LINE_CHORD (tangent or chord): l = -yP + (m xP) w + c w^3 with m the slope and
// c = yT - m xT -- what line() of pairing.h evaluates.  LINE_VERTICAL: l = xP - c w^2 with c = xT.  LINE_ONE: l = 1.
struct PvkLine {
  Fq2 m, c;
};
struct PvkTable {
  PvkLine line[COOP_STEPS];
  uint8_t kind[COOP_STEPS];
  uint8_t pad[2];
  uint32_t inf;  // the point is at infinity: the pair contributes 1
};

// G1 side of a prepared pair, scaled by s in Fq*: (xs, ys, zs) = (s x, s y, s).  An affine point has zs = 1.
struct ScaledG1 {
  Fq xs, ys, zs;
  uint32_t inf, pad[3];
};

struct CoopFly {
  G2Affine q, q1, q2;  // Q, pi(Q), -pi^2(Q)
  G1Affine p;
  Fq2 T[2][3];  // homogeneous projective (X : Y : Z), double-buffered
  uint32_t live, pad[3];
};

struct CoopLds {
  Fq prod[144];
  Fq kc[4];  // 18, 82, 242, 1476
  F12 f, ln[3], y[12];
  Fq2 s[6];
  ScaledG1 sp[2];
  uint32_t flag[4];
  CoopFly fly[COOP_MAX_PAIRS];
};

__device__ const uint8_t COOP_DENSE[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
__device__ const uint8_t COOP_LINE_PROJ[6] = {0, 1, 3, 6, 7, 9};  // Fq2 coefficients at w^0, w^1, w^3
__device__ const uint8_t COOP_LINE_CHORD[5] = {0, 1, 3, 7, 9};    // w^0 in Fq
__device__ const uint8_t COOP_LINE_VERT[3] = {0, 2, 8};
__device__ const uint8_t COOP_FQ2[2] = {0, 6};

__device__ __forceinline__ void coop_init(CoopLds& L) {
  const uint32_t t = threadIdx.x;
  if (t < 4) L.kc[t] = Fq::from_u32(t == 0 ? 18u : t == 1 ? 82u : t == 2 ? 242u : 1476u);
  __syncthreads();
}

// out = a * b; a's non-zero coefficients are idx[0 .. na).  out may be a or b.
__device__ __attribute__((noinline)) void coop_mul(CoopLds& L, F12* out, const F12* a, const uint8_t* idx, int na,
                                                    const F12* b) {
  const int t = (int)threadIdx.x;
  const int np = na * 12;
#pragma unroll 1
  for (int p = t; p < np; p += (int)COOP_LANES) {
    const int s = p / 12, j = p - 12 * s;
    L.prod[p] = a->c[idx[s]] * b->c[j];
  }
  __syncthreads();
  if (t < 12) {
    const bool lo = t < 6;
    const int k1 = lo ? t + 12 : t + 6, k2 = lo ? t + 18 : t + 12;
    Fq t0 = Fq::zero(), t1 = Fq::zero(), t2 = Fq::zero();
#pragma unroll 1
    for (int s = 0; s < na; ++s) {
      const int i = idx[s];
      const Fq* row = L.prod + 12 * s;
      if ((unsigned)(t - i) < 12u) t0 = t0 + row[t - i];
      if ((unsigned)(k1 - i) < 12u) t1 = t1 + row[k1 - i];
      if ((unsigned)(k2 - i) < 12u) t2 = t2 + row[k2 - i];
    }
    out->c[t] = lo ? t0 - L.kc[1] * t1 - L.kc[3] * t2 : t0 + L.kc[0] * t1 + L.kc[2] * t2;
  }
  __syncthreads();
}
__device__ __forceinline__ void coop_mul_dense(CoopLds& L, F12* out, const F12* a, const F12* b) {
  coop_mul(L, out, a, COOP_DENSE, 12, b);
}

// out = a^(q^k) through tab[i] = (w^i)^(q^k) (global memory): out_j = sum_i a_i tab[i].c[j]
__device__ __attribute__((noinline)) void coop_frob(CoopLds& L, F12* out, const F12* a, const F12* tab) {
  const int t = (int)threadIdx.x;
#pragma unroll 1
  for (int p = t; p < 144; p += (int)COOP_LANES) {
    const int i = p / 12, j = p - 12 * i;
    L.prod[p] = a->c[i] * tab[i].c[j];
  }
  __syncthreads();
  if (t < 12) {
    Fq r = L.prod[t];
#pragma unroll 1
    for (int i = 1; i < 12; ++i) r = r + L.prod[12 * i + t];
    out->c[t] = r;
  }
  __syncthreads();
}

// out = conj(a): w -> -w.  out may be a.
__device__ __forceinline__ void coop_conj(F12* out, const F12* a) {
  const uint32_t t = threadIdx.x;
  if (t < 12) out->c[t] = (t & 1) ? a->c[t].neg() : a->c[t];
  __syncthreads();
}
__device__ __forceinline__ void coop_copy(F12* out, const F12* a) {
  const uint32_t t = threadIdx.x;
  if (t < 12) out->c[t] = a->c[t];
  __syncthreads();
}

// out = conj(a^x), x the BN parameter ("exp_by_neg_x" of ark-ec's BN template); out != a
__device__ __attribute__((noinline)) void coop_exp_neg_x(CoopLds& L, F12* out, const F12* a) {
  const uint64_t X = 4965661367192848881ull;  // bit 62 is its top bit
  coop_copy(out, a);
#pragma unroll 1
  for (int bit = 61; bit >= 0; --bit) {
    coop_mul_dense(L, out, out, out);
    if ((X >> bit) & 1) coop_mul_dense(L, out, out, a);
  }
  coop_conj(out, out);
}

// z = a + b i -> (a - 9 b) at w^shift, b at w^(shift + 6)
__device__ __forceinline__ void coop_embed(F12* l, const Fq2& z, int shift) {
  const Fq b = z.c1;
  l->c[shift] = z.c0 - (b.dbl().dbl().dbl() + b);
  l->c[shift + 6] = b;
}

// L.y[0] <- L.f^((q^12 - 1) / r * m), m = 2 x (6 x^2 + 3 x + 1) the cofactor of the Fuentes-Castaneda hard part: the
// VALUE form (gt.hip hands it out; it is the GT element ark-ec's final_exponentiation and snarkjs return).  Destroys
// L.f and the rest of L.y; ends behind a barrier.
__device__ __attribute__((noinline)) void coop_final_exp(CoopLds& L, const VkDev* vk) {
  F12* y = L.y;
  F12* f = &L.f;
  // 1 / f = conj(f) * g^(q^2) * g^(q^4) / N, g = f conj(f) in Fq6, N = g g^(q^2) g^(q^4) in Fq2
  coop_conj(&y[0], f);                   // y0 = conj(f)
  coop_mul_dense(L, &y[1], f, &y[0]);    // g
  coop_frob(L, &y[2], &y[1], vk->frob[1]);
  coop_frob(L, &y[3], &y[2], vk->frob[1]);
  coop_mul_dense(L, &y[2], &y[2], &y[3]);  // g^(q^2) g^(q^4)
  coop_mul_dense(L, &y[3], &y[1], &y[2]);  // N: c[0] and c[6] only
  if (threadIdx.x == 0) {
    const Fq b = y[3].c[6];
    const Fq a = y[3].c[0] + (b.dbl().dbl().dbl() + b);
    const Fq ni = (a.sqr() + b.sqr()).inv();
    coop_embed(&y[4], Fq2{a * ni, (b * ni).neg()}, 0);
  }
  __syncthreads();
  coop_mul_dense(L, &y[2], &y[2], &y[0]);          // conj(f) g^(q^2) g^(q^4)
  coop_mul(L, &y[2], &y[4], COOP_FQ2, 2, &y[2]);   // 1 / f
  // easy part: r = (conj(f) / f)^(q^2 + 1)
  coop_mul_dense(L, &y[0], &y[0], &y[2]);
  coop_frob(L, &y[1], &y[0], vk->frob[1]);
  F12* r = &L.f;
  coop_mul_dense(L, r, &y[1], &y[0]);
  // hard part, named as final_exp_is_one of pairing.h names them: y[k] holds y_k while it is live
  coop_exp_neg_x(L, &y[0], r);                 // y0
  coop_mul_dense(L, &y[1], &y[0], &y[0]);      // y1
  coop_mul_dense(L, &y[2], &y[1], &y[1]);      // y2
  coop_mul_dense(L, &y[3], &y[2], &y[1]);      // y3
  coop_exp_neg_x(L, &y[4], &y[3]);             // y4
  coop_mul_dense(L, &y[5], &y[4], &y[4]);      // y5
  coop_exp_neg_x(L, &y[6], &y[5]);             // y6
  coop_conj(&y[3], &y[3]);
  coop_conj(&y[6], &y[6]);
  coop_mul_dense(L, &y[7], &y[6], &y[4]);      // y7
  coop_mul_dense(L, &y[8], &y[7], &y[3]);      // y8
  coop_mul_dense(L, &y[9], &y[8], &y[1]);      // y9
  coop_mul_dense(L, &y[10], &y[8], &y[4]);     // y10
  coop_mul_dense(L, &y[11], &y[10], r);        // y11
  coop_frob(L, &y[0], &y[9], vk->frob[0]);     // y12
  coop_mul_dense(L, &y[0], &y[0], &y[11]);     // y13
  coop_frob(L, &y[8], &y[8], vk->frob[1]);
  coop_mul_dense(L, &y[0], &y[8], &y[0]);      // y14
  coop_conj(r, r);
  coop_mul_dense(L, &y[1], r, &y[9]);          // y15
  coop_frob(L, &y[1], &y[1], vk->frob[2]);
  coop_mul_dense(L, &y[0], &y[1], &y[0]);
}

// L.f^((q^12 - 1) / r * m) == 1: the check form.  Destroys L.f and L.y.
__device__ __forceinline__ bool coop_final_exp_is_one(CoopLds& L, const VkDev* vk) {
  coop_final_exp(L, vk);
  if (threadIdx.x == 0) L.flag[3] = f12_is_one(L.y[0]) ? 1u : 0u;
  __syncthreads();
  return L.flag[3] != 0;
}

// ---- on-the-fly pairs: homogeneous projective steps on the twist y^2 = x^3 + b' ------------------------------
// doubling: T <- 2 T, line -H yP + 3 J xP w + (E - B) w^3 into *l (coefficients COOP_LINE_PROJ).  Two rounds.
__device__ __forceinline__ void coop_fly_double(CoopLds& L, CoopFly& F, int cur, const Fq2& b_twist, F12* l) {
  const uint32_t t = threadIdx.x;
  Fq2* T = F.T[cur];
  if (t == 0) L.s[0] = T[0] * T[1];               // A = X Y
  else if (t == 1) L.s[1] = T[1].sqr();           // B = Y^2
  else if (t == 2) L.s[2] = T[2].sqr();           // C = Z^2
  else if (t == 3) L.s[3] = (T[1] + T[2]).sqr();  // (Y + Z)^2
  else if (t == 4) L.s[4] = T[0].sqr();           // J = X^2
  __syncthreads();
  if (t < 6) {
    const Fq2 B = L.s[1], C = L.s[2];
    if (t == 0 || t == 1 || t == 5) {
      const Fq2 E = b_twist * (C.dbl() + C);  // 3 b' Z^2
      const Fq2 Fv = E.dbl() + E;
      if (t == 0) {
        T[0] = (L.s[0] * (B - Fv)).dbl();  // 4 x ark-ec's (X3, Y3, Z3): no halving
      } else if (t == 1) {
        const Fq2 e2 = E.sqr();
        const Fq2 e4 = e2.dbl().dbl();
        T[1] = (B + Fv).sqr() - (e4.dbl() + e4);  // (B + F)^2 - 12 E^2
      } else {
        coop_embed(l, E - B, 3);
      }
    } else if (t == 2) {
      const Fq2 H = L.s[3] - (B + C);  // 2 Y Z
      T[2] = (B * H).dbl().dbl();
    } else if (t == 3) {
      const Fq2 H = L.s[3] - (B + C);
      coop_embed(l, Fq2{H.c0 * F.p.y, H.c1 * F.p.y}.neg(), 0);
    } else {  // t == 4
      const Fq2 J3 = L.s[4].dbl() + L.s[4];
      coop_embed(l, Fq2{J3.c0 * F.p.x, J3.c1 * F.p.x}, 1);
    }
  }
  __syncthreads();
}

// addition of the affine q: T[cur ^ 1] <- T[cur] + q, line lambda yP - theta xP w + (theta xq - lambda yq) w^3.
// Two rounds with a barrier each, then the point update WITHOUT one: it writes the other buffer and reads only T
// and s, which the line multiplication that follows does not touch; that multiplication's barriers cover it.
__device__ __forceinline__ void coop_fly_add(CoopLds& L, CoopFly& F, int cur, const G2Affine& q, F12* l) {
  const uint32_t t = threadIdx.x;
  const Fq2* T = F.T[cur];
  if (t == 0) L.s[0] = T[1] - q.y * T[2];       // theta
  else if (t == 1) L.s[1] = T[0] - q.x * T[2];  // lambda
  __syncthreads();
  if (t < 5) {
    const Fq2 th = L.s[0], la = L.s[1];
    if (t == 0) L.s[2] = th.sqr();  // C
    else if (t == 1) {
      const Fq2 D = la.sqr();
      L.s[3] = D;
      L.s[4] = la * D;  // E
    } else if (t == 2) coop_embed(l, th * q.x - la * q.y, 3);
    else if (t == 3) coop_embed(l, Fq2{la.c0 * F.p.y, la.c1 * F.p.y}, 0);
    else coop_embed(l, Fq2{th.c0 * F.p.x, th.c1 * F.p.x}.neg(), 1);
  }
  __syncthreads();
  if (t < 3) {
    Fq2* N = F.T[cur ^ 1];
    const Fq2 E = L.s[4];
    if (t == 2) {
      N[2] = T[2] * E;
    } else {
      const Fq2 G = T[0] * L.s[3];
      const Fq2 H = E + T[2] * L.s[2] - G.dbl();
      if (t == 0) N[0] = L.s[1] * H;
      else N[1] = L.s[0] * (G - H) - E * T[1];
    }
  }
}

// the lines of step `si` of the prepared pairs at their G1 sides, into L.ln[1 + k]; lanes 8 + 2 k, 9 + 2 k.  No barrier.
__device__ __forceinline__ void coop_table_lines(CoopLds& L, const PvkTable* tabs, uint32_t n_tab, uint32_t si) {
  const uint32_t t = threadIdx.x;
  if (t < 8 || t >= 8 + 2 * n_tab) return;
  const uint32_t k = (t - 8) >> 1, part = (t - 8) & 1;
  if (!L.flag[1 + k]) return;
  const PvkTable* tb = tabs + k;
  const uint8_t kind = tb->kind[si];
  if (kind == LINE_ONE) return;
  const ScaledG1& P = L.sp[k];
  F12* l = &L.ln[1 + k];
  if (kind == LINE_CHORD) {
    if (part == 0) {
      const Fq2 m = tb->line[si].m;
      l->c[0] = P.ys.neg();
      coop_embed(l, Fq2{m.c0 * P.xs, m.c1 * P.xs}, 1);
    } else {
      const Fq2 c = tb->line[si].c;
      coop_embed(l, Fq2{c.c0 * P.zs, c.c1 * P.zs}, 3);
    }
  } else if (part == 0) {
    l->c[0] = P.xs;
  } else {
    const Fq2 c = tb->line[si].c;
    coop_embed(l, Fq2{c.c0 * P.zs, c.c1 * P.zs}.neg(), 2);
  }
}

// L.f <- product over the live pairs of ML(Q, P).  The caller has filled L.fly[0 .. n_fly) (q, p, live) and, for
// the prepared pairs, L.sp[k] and L.flag[1 + k] (live), behind a barrier.
__device__ __attribute__((noinline)) void coop_miller(CoopLds& L, const VkDev* vk, uint32_t n_fly, const PvkTable* tabs,
                                                      uint32_t n_tab) {
  const uint32_t t = threadIdx.x;
  if (t < n_fly) {
    CoopFly& F = L.fly[t];
    F.q1 = frob_g2(F.q, vk);
    G2Affine q2 = frob_g2(F.q1, vk);
    q2.y = q2.y.neg();
    F.q2 = q2;
    F.T[0][0] = F.q.x;
    F.T[0][1] = F.q.y;
    F.T[0][2] = Fq2::one();
  }
  if (t < 12) L.f.c[t] = t == 0 ? Fq::one() : Fq::zero();
  __syncthreads();
  const Fq2 b_twist = vk->b_twist;
  int cur = 0;  // the buffer of T every on-the-fly pair is in: they all flip together
  uint32_t si = 0;
  // step kinds: 0 doubling, 1 addition of Q, 2 addition of pi(Q), 3 addition of -pi^2(Q)
  auto step = [&](int what) {
    coop_table_lines(L, tabs, n_tab, si);
    bool synced = false;
#pragma unroll 1
    for (uint32_t p = 0; p < n_fly; ++p) {
      CoopFly& F = L.fly[p];
      if (!F.live) continue;
      if (what == 0) coop_fly_double(L, F, cur, b_twist, &L.ln[0]);
      else coop_fly_add(L, F, cur, what == 1 ? F.q : what == 2 ? F.q1 : F.q2, &L.ln[0]);
      coop_mul(L, &L.f, &L.ln[0], COOP_LINE_PROJ, 6, &L.f);
      synced = true;
    }
    if (what != 0) cur ^= 1;
    if (!synced) __syncthreads();
#pragma unroll 1
    for (uint32_t k = 0; k < n_tab; ++k) {
      if (!L.flag[1 + k]) continue;
      const uint8_t kind = tabs[k].kind[si];
      if (kind == LINE_CHORD) coop_mul(L, &L.f, &L.ln[1 + k], COOP_LINE_CHORD, 5, &L.f);
      else if (kind == LINE_VERTICAL) coop_mul(L, &L.f, &L.ln[1 + k], COOP_LINE_VERT, 3, &L.f);
    }
    ++si;
  };
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {
    coop_mul_dense(L, &L.f, &L.f, &L.f);
    step(0);
    if ((COOP_ATE_LO >> i) & 1) step(1);
  }
  step(2);
  step(3);
}

// ---- per-key preparation (one lane per point; not latency-critical) -------------------------------------------
// line() of pairing.h without the evaluation at P: the coefficients of the line through T and Q, T <- T + Q
__device__ __host__ inline void coop_line_coeffs(PvkLine* rec, uint8_t* kind, G2Affine* T, const G2Affine* Qp, bool* t_inf) {
  rec->m = Fq2::zero();
  rec->c = Fq2::zero();
  if (*t_inf) {
    *kind = LINE_ONE;
    if (Qp == T) return;
    *T = *Qp;
    *t_inf = false;
    return;
  }
  const bool same_x = T->x == Qp->x;
  if (same_x && T->y != Qp->y) {
    *kind = LINE_VERTICAL;
    rec->c = T->x;
    *t_inf = true;
    return;
  }
  Fq2 m;
  if (same_x) {
    const Fq2 x2 = T->x.sqr();
    m = (x2.dbl() + x2) * T->y.dbl().inv();
  } else {
    m = (Qp->y - T->y) * (Qp->x - T->x).inv();
  }
  const Fq2 x3 = m.sqr() - T->x - Qp->x;
  const Fq2 y3 = m * (T->x - x3) - T->y;
  *kind = LINE_CHORD;
  rec->m = m;
  rec->c = T->y - m * T->x;
  T->x = x3;
  T->y = y3;
}

__device__ __host__ inline void coop_prepare_g2(PvkTable* tb, const G2Affine* Qp, const VkDev* vk) {
  tb->inf = Qp->is_inf() ? 1u : 0u;
  tb->pad[0] = tb->pad[1] = 0;
  if (tb->inf) {
    for (uint32_t s = 0; s < COOP_STEPS; ++s) {
      tb->kind[s] = LINE_ONE;
      tb->line[s].m = Fq2::zero();
      tb->line[s].c = Fq2::zero();
    }
    return;
  }
  G2Affine T = *Qp;
  bool t_inf = false;
  uint32_t si = 0;
  for (int i = 63; i >= 0; --i) {
    coop_line_coeffs(&tb->line[si], &tb->kind[si], &T, &T, &t_inf);
    ++si;
    if ((COOP_ATE_LO >> i) & 1) {
      coop_line_coeffs(&tb->line[si], &tb->kind[si], &T, Qp, &t_inf);
      ++si;
    }
  }
  const G2Affine q1 = frob_g2(*Qp, vk);
  G2Affine q2 = frob_g2(q1, vk);
  q2.y = q2.y.neg();
  coop_line_coeffs(&tb->line[si], &tb->kind[si], &T, &q1, &t_inf);
  ++si;
  coop_line_coeffs(&tb->line[si], &tb->kind[si], &T, &q2, &t_inf);
}

// psi(B) == [6 x^2] B, the short subgroup test of the twist (ark-bn254's; eprint 2022/352 section 4.3): q - r = 6 x^2
// is a 127-bit integer, psi is frob_g2.  The point is on the twist and not at infinity.
__device__ __forceinline__ bool coop_g2_in_subgroup(const G2Affine& p, const VkDev* vk, uint64_t k_lo, uint64_t k_hi) {
  const G2XYZZ acc = mul_rho(p, k_lo, k_hi);
  if (acc.is_inf()) return false;
  const G2Affine psi = frob_g2(p, vk);
  return acc.x == psi.x * acc.zz && acc.y == psi.y * acc.zzz;
}


// pts + i * stride: a G2 point as stored.  ok[i] = canonical words, on the twist, in G2.
__global__ void __launch_bounds__(COOP_LANES) k_vp_g2(const VkDev* vk, const uint8_t* pts, uint32_t stride, uint32_t n,
                                                      uint64_t k_lo, uint64_t k_hi, uint8_t* ok) {
  const uint32_t i = blockIdx.x * COOP_LANES + threadIdx.x;
  if (i >= n) return;
  G2Affine B;
  memcpy(&B, pts + (size_t)i * stride, 128);
  bool good = fq2_words_canonical(B.x) && fq2_words_canonical(B.y);
  if (good && !B.is_inf()) good = on_curve_g2(B, vk) && coop_g2_in_subgroup(B, vk, k_lo, k_hi);
  ok[i] = good ? 1 : 0;
}

// q - r = 6 x^2 as two 64-bit words (it has 127 bits)
inline void six_x_squared(uint64_t* lo, uint64_t* hi) {
  uint32_t d[8];
  uint64_t br = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)FqParams::MOD[i] - FrParams::MOD[i] - br;
    d[i] = (uint32_t)t;
    br = (t >> 32) & 1;
  }
  *lo = (uint64_t)d[0] | ((uint64_t)d[1] << 32);
  *hi = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
}

}  // namespace
}  // namespace g16
