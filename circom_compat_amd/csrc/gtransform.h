// gtransform.h -- the group transform that setup_srs.hip (g16_setup_from_srs) and srs_prepare.hip (g16_srs_prepare)
// share: the inverse radix-2 transform of an array of curve points (the Lagrange basis of a powers-of-tau string), its
// twiddle schedules, and the batched conversion back to affine.  One copy, included by both files, the way keycheck.h
// is shared.  Everything on the lazy limbs of field29.h / ec29.h; all kernels one wave per block, no atomics: the
// results are group elements, the bytes do not depend on any order.
//   k_naf         a scalar (twiddle) -> its non-adjacent form, two 256-bit masks, once per transform size
//   k_gntt_stage  one DIF butterfly per lane, (P, Q) -> (P + Q, w^j (P - Q)), points resident as XYZZ.  The
//                 product is a 255-step double-and-add over the NAF (254 doublings, ~85 additions).  Stages
//                 with >= 64 blocks index j-major: a whole wave shares j, hence the digit schedule.
//   k_scale       the upper half of the first stage times 1/n (the lower half has it in its twiddle): n/2
//                 products instead of n; no output of a DIF passes through a twiddle on every path.
//   k_affine      XYZZ -> canonical affine, one Fermat inversion per SS_RUN points (Montgomery's trick), with the
//                 bit reversal of the transform's output folded into the store
#pragma once
#include "ec29.h"
#include "hostcall.h"
#include "keygen.h"
#include "ntt.h"

namespace g16 {
namespace {

constexpr uint32_t SS_BLOCK = 64;      // lanes per block: one wave
constexpr uint32_t SS_RUN = 4;         // points per lane of k_affine: one inversion per SS_RUN points

// k = sum (pos_i - neg_i) 2^i, non-adjacent.  Digit i is bit i+1 of 3k minus bit i+1 of k; k < r < 2^254, so 3k
// fits 256 bits and the leading digit is at most bit 254.
struct Naf {
  uint32_t pos[8], neg[8];
};

G16_HD Naf naf_of(const U256& k) {
  uint32_t p[8], q[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += 3ull * k.v[i];
    const uint32_t h = (uint32_t)c;
    c >>= 32;
    p[i] = h & ~k.v[i];
    q[i] = k.v[i] & ~h;
  }
  Naf r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r.pos[i] = (p[i] >> 1) | (i < 7 ? p[i + 1] << 31 : 0u);
    r.neg[i] = (q[i] >> 1) | (i < 7 ? q[i + 1] << 31 : 0u);
  }
  return r;
}

__global__ void __launch_bounds__(256) k_naf(const Fr* sc, uint32_t n, Naf* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = naf_of(sc[i].to_canonical());
}

template <class LF>
__device__ __forceinline__ Aff29<LF> aff_neg(const Aff29<LF>& p) {
  return Aff29<LF>{p.x, p.y.neg().carry(), p.inf};
}

// s D for a point held as XYZZ: full additions (12M + 2S), D is not affine
template <class LF>
__device__ __forceinline__ XYZZ29<LF> mul_naf(const XYZZ29<LF>& D, const Naf* s) {
  XYZZ29<LF> acc = XYZZ29<LF>::infinity();
  if (D.is_inf()) return acc;
  const LF ny = D.y.neg().carry();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    const uint32_t pw = s->pos[w], nw = s->neg[w];
    if (!(pw | nw) && acc.is_inf()) continue;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc.dbl_in_place();
      const uint32_t m = 1u << b;
      if ((pw | nw) & m) acc.add(XYZZ29<LF>{D.x, (nw & m) ? ny : D.y, D.zz, D.zzz});
    }
  }
  return acc;
}

// ---- group transform ---------------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(SS_BLOCK) k_load_affine(const Affine<F>* in, uint32_t n,
                                                          XYZZ29<typename Lazy<F>::type>* out) {
  const uint32_t i = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = XYZZ29<typename Lazy<F>::type>::from_affine(affine_from_mont256<F>(in[i]));
}

// pair t of the stage with half-size 2^hl in a transform of 2 * npairs points; 2^nbl = blocks of the stage =
// stride of j in the twiddle table tw[e] = NAF(omega^-e), e < npairs
template <class LF>
__global__ void __launch_bounds__(SS_BLOCK) k_gntt_stage(XYZZ29<LF>* a, uint32_t npairs, uint32_t hl, uint32_t nbl,
                                                         uint32_t jmajor, const Naf* tw) {
  const uint32_t t = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (t >= npairs) return;
  uint32_t b, j;
  if (jmajor) {
    j = t >> nbl;
    b = t & ((1u << nbl) - 1u);
  } else {
    b = t >> hl;
    j = t & ((1u << hl) - 1u);
  }
  const size_t i0 = ((size_t)b << (hl + 1)) + j, i1 = i0 + ((size_t)1 << hl);
  const XYZZ29<LF> P = a[i0], Q = a[i1];
  XYZZ29<LF> S = P, D = P;
  S.add(Q);
  D.add(Q.neg());
  a[i0] = S;
  a[i1] = mul_naf(D, tw + ((size_t)j << nbl));
}

template <class LF>
__global__ void __launch_bounds__(SS_BLOCK) k_scale(XYZZ29<LF>* a, uint32_t n, const Naf* s) {
  const uint32_t i = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (i >= n) return;
  a[i] = mul_naf(a[i], s);
}

// lane t of block g owns the points g * SS_BLOCK * SS_RUN + r * SS_BLOCK + t, r < SS_RUN.  Prefix products of the
// ZZZ down the run (an infinite point counts as 1), one inversion, then back up: 1/ZZZ_r = inv(prefix_r ZZZ_r)
// prefix_r, 1/ZZ = (ZZ / ZZZ)^2.  brev_bits >= 0: entry i of work is entry bitrev(i) of the output.
// PACKED: the internal form load_packed_affine reads (the bases of the combinations); else the zkey encoding.
template <class F, bool PACKED>
__global__ void __launch_bounds__(SS_BLOCK) k_affine(const XYZZ29<typename Lazy<F>::type>* work, uint32_t n,
                                                     int brev_bits, Affine<F>* out) {
  using LF = typename Lazy<F>::type;
  const uint32_t first = blockIdx.x * (SS_BLOCK * SS_RUN) + threadIdx.x;
  LF pre[SS_RUN];
  LF run = LF::one();
#pragma unroll
  for (uint32_t r = 0; r < SS_RUN; ++r) {
    const uint32_t i = first + r * SS_BLOCK;
    pre[r] = run;
    if (i < n && !work[i].is_inf()) run = run * work[i].zzz;
  }
  LF inv = f29_inv(run);
#pragma unroll
  for (int r = SS_RUN - 1; r >= 0; --r) {
    const uint32_t i = first + (uint32_t)r * SS_BLOCK;
    if (i >= n) continue;
    const uint32_t dst = brev_bits > 0 ? __brev(i) >> (32 - brev_bits) : i;
    const XYZZ29<LF> P = work[i];
    if (P.is_inf()) {
      out[dst] = Affine<F>::infinity();
      continue;
    }
    const LF iz3 = inv * pre[r];
    inv = inv * P.zzz;
    const LF iz2 = (iz3 * P.zz).sqr();
    const LF x = P.x * iz2, y = P.y * iz3;
    if (PACKED) {
      out[dst] = store_packed_affine<F>(Aff29<LF>{x, y, false});
    } else {
      out[dst] = Affine<F>{x.to_mont256(), y.to_mont256()};
    }
  }
}

struct Twiddles {  // of one transform size n = 2^k
  DevBuf<Naf> tw, tw_scaled, top, h;  // omega_n^-e | omega_n^-e / n, e < n/2 | 1/n | omega_2n^-j / (2n), j < n
};

void naf_table(const Fr& base, const Fr& scale, uint32_t count, Fr* tmp, DevBuf<Naf>& out, hipStream_t s) {
  out.alloc(count ? count : 1);
  if (!count) return;
  fr_powers(base, scale, tmp, count, count, s);
  G16_LAUNCH(k_naf, ceil_div(count, 256), 256, 0, s, (const Fr*)tmp, count, out.p);
}

// in place: natural order in, bit-reversed out; scaled: times 1/n
template <class LF>
void group_intt(XYZZ29<LF>* a, int k, const Twiddles& T, bool scaled, hipStream_t s) {
  const uint32_t npairs = k ? 1u << (k - 1) : 0;
  for (int st = 0; st < k; ++st) {
    const uint32_t hl = (uint32_t)(k - 1 - st), nbl = (uint32_t)st;
    const Naf* tw = (st == 0 && scaled) ? T.tw_scaled.p : T.tw.p;
    G16_LAUNCH((k_gntt_stage<LF>), ceil_div(npairs, SS_BLOCK), SS_BLOCK, 0, s, a, npairs, hl, nbl,
               (uint32_t)(nbl >= 6 ? 1 : 0), tw);
    if (st == 0 && scaled)
      G16_LAUNCH((k_scale<LF>), ceil_div(npairs, SS_BLOCK), SS_BLOCK, 0, s, a, npairs, (const Naf*)T.top.p);
  }
}

template <class F, bool PACKED>
void to_affine(const XYZZ29<typename Lazy<F>::type>* work, uint32_t n, int brev_bits, Affine<F>* out, hipStream_t s) {
  if (n) G16_LAUNCH((k_affine<F, PACKED>), ceil_div(n, SS_BLOCK * SS_RUN), SS_BLOCK, 0, s, work, n, brev_bits, out);
}

// the schedules of one transform size n = 2^k; tmp holds max(n / 2, with_h ? n : 1) scalars
void build_twiddles(Twiddles& T, int k, bool with_h, Fr* tmp, hipStream_t s) {
  const uint32_t n = 1u << k;
  const Fr winv = fr_root_of_unity(k).inv(), ninv = Fr::from_u32(n).inv();
  naf_table(winv, Fr::one(), n / 2, tmp, T.tw, s);
  naf_table(winv, ninv, n / 2, tmp, T.tw_scaled, s);
  naf_table(Fr::one(), ninv, 1, tmp, T.top, s);
  if (with_h) naf_table(fr_root_of_unity(k + 1).inv(), Fr::from_u32(2 * n).inv(), n, tmp, T.h, s);
  G16_HIP(hipStreamSynchronize(s));
}

template <class T>
void fetch(std::vector<uint8_t>& dst, const T* dev, size_t count) {
  dst.resize(count ? count * sizeof(T) : 1);
  if (count) G16_HIP(hipMemcpy(dst.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
}

}  // namespace
}  // namespace g16
