// gt.hip -- pairing VALUES: the library's other pairing calls answer "is this product 1?"; these hand the element of
// GT out, multiply and raise such elements, and carry them to and from the form other software reads (gt.h has the
// convention and the basis map).  All of it on the wave-cooperative arithmetic of pairing_coop.h:
//   k_gt_products   one workgroup of 64 lanes per PRODUCT (blockIdx.x): pairs off[i] .. off[i + 1], 0 to 16 of them, all
//                   on the on-the-fly line path of ONE Miller loop, then coop_final_exp; the value leaves in the flat
//                   Montgomery form.  The structural rules are k_pc_pairing's; a product with a malformed point leaves
//                   as the all-zero element with ok[i] = 0, its neighbours untouched.
//   k_vp_g2         (pairing_coop.h) the G2 tests of every pair, one lane per point, on a SECOND stream beside it
//   k_gt_mask       folds those verdicts in: a product with a bad G2 point becomes the zero element
//   k_gt_multiexp   one workgroup per output: out_i = prod_j g_ij ^ s_ij, square-and-multiply (coop_pow) in the fixed
//                   order of the input, sums in coop_mul's fixed order: the bytes depend on the input alone
//   k_gt_codec      one lane per element, both directions between the flat and the tower form
//   k_gt_member     after k_gt_multiexp with the scalar r: an element whose r-th power is not 1 is outside GT
// Per-call streams, synchronised on their own (as g16_pairing_check): other work on the card is not stalled.
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "gt.h"

namespace g16 {
namespace {

enum { T_UPLOAD = 0, T_G2, T_KERNEL, T_DOWNLOAD, T_COUNT };
thread_local PhaseTimes<T_COUNT> t_gt;

// g1: 64-byte points, g2: 128-byte points, pair p of product i is point off[i] + p of both
__global__ void __launch_bounds__(COOP_LANES) k_gt_products(const VkDev* vk, const uint8_t* g1, const uint8_t* g2,
                                                            const uint32_t* off, uint32_t n, F12* out, uint8_t* ok) {
  __shared__ CoopLds L;
  const uint32_t t = threadIdx.x, i = blockIdx.x;
  if (i >= n) return;
  const uint32_t first = off[i];
  uint32_t np = off[i + 1] - first;
  if (np > COOP_MAX_PAIRS) np = COOP_MAX_PAIRS;  // the host has refused such a call; LDS holds 16
  if (t < np) {
    G1Affine P;
    G2Affine Q;
    memcpy(&P, g1 + (size_t)(first + t) * 64, 64);
    memcpy(&Q, g2 + (size_t)(first + t) * 128, 128);
    const bool good = g1_well_formed(P);
    L.fly[t].q = Q;
    L.fly[t].p = P;
    L.fly[t].live = (good && !P.is_inf() && !Q.is_inf()) ? 1u : 0u;
    L.fly[t].pad[0] = good ? 1u : 0u;
  }
  coop_init(L);
  if (t == 0) {
    uint32_t all = 1, live = 0;
    for (uint32_t p = 0; p < np; ++p) {
      all &= L.fly[p].pad[0];
      live |= L.fly[p].live;
    }
    L.flag[0] = all;
    L.flag[1] = live;
  }
  __syncthreads();
  F12* o = out + i;
  if (!L.flag[0]) {  // block-uniform: a malformed G1 point, nothing is paired
    if (t < 12) o->c[t] = Fq::zero();
    if (t == 0) ok[i] = 0;
    return;
  }
  if (t == 0) ok[i] = 1;
  if (!L.flag[1]) {  // the empty product, or every pair has an infinite side
    if (t < 12) o->c[t] = t == 0 ? Fq::one() : Fq::zero();
    return;
  }
  coop_miller(L, vk, np, nullptr, 0);
  coop_final_exp(L, vk);
  if (t < 12) o->c[t] = L.y[0].c[t];
}

// ok[i] &= AND of g2ok[off[i] .. off[i + 1]); a product that fails becomes the zero element
__global__ void k_gt_mask(const uint32_t* off, const uint8_t* g2ok, uint32_t n, F12* out, uint8_t* ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t v = 1;
  for (uint32_t p = off[i]; p < off[i + 1]; ++p) v &= g2ok[p];
  if (v) return;
  ok[i] = 0;
#pragma unroll 1
  for (int k = 0; k < 12; ++k) out[i].c[k] = Fq::zero();
}

// out[i] = prod over j in off[i] .. off[i + 1] of g[j] ^ s[j], s[j] = the 4 x u64 at scalars + j * s_stride.
// off == NULL: group i is element i alone.  s_stride == 0: one scalar for every element (the membership test).
__global__ void __launch_bounds__(COOP_LANES) k_gt_multiexp(const F12* g, const uint64_t* scalars, uint32_t s_stride,
                                                            const uint32_t* off, uint32_t n, F12* out) {
  __shared__ CoopLds L;
  const uint32_t t = threadIdx.x, i = blockIdx.x;
  if (i >= n) return;
  const uint32_t first = off ? off[i] : i, last = off ? off[i + 1] : i + 1;
  coop_init(L);
  if (first >= last) coop_set_one(&L.f);
#pragma unroll 1
  for (uint32_t j = first; j < last; ++j) {
    if (t < 12) L.y[0].c[t] = g[j].c[t];
    __syncthreads();
    const uint64_t* e = scalars + (size_t)j * s_stride;
    if (j == first) {
      coop_pow(L, &L.f, &L.y[0], e);
    } else {
      coop_pow(L, &L.y[1], &L.y[0], e);
      coop_mul_dense(L, &L.f, &L.f, &L.y[1]);
    }
  }
  if (t < 12) out[i].c[t] = L.f.c[t];
}

// to_tower = 1: flat[i] -> tower bytes; 0: tower bytes -> flat[i] with reason[i] (0 = accepted)
__global__ void __launch_bounds__(GT_CODEC_BLOCK) k_gt_codec(int to_tower, F12* flat, uint8_t* tower, uint32_t n,
                                                             uint8_t* reason) {
  const uint32_t i = blockIdx.x * GT_CODEC_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (to_tower) {
    gt_flat_to_tower(flat[i], tower + (size_t)i * GT_BYTES);
  } else {
    F12 a;
    reason[i] = gt_tower_to_flat(tower + (size_t)i * GT_BYTES, &a);
    flat[i] = a;
  }
}

// pw[i] = flat[i]^r.  An accepted element whose power is not 1: G16_KEY_BAD_SUBGROUP and the zero element.
__global__ void __launch_bounds__(GT_CODEC_BLOCK) k_gt_member(const F12* pw, F12* flat, uint32_t n, uint8_t* reason) {
  const uint32_t i = blockIdx.x * GT_CODEC_BLOCK + threadIdx.x;
  if (i >= n || reason[i]) return;
  if (f12_is_one(pw[i])) return;
  reason[i] = G16_KEY_BAD_SUBGROUP;
#pragma unroll 1
  for (int k = 0; k < 12; ++k) flat[i].c[k] = Fq::zero();
}

enum { E_UP0 = 0, E_UP1, E_G2A, E_G2B, E_K, E_DN, E_COUNT };

// the two streams and the events of one call
struct GtCall {
  StreamBox s1, s2;
  EventBox ev[E_COUNT];
  explicit GtCall(bool second) {
    s1.create();
    if (second) s2.create();
    for (auto& e : ev) e.create(true);
  }
  void open() {
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s1.s);
    G16_HIP(hipEventRecord(ev[E_UP0].e, s1.s));
  }
  void mark(int which) { G16_HIP(hipEventRecord(ev[which].e, s1.s)); }
  // after E_DN: the one wait, then the phase times
  void finish(bool g2) {
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(s1.s));
    if (g2) G16_HIP(hipStreamSynchronize(s2.s));
    t_gt.take(Stored::REPLACE, ev, {{E_UP0, E_UP1, T_UPLOAD}, {E_UP1, E_K, T_KERNEL}, {E_K, E_DN, T_DOWNLOAD}});
    if (g2) t_gt.take(Stored::REPLACE, ev, {{E_G2A, E_G2B, T_G2}});
    else t_gt.ms[T_G2] = 0.f;  // no G2 work in this call
  }
};

void upload_consts(DevBuf<VkDev>& dvk, hipStream_t s, std::unique_ptr<VkDev>& hv) {
  hv.reset(new VkDev());
  memset((void*)hv.get(), 0, sizeof(VkDev));
  vk_consts(hv.get());
  hv->ml_alpha_beta = f12_one();
  dvk.alloc(1);
  G16_HIP(hipMemcpyAsync(dvk.p, hv.get(), sizeof(VkDev), hipMemcpyHostToDevice, s));
}

// offsets[0 .. n]: non-decreasing from 0, each group at most `most` long (0: any length); names the group on failure
bool offsets_ok(const char* fn, const uint32_t* off, uint32_t n, uint32_t most) {
  if (off[0] != 0) {
    set_create_error(std::string(fn) + ": offsets[0] is not 0");
    return false;
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (off[i + 1] < off[i]) {
      set_create_error(std::string(fn) + ": offsets decrease at " + std::to_string(i));
      return false;
    }
    if (most && off[i + 1] - off[i] > most) {
      set_create_error(std::string(fn) + ": product " + std::to_string(i) + " has " + std::to_string(off[i + 1] - off[i]) +
                       " pairs, at most " + std::to_string(most) + " fit one Miller loop");
      return false;
    }
  }
  return true;
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" g16_status g16_pairing_products(int device, const uint8_t* g1, const uint8_t* g2, const uint32_t* offsets,
                                           uint32_t n, uint8_t* gt_out, uint8_t* ok_out) {
  if (!n) return G16_OK;
  if (!offsets || !gt_out || n > 0xffffffffu / GT_BYTES) return G16_ERR_INVALID;
  if (!offsets_ok("g16_pairing_products", offsets, n, COOP_MAX_PAIRS)) return G16_ERR_INVALID;
  const uint32_t total = offsets[n];
  if (total && (!g1 || !g2)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&] {
    G16_HIP(hipSetDevice(device));
    uint64_t k_lo, k_hi;
    six_x_squared(&k_lo, &k_hi);
    std::unique_ptr<VkDev> hv;
    DevBuf<VkDev> dvk;
    DevBuf<uint8_t> d1, d2, dok, dg2ok;
    DevBuf<uint32_t> doff;
    DevBuf<F12> dout;
    GtCall c(true);
    d1.alloc((size_t)total * 64);
    d2.alloc((size_t)total * 128);
    dg2ok.alloc(total);
    doff.alloc((size_t)n + 1);
    dout.alloc(n);
    dok.alloc(n);
    std::vector<uint8_t> ok(n);
    hipStream_t s1 = c.s1.s, s2 = c.s2.s;
    c.open();
    upload_consts(dvk, s1, hv);
    if (total) {
      G16_HIP(hipMemcpyAsync(d1.p, g1, d1.bytes(), hipMemcpyHostToDevice, s1));
      G16_HIP(hipMemcpyAsync(d2.p, g2, d2.bytes(), hipMemcpyHostToDevice, s1));
    }
    G16_HIP(hipMemcpyAsync(doff.p, offsets, doff.bytes(), hipMemcpyHostToDevice, s1));
    c.mark(E_UP1);
    G16_HIP(hipStreamWaitEvent(s2, c.ev[E_UP1].e, 0));
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s2);
    G16_HIP(hipEventRecord(c.ev[E_G2A].e, s2));
    if (total)
      G16_LAUNCH(k_vp_g2, ceil_div(total, COOP_LANES), COOP_LANES, 0, s2, (const VkDev*)dvk.p, (const uint8_t*)d2.p, 128u,
                 total, k_lo, k_hi, dg2ok.p);
    G16_HIP(hipEventRecord(c.ev[E_G2B].e, s2));
    G16_LAUNCH(k_gt_products, n, COOP_LANES, 0, s1, (const VkDev*)dvk.p, (const uint8_t*)d1.p, (const uint8_t*)d2.p,
               (const uint32_t*)doff.p, n, dout.p, dok.p);
    G16_HIP(hipStreamWaitEvent(s1, c.ev[E_G2B].e, 0));
    G16_LAUNCH(k_gt_mask, ceil_div(n, 256), 256, 0, s1, (const uint32_t*)doff.p, (const uint8_t*)dg2ok.p, n, dout.p, dok.p);
    c.mark(E_K);
    G16_HIP(hipMemcpyAsync(gt_out, dout.p, dout.bytes(), hipMemcpyDeviceToHost, s1));
    G16_HIP(hipMemcpyAsync(ok.data(), dok.p, n, hipMemcpyDeviceToHost, s1));
    c.mark(E_DN);
    c.finish(true);
    if (ok_out) memcpy(ok_out, ok.data(), n);
  });
}

extern "C" g16_status g16_gt_multiexp(int device, const uint8_t* gt, const uint64_t* scalars, const uint32_t* offsets,
                                      uint32_t n, uint8_t* gt_out) {
  if (!n) return G16_OK;
  if (!offsets || !gt_out || n > 0xffffffffu / GT_BYTES) return G16_ERR_INVALID;
  if (!offsets_ok("g16_gt_multiexp", offsets, n, 0)) return G16_ERR_INVALID;
  const uint32_t total = offsets[n];
  if (total && (!gt || !scalars)) return G16_ERR_INVALID;
  for (uint32_t j = 0; j < total; ++j)
    if (!fr_words_canonical(scalars + 4 * (size_t)j)) {
      set_create_error("g16_gt_multiexp: scalar " + std::to_string(j) + " is not below r");
      return G16_ERR_INVALID;
    }
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&] {
    G16_HIP(hipSetDevice(device));
    DevBuf<F12> dg, dout;
    DevBuf<uint64_t> ds;
    DevBuf<uint32_t> doff;
    GtCall c(false);
    dg.alloc(total);
    ds.alloc((size_t)total * 4);
    doff.alloc((size_t)n + 1);
    dout.alloc(n);
    hipStream_t s1 = c.s1.s;
    c.open();
    if (total) {
      G16_HIP(hipMemcpyAsync(dg.p, gt, dg.bytes(), hipMemcpyHostToDevice, s1));
      G16_HIP(hipMemcpyAsync(ds.p, scalars, ds.bytes(), hipMemcpyHostToDevice, s1));
    }
    G16_HIP(hipMemcpyAsync(doff.p, offsets, doff.bytes(), hipMemcpyHostToDevice, s1));
    c.mark(E_UP1);
    G16_LAUNCH(k_gt_multiexp, n, COOP_LANES, 0, s1, (const F12*)dg.p, (const uint64_t*)ds.p, 4u, (const uint32_t*)doff.p, n,
               dout.p);
    c.mark(E_K);
    G16_HIP(hipMemcpyAsync(gt_out, dout.p, dout.bytes(), hipMemcpyDeviceToHost, s1));
    c.mark(E_DN);
    c.finish(false);
  });
}

extern "C" g16_status g16_gt_to_ark(int device, const uint8_t* gt, uint32_t n, uint8_t* out) {
  if (!n) return G16_OK;
  if (!gt || !out || n > 0xffffffffu / GT_BYTES) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&] {
    G16_HIP(hipSetDevice(device));
    DevBuf<F12> dflat;
    DevBuf<uint8_t> dtower;
    GtCall c(false);
    dflat.alloc(n);
    dtower.alloc((size_t)n * GT_BYTES);
    hipStream_t s1 = c.s1.s;
    c.open();
    G16_HIP(hipMemcpyAsync(dflat.p, gt, dflat.bytes(), hipMemcpyHostToDevice, s1));
    c.mark(E_UP1);
    G16_LAUNCH(k_gt_codec, ceil_div(n, GT_CODEC_BLOCK), GT_CODEC_BLOCK, 0, s1, 1, dflat.p, dtower.p, n, (uint8_t*)nullptr);
    c.mark(E_K);
    G16_HIP(hipMemcpyAsync(out, dtower.p, dtower.bytes(), hipMemcpyDeviceToHost, s1));
    c.mark(E_DN);
    c.finish(false);
  });
}

extern "C" g16_status g16_gt_from_ark(int device, const uint8_t* in, uint32_t n, int validate, uint8_t* gt_out,
                                      uint8_t* reason_out) {
  if (!n) return G16_OK;
  if (!in || !gt_out || n > 0xffffffffu / GT_BYTES) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&] {
    G16_HIP(hipSetDevice(device));
    DevBuf<F12> dflat, dpow;
    DevBuf<uint8_t> dtower, dreason;
    DevBuf<uint64_t> dr;
    GtCall c(false);
    dflat.alloc(n);
    dtower.alloc((size_t)n * GT_BYTES);
    dreason.alloc(n);
    std::vector<uint8_t> reason(n);
    uint64_t r[4];
    for (int k = 0; k < 4; ++k) r[k] = (uint64_t)FrParams::MOD[2 * k] | ((uint64_t)FrParams::MOD[2 * k + 1] << 32);
    hipStream_t s1 = c.s1.s;
    c.open();
    G16_HIP(hipMemcpyAsync(dtower.p, in, dtower.bytes(), hipMemcpyHostToDevice, s1));
    if (validate) {
      dpow.alloc(n);
      dr.alloc(4);
      G16_HIP(hipMemcpyAsync(dr.p, r, sizeof r, hipMemcpyHostToDevice, s1));
    }
    c.mark(E_UP1);
    G16_LAUNCH(k_gt_codec, ceil_div(n, GT_CODEC_BLOCK), GT_CODEC_BLOCK, 0, s1, 0, dflat.p, dtower.p, n, dreason.p);
    if (validate) {
      G16_LAUNCH(k_gt_multiexp, n, COOP_LANES, 0, s1, (const F12*)dflat.p, (const uint64_t*)dr.p, 0u,
                 (const uint32_t*)nullptr, n, dpow.p);
      G16_LAUNCH(k_gt_member, ceil_div(n, GT_CODEC_BLOCK), GT_CODEC_BLOCK, 0, s1, (const F12*)dpow.p, dflat.p, n, dreason.p);
    }
    c.mark(E_K);
    G16_HIP(hipMemcpyAsync(gt_out, dflat.p, dflat.bytes(), hipMemcpyDeviceToHost, s1));
    G16_HIP(hipMemcpyAsync(reason.data(), dreason.p, n, hipMemcpyDeviceToHost, s1));
    c.mark(E_DN);
    c.finish(false);
    if (reason_out) memcpy(reason_out, reason.data(), n);
  });
}

extern "C" g16_status g16_gt_times(float* ms, uint32_t cap) {
  return t_gt.read(ms, cap);
}
