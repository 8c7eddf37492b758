// verify_prepared.hip -- low-latency Groth16 verification: a PREPARED verifying key (g16_pvk, what
// Groth16::process_vk returns) and verify_with_processed_vk on the wave-cooperative pairing of pairing_coop.h.
// verify.hip checks a proof in ONE lane (a throughput kernel); here ONE WORKGROUP of 64 lanes checks a proof:
//   k_pvk_prepare   once per key, one lane per job: the Miller value of (beta, -alpha) with pairing.h's loop, and the
//                   line coefficients of gamma and of delta for every step of the loop (PvkTable)
//   k_vp_inputs     one workgroup per proof: X = IC_0 + sum_j pub_j IC_{j+1}, one lane per term (striding past 64), a
//                   fixed LDS tree; -X leaves PROJECTIVE (ScaledG1): the Fq factor vanishes in the final exponentiation
//   k_vp_g2         (pairing_coop.h: gt.hip launches it too) one lane per G2 point, on a SECOND STREAM beside the other two: every word canonical, the point
//                   on the twist, and psi(B) = [6 x^2] B (a 127-bit ladder instead of the 254 bits of [r] B)
//   k_vp_pairing    one workgroup per proof: the tests of A and C, then ONE Miller loop for the three pairs
//                   (A, B) on the fly, (-X, gamma) and (-C, delta) from the tables, times the stored (beta, -alpha)
//                   value, and the final exponentiation
//   k_pc_pairing    g16_pairing_check: up to 16 pairs, all on the fly, one workgroup
//   k_vp_and        verdict = pairing AND the G2 tests
//   k_vp_inputs_affine / k_vp_inputs_given   prepare_inputs (X normalised) and verify_prepared_inputs (X given)
// A call uses the handle's two streams and synchronises those, not the device.
#include <stdlib.h>

#include <memory>
#include <mutex>

#include "pairing_coop.h"

namespace g16 {
namespace {

enum { T_UPLOAD = 0, T_INPUTS, T_G2, T_PAIRING, T_DOWNLOAD, T_PREPARE, T_COUNT };
thread_local PhaseTimes<T_COUNT> t_phase;

// block 0: ML(beta, -alpha); block 1: gamma's table; block 2: delta's
__global__ void k_pvk_prepare(VkDev* vk, PvkTable* tabs) {
  if (threadIdx.x != 0) return;
  if (blockIdx.x == 0) {
    F12 f = f12_one();
    miller_mul(&f, &vk->beta, &vk->alpha_neg, vk);
    vk->ml_alpha_beta = f;
  } else if (blockIdx.x <= 2) {
    coop_prepare_g2(&tabs[blockIdx.x - 1], blockIdx.x == 1 ? &vk->gamma : &vk->delta, vk);
  }
}

__global__ void __launch_bounds__(COOP_LANES) k_vp_inputs(const G1Affine* ic, uint32_t n_pub, const Fr* pubs, uint32_t n,
                                                          ScaledG1* xs) {
  __shared__ G1XYZZ sh[COOP_LANES];
  const uint32_t t = threadIdx.x, i = blockIdx.x;
  if (i >= n) return;
  G1XYZZ acc = G1XYZZ::infinity();
  if (t == 0) acc = G1XYZZ::from_affine(ic[0]);
#pragma unroll 1
  for (uint32_t j = t; j < n_pub; j += COOP_LANES) {
    const U256 s = pubs[(size_t)i * n_pub + j].to_canonical();
    acc.add(G1XYZZ::from_affine(ic[j + 1]).mul(s));
  }
  kc_block_sum(sh, acc);
  if (t == 0) {
    const G1XYZZ X = sh[0];
    ScaledG1 o;
    o.inf = X.is_inf() ? 1u : 0u;
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    // (x, y) = (X / ZZ, Y / ZZZ), scaled by ZZ ZZZ; y negated: the pair is (-X, gamma)
    o.xs = X.x * X.zzz;
    o.ys = (X.y * X.zz).neg();
    o.zs = X.zz * X.zzz;
    xs[i] = o;
  }
}

// prepare_inputs: k_vp_inputs' sum NORMALISED, X as a packed affine point (one inversion per proof; all-zero = infinity)
__global__ void k_vp_inputs_affine(const ScaledG1* xs, uint32_t n, G1Affine* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ScaledG1 s = xs[i];
  G1Affine p;
  if (s.inf) {
    p.x = Fq::zero();
    p.y = Fq::zero();
  } else {
    const Fq zi = s.zs.inv();
    p.x = s.xs * zi;
    p.y = (s.ys * zi).neg();
  }
  out[i] = p;
}

// verify_prepared_inputs: the caller's X, tested like a proof's point, as the G1 side of (-X, gamma).  A malformed X
// leaves as infinity (its pair is skipped) with good[i] = 0: that proof alone is refused.
__global__ void k_vp_inputs_given(const G1Affine* pts, uint32_t n, ScaledG1* xs, uint8_t* good) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Affine X = pts[i];
  const bool ok = g1_well_formed(X);
  ScaledG1 o;
  o.xs = X.x;
  o.ys = X.y.neg();
  o.zs = Fq::one();
  o.inf = (!ok || X.is_inf()) ? 1u : 0u;
  o.pad[0] = o.pad[1] = o.pad[2] = 0;
  xs[i] = o;
  good[i] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(COOP_LANES) k_vp_pairing(const VkDev* vk, const PvkTable* tabs, const uint8_t* proofs,
                                                           const ScaledG1* xs, uint32_t n, uint8_t* ok) {
  __shared__ CoopLds L;
  const uint32_t t = threadIdx.x, i = blockIdx.x;
  if (i >= n) return;
  const uint8_t* rec = proofs + (size_t)i * G16_PROOF_BYTES;
  if (t == 0) {  // A, and B as it comes: k_vp_g2 judges B
    G1Affine A;
    G2Affine B;
    memcpy(&A, rec, 64);
    memcpy(&B, rec + 64, 128);
    const bool good = g1_well_formed(A);
    L.fly[0].q = B;
    L.fly[0].p = A;
    L.fly[0].live = (good && !A.is_inf() && !B.is_inf()) ? 1u : 0u;
    L.flag[0] = good ? 1u : 0u;
    L.sp[0] = xs[i];
    L.flag[1] = (!tabs[0].inf && !L.sp[0].inf) ? 1u : 0u;
  } else if (t == 1) {
    G1Affine C;
    memcpy(&C, rec + 192, 64);
    const bool good = g1_well_formed(C);
    ScaledG1 o;
    o.xs = C.x;
    o.ys = C.y.neg();
    o.zs = Fq::one();
    o.inf = C.is_inf() ? 1u : 0u;
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    L.sp[1] = o;
    L.flag[2] = (good && !tabs[1].inf && !o.inf) ? 1u : 0u;
    L.flag[3] = good ? 1u : 0u;
  }
  coop_init(L);
  if (!(L.flag[0] && L.flag[3])) {  // block-uniform: a malformed proof is never paired
    if (t == 0) ok[i] = 0;
    return;
  }
  coop_miller(L, vk, 1, tabs, 2);
  if (t < 12) L.y[0].c[t] = vk->ml_alpha_beta.c[t];
  __syncthreads();
  coop_mul_dense(L, &L.f, &L.f, &L.y[0]);
  const bool one = coop_final_exp_is_one(L, vk);
  if (t == 0) ok[i] = one ? 1 : 0;
}

// g1: n x 64, g2: n x 128; *ok = all G1 points well formed AND the product of the pairings is 1
__global__ void __launch_bounds__(COOP_LANES) k_pc_pairing(const VkDev* vk, const uint8_t* g1, const uint8_t* g2,
                                                           uint32_t n, uint8_t* ok) {
  __shared__ CoopLds L;
  const uint32_t t = threadIdx.x;
  if (t < n) {
    G1Affine P;
    G2Affine Q;
    memcpy(&P, g1 + (size_t)t * 64, 64);
    memcpy(&Q, g2 + (size_t)t * 128, 128);
    const bool good = g1_well_formed(P);
    L.fly[t].q = Q;
    L.fly[t].p = P;
    L.fly[t].live = (good && !P.is_inf() && !Q.is_inf()) ? 1u : 0u;
    L.fly[t].pad[0] = good ? 1u : 0u;
  }
  coop_init(L);
  if (t == 0) {
    uint32_t all = 1;
    for (uint32_t p = 0; p < n; ++p) all &= L.fly[p].pad[0];
    L.flag[0] = all;
  }
  __syncthreads();
  if (!L.flag[0]) {
    if (t == 0) *ok = 0;
    return;
  }
  coop_miller(L, vk, n, nullptr, 0);
  const bool one = coop_final_exp_is_one(L, vk);
  if (t == 0) *ok = one ? 1 : 0;
}

// ok[i] &= g2ok[i]   (all = 0), or ok[0] &= AND of g2ok[0 .. m)   (all = 1, one lane)
__global__ void k_vp_and(uint8_t* ok, const uint8_t* g2ok, uint32_t n, uint32_t m, int all) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (all) {
    if (i != 0) return;
    uint8_t v = ok[0];
    for (uint32_t k = 0; k < m; ++k) v &= g2ok[k];
    ok[0] = v;
    return;
  }
  if (i < n) ok[i] &= g2ok[i];
}

// a buffer that only grows: releasing device memory waits for the whole device
template <class T>
struct GrowBuf {
  DevBuf<T> d;
  void need(size_t count) {
    if (count > d.n) d.alloc(count + count / 2);
  }
};
struct GrowPinned {
  uint8_t* p = nullptr;
  size_t n = 0;
  ~GrowPinned() {
    if (p) (void)hipHostFree(p);
  }
  void need(size_t bytes) {
    if (bytes <= n) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    G16_HIP(hipHostMalloc((void**)&p, bytes + bytes / 2, hipHostMallocPortable));
    n = bytes + bytes / 2;
  }
};

void fill_consts(VkDev* hv) {
  vk_consts(hv);
  hv->ml_alpha_beta = f12_one();
}

const char* reason_of(uint8_t flag) {
  return flag == G16_KEY_BAD_NONCANONICAL ? "non-canonical coordinate"
         : flag == G16_KEY_BAD_OFF_CURVE  ? "off the curve"
                                          : "outside the prime-order subgroup";
}

enum { E_UP0 = 0, E_UP1, E_IN, E_G2A, E_G2B, E_PAIR, E_DN0, E_DN1, E_COUNT };

}  // namespace
}  // namespace g16

using namespace g16;

struct g16_pvk {
  int device = 0;
  uint32_t n_pub = 0;
  std::mutex mu;
  DevBuf<VkDev> dvk;
  DevBuf<PvkTable> dtab;
  DevBuf<G1Affine> dic;
  F12 ml_alpha_beta;
  uint8_t alpha[64], beta[128];   // as given: what g16_pvk_alpha_g1_beta_g2 pairs on first use
  uint8_t gt_alpha_beta[384];
  bool gt_made = false;
  uint64_t k_lo = 0, k_hi = 0;
  StreamBox s1, s2;
  EventBox ev[E_COUNT];
  GrowPinned pin;
  GrowBuf<uint8_t> dproofs, dok, dg2ok, dxok;
  GrowBuf<Fr> dpub;
  GrowBuf<ScaledG1> dxs;
};

extern "C" g16_status g16_pvk_create(int device, const g16_vk_desc* vk, g16_pvk** out) {
  if (out) *out = nullptr;
  if (!vk || !out || !vk->ic || vk->ic_count < 1) {
    set_create_error("g16_pvk_create: a NULL argument or a key without gamma_abc_g1");
    return G16_ERR_INVALID;
  }
  const g16_status ds = device_ok(device);
  if (ds == G16_ERR_NO_DEVICE) return ds;
  if (ds != G16_OK) {
    set_create_error("g16_pvk_create: device out of range");
    return G16_ERR_INVALID;
  }
  return guarded_call([&]() -> g16_status {
    std::unique_ptr<VkDev> hv(new VkDev());
    fill_consts(hv.get());
    G1Affine alpha;
    memcpy(&alpha, vk->alpha_g1, 64);
    memcpy(&hv->beta, vk->beta_g2, 128);
    memcpy(&hv->gamma, vk->gamma_g2, 128);
    memcpy(&hv->delta, vk->delta_g2, 128);
    // the key is tested, unlike g16_verify_batch's: once per key, on the host (the field classes compile for it)
    auto refuse = [](const std::string& point, uint8_t flag) {
      set_create_error("g16_pvk_create: " + point + ": " + reason_of(flag));
      return G16_ERR_INVALID;
    };
    uint8_t fl = g1_flag(alpha);
    if (fl & ~KC_INF) return refuse("alpha_g1", fl);
    const char* g2_names[3] = {"beta_g2", "gamma_g2", "delta_g2"};
    const G2Affine* g2_pts[3] = {&hv->beta, &hv->gamma, &hv->delta};
    for (int k = 0; k < 3; ++k) {
      fl = g2_flag(*g2_pts[k], hv.get());
      if (fl & ~KC_INF) return refuse(g2_names[k], fl);
    }
    std::vector<G1Affine> ic(vk->ic_count);
    memcpy(ic.data(), vk->ic, (size_t)vk->ic_count * 64);
    for (uint32_t j = 0; j < vk->ic_count; ++j) {
      fl = g1_flag(ic[j]);
      if (fl & ~KC_INF) return refuse("gamma_abc_g1[" + std::to_string(j) + "]", fl);
    }
    hv->alpha_neg = alpha.neg();

    G16_HIP(hipSetDevice(device));
    std::unique_ptr<g16_pvk> h(new g16_pvk());
    h->device = device;
    h->n_pub = vk->ic_count - 1;
    memcpy(h->alpha, vk->alpha_g1, 64);
    memcpy(h->beta, vk->beta_g2, 128);
    six_x_squared(&h->k_lo, &h->k_hi);
    h->dvk.alloc(1);
    h->dtab.alloc(2);
    h->dic.alloc(vk->ic_count);
    h->s1.create();
    h->s2.create();
    for (auto& e : h->ev) e.create(true);
    hipStream_t s = h->s1.s;
    G16_HIP(hipMemcpyAsync(h->dvk.p, hv.get(), sizeof(VkDev), hipMemcpyHostToDevice, s));
    G16_HIP(hipMemcpyAsync(h->dic.p, ic.data(), h->dic.bytes(), hipMemcpyHostToDevice, s));
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s);
    G16_HIP(hipEventRecord(h->ev[E_UP0].e, s));
    G16_LAUNCH(k_pvk_prepare, 3, 1, 0, s, h->dvk.p, h->dtab.p);
    G16_HIP(hipEventRecord(h->ev[E_UP1].e, s));
    G16_HIP(hipMemcpyAsync(&h->ml_alpha_beta, &h->dvk.p->ml_alpha_beta, sizeof(F12), hipMemcpyDeviceToHost, s));
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(s));
    t_phase.take(Stored::REPLACE, h->ev, {{E_UP0, E_UP1, T_PREPARE}});
    *out = h.release();
    return G16_OK;
  });
}

extern "C" void g16_pvk_destroy(g16_pvk* pvk) {
  if (!pvk) return;
  (void)hipSetDevice(pvk->device);
  delete pvk;
}

extern "C" g16_status g16_pvk_alpha_beta(const g16_pvk* pvk, uint8_t out[384]) {
  if (!pvk || !out) return G16_ERR_INVALID;
  memcpy(out, &pvk->ml_alpha_beta, sizeof(F12));  // already the w-basis: the kernels use no other
  return G16_OK;
}

// g16_verify_prepared (prepared == NULL: X from public_inputs by k_vp_inputs) and g16_verify_prepared_inputs (X given:
// n x 64 bytes, the input ladder is skipped)
static g16_status verify_prepared_run(g16_pvk* h, const uint8_t* proofs, const uint64_t* public_inputs,
                                      const uint8_t* prepared, uint32_t n, uint8_t* ok_out) {
  if (!h || (n && (!proofs || !ok_out))) return G16_ERR_INVALID;
  const uint32_t n_pub = prepared ? 2 : h->n_pub;   // words of 32 bytes per proof in the input block
  if (n && n_pub && !public_inputs && !prepared) return G16_ERR_INVALID;
  if ((uint64_t)n * n_pub > 0xffffffffull / 32 || n > 0xffffffffu / G16_PROOF_BYTES) return G16_ERR_INVALID;
  if (!n) return G16_OK;
  std::lock_guard<std::mutex> guard(h->mu);
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(h->device));
    const size_t pbytes = (size_t)n * G16_PROOF_BYTES, ibytes = (size_t)n * n_pub * 32;
    if (prepared) h->dxok.need(n);
    h->pin.need(pbytes + ibytes + n);
    h->dproofs.need(pbytes);
    h->dpub.need((size_t)n * n_pub + 1);
    h->dok.need(n);
    h->dg2ok.need(n);
    h->dxs.need(n);
    hipStream_t s1 = h->s1.s, s2 = h->s2.s;
    auto* ev = h->ev;
    uint8_t* pin_ok = h->pin.p + pbytes + ibytes;
    memcpy(h->pin.p, proofs, pbytes);
    if (ibytes) memcpy(h->pin.p + pbytes, prepared ? (const void*)prepared : (const void*)public_inputs, ibytes);

    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s1);
    G16_HIP(hipEventRecord(ev[E_UP0].e, s1));
    G16_HIP(hipMemcpyAsync(h->dproofs.d.p, h->pin.p, pbytes, hipMemcpyHostToDevice, s1));
    if (ibytes) G16_HIP(hipMemcpyAsync(h->dpub.d.p, h->pin.p + pbytes, ibytes, hipMemcpyHostToDevice, s1));
    G16_HIP(hipEventRecord(ev[E_UP1].e, s1));

    // the tests of B on the second stream, beside the inputs and the pairing
    G16_HIP(hipStreamWaitEvent(s2, ev[E_UP1].e, 0));
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s2);
    G16_HIP(hipEventRecord(ev[E_G2A].e, s2));
    G16_LAUNCH(k_vp_g2, ceil_div(n, COOP_LANES), COOP_LANES, 0, s2, (const VkDev*)h->dvk.p,
               (const uint8_t*)h->dproofs.d.p + 64, (uint32_t)G16_PROOF_BYTES, n, h->k_lo, h->k_hi, h->dg2ok.d.p);
    G16_HIP(hipEventRecord(ev[E_G2B].e, s2));

    if (prepared)
      G16_LAUNCH(k_vp_inputs_given, ceil_div(n, 256), 256, 0, s1, (const G1Affine*)h->dpub.d.p, n, h->dxs.d.p,
                 h->dxok.d.p);
    else
      G16_LAUNCH(k_vp_inputs, n, COOP_LANES, 0, s1, (const G1Affine*)h->dic.p, n_pub, (const Fr*)h->dpub.d.p, n,
                 h->dxs.d.p);
    G16_HIP(hipEventRecord(ev[E_IN].e, s1));
    G16_LAUNCH(k_vp_pairing, n, COOP_LANES, 0, s1, (const VkDev*)h->dvk.p, (const PvkTable*)h->dtab.p,
               (const uint8_t*)h->dproofs.d.p, (const ScaledG1*)h->dxs.d.p, n, h->dok.d.p);
    G16_HIP(hipEventRecord(ev[E_PAIR].e, s1));
    G16_HIP(hipStreamWaitEvent(s1, ev[E_G2B].e, 0));
    G16_LAUNCH(k_vp_and, ceil_div(n, 256), 256, 0, s1, h->dok.d.p, (const uint8_t*)h->dg2ok.d.p, n, n, 0);
    if (prepared) G16_LAUNCH(k_vp_and, ceil_div(n, 256), 256, 0, s1, h->dok.d.p, (const uint8_t*)h->dxok.d.p, n, n, 0);
    G16_HIP(hipEventRecord(ev[E_DN0].e, s1));
    G16_HIP(hipMemcpyAsync(pin_ok, h->dok.d.p, n, hipMemcpyDeviceToHost, s1));
    G16_HIP(hipEventRecord(ev[E_DN1].e, s1));
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(s1));
    G16_HIP(hipStreamSynchronize(s2));
    memcpy(ok_out, pin_ok, n);

    t_phase.take(Stored::REPLACE, ev,  // T_PREPARE stays: it is g16_pvk_create's
                 {{E_UP0, E_UP1, T_UPLOAD}, {E_UP1, E_IN, T_INPUTS}, {E_G2A, E_G2B, T_G2},
                  {E_IN, E_PAIR, T_PAIRING}, {E_DN0, E_DN1, T_DOWNLOAD}});
    return G16_OK;
  });
}

extern "C" g16_status g16_verify_prepared(g16_pvk* h, const uint8_t* proofs, const uint64_t* public_inputs,
                                          uint32_t n, uint8_t* ok_out) {
  return verify_prepared_run(h, proofs, public_inputs, nullptr, n, ok_out);
}

extern "C" g16_status g16_verify_prepared_inputs(g16_pvk* h, const uint8_t* proofs, const uint8_t* prepared, uint32_t n,
                                                 uint8_t* ok_out) {
  if (n && !prepared) return G16_ERR_INVALID;
  return verify_prepared_run(h, proofs, nullptr, n ? prepared : nullptr, n, ok_out);
}

extern "C" g16_status g16_pvk_prepare_inputs(g16_pvk* h, const uint64_t* public_inputs, uint32_t n, uint8_t* out) {
  if (!h || (n && !out)) return G16_ERR_INVALID;
  const uint32_t n_pub = h->n_pub;
  if (n && n_pub && !public_inputs) return G16_ERR_INVALID;
  if ((uint64_t)n * n_pub > 0xffffffffull / 32 || n > 0xffffffffu / 64) return G16_ERR_INVALID;
  if (!n) return G16_OK;
  std::lock_guard<std::mutex> guard(h->mu);
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(h->device));
    const size_t ibytes = (size_t)n * n_pub * 32;
    h->dpub.need((size_t)n * n_pub + 1);
    h->dxs.need(n);
    h->dproofs.need((size_t)n * 64);   // the normalised points leave through the proof buffer
    hipStream_t s1 = h->s1.s;
    if (ibytes) G16_HIP(hipMemcpyAsync(h->dpub.d.p, public_inputs, ibytes, hipMemcpyHostToDevice, s1));
    G16_LAUNCH(k_vp_inputs, n, COOP_LANES, 0, s1, (const G1Affine*)h->dic.p, n_pub, (const Fr*)h->dpub.d.p, n,
               h->dxs.d.p);
    G16_LAUNCH(k_vp_inputs_affine, ceil_div(n, 64), 64, 0, s1, (const ScaledG1*)h->dxs.d.p, n,
               (G1Affine*)h->dproofs.d.p);
    G16_HIP(hipMemcpyAsync(out, h->dproofs.d.p, (size_t)n * 64, hipMemcpyDeviceToHost, s1));
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(s1));
    return G16_OK;
  });
}

extern "C" g16_status g16_pvk_alpha_g1_beta_g2(const g16_pvk* pvk, uint8_t out[384]) {
  if (!pvk || !out) return G16_ERR_INVALID;
  g16_pvk* h = const_cast<g16_pvk*>(pvk);   // the cache is not part of the key
  std::lock_guard<std::mutex> guard(h->mu);
  if (!h->gt_made) {  // first use: one product of one pair, (alpha, beta) as the key gave them
    const uint32_t off[2] = {0, 1};
    uint8_t ok = 0;
    const g16_status st = g16_pairing_products(h->device, h->alpha, h->beta, off, 1, h->gt_alpha_beta, &ok);
    if (st != G16_OK) return st;
    if (!ok) return G16_ERR_INTERNAL;  // g16_pvk_create has tested both points
    h->gt_made = true;
  }
  memcpy(out, h->gt_alpha_beta, 384);
  return G16_OK;
}

extern "C" g16_status g16_pairing_check(int device, const uint8_t* g1, const uint8_t* g2, uint32_t n_pairs,
                                        uint8_t* ok_out) {
  if (!g1 || !g2 || !ok_out || n_pairs < 1 || n_pairs > COOP_MAX_PAIRS) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    std::unique_ptr<VkDev> hv(new VkDev());
    memset((void*)hv.get(), 0, sizeof(VkDev));
    fill_consts(hv.get());
    uint64_t k_lo, k_hi;
    six_x_squared(&k_lo, &k_hi);
    DevBuf<VkDev> dvk;
    DevBuf<uint8_t> d1, d2, dok, dg2ok;
    StreamBox s1, s2;
    EventBox up, done;
    dvk.alloc(1);
    d1.alloc((size_t)n_pairs * 64);
    d2.alloc((size_t)n_pairs * 128);
    dok.alloc(1);
    dg2ok.alloc(n_pairs);
    s1.create();
    s2.create();
    up.create();
    done.create();
    G16_HIP(hipMemcpyAsync(dvk.p, hv.get(), sizeof(VkDev), hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipMemcpyAsync(d1.p, g1, d1.bytes(), hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipMemcpyAsync(d2.p, g2, d2.bytes(), hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipEventRecord(up.e, s1.s));
    G16_HIP(hipStreamWaitEvent(s2.s, up.e, 0));
    G16_LAUNCH(k_vp_g2, 1, COOP_LANES, 0, s2.s, (const VkDev*)dvk.p, (const uint8_t*)d2.p, 128u, n_pairs, k_lo, k_hi,
               dg2ok.p);
    G16_HIP(hipEventRecord(done.e, s2.s));
    G16_LAUNCH(k_pc_pairing, 1, COOP_LANES, 0, s1.s, (const VkDev*)dvk.p, (const uint8_t*)d1.p, (const uint8_t*)d2.p,
               n_pairs, dok.p);
    G16_HIP(hipStreamWaitEvent(s1.s, done.e, 0));
    G16_LAUNCH(k_vp_and, 1, 64, 0, s1.s, dok.p, (const uint8_t*)dg2ok.p, 1u, n_pairs, 1);
    uint8_t ok = 0;
    G16_HIP(hipMemcpyAsync(&ok, dok.p, 1, hipMemcpyDeviceToHost, s1.s));
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(s1.s));
    G16_HIP(hipStreamSynchronize(s2.s));
    *ok_out = ok;
    return G16_OK;
  });
}

extern "C" g16_status g16_verify_prepared_times(float* ms, uint32_t cap) {
  return t_phase.read(ms, cap);
}
