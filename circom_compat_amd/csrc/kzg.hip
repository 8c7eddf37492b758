// kzg.hip -- KZG commit / open / verify on a powers-of-tau string (include/g16_amd.h), the first user of the MSM over
// caller-supplied bases (msm_bases.hip) and of the division by (X - z) (poly.hip).
//   key      an MSM handle over tau_g1[0, max_len) with planes, plus tau_g2[1]
//   commit   g16_msm on the key's bases
//   open     per chunk of the handle's batch: coefficients -> division -> quotients stay in device memory -> one
//            chunked MSM (one sort, one accumulation, one reduction) -> count x (32 + 64) bytes to the host
//   verify   e(sum rho_i (C_i - y_i G + z_i pi_i), G2) e(-sum rho_i pi_i, tau G2) = 1: the scalars rho_i, rho_i z_i,
//            -sum rho_i y_i and -rho_i on the lazy Fr of field29.h (k_kzg_scalars, k_kzg_sum: a fixed tree, no
//            atomics), two one-shot MSMs over 2n + 1 and n points, then g16_pairing_check on two pairs
#include "msm_bases.h"

#include <algorithm>
#include <memory>

#include "keycheck.h"
#include "poly.h"

using namespace g16;

struct g16_kzg_key {
  g16_msm_bases* bases = nullptr;
  uint8_t tau_g2[128] = {0};
  uint32_t max_len = 0;
  PolyDivScratch ws;
  DevBuf<Fr> cstage, quot;  // [batch][max_len]: coefficients that arrive from the host / in canonical form; quotients
  DevBuf<Fr> zdev, rem;     // [batch]
  DevBuf<unsigned long long> bad;  // [2]: first coefficient / first point >= r
  ~g16_kzg_key() { g16_msm_bases_destroy(bases); }
};

namespace {

enum { T_IN = 0, T_MID, T_MSM, T_OUT, T_COUNT };
thread_local PhaseTimes<T_COUNT> t_phase;

// T_COUNT + 1 marks on stream s; collect() adds the intervals to the thread's phase times
struct Marks {
  EventBox e[T_COUNT + 1];
  hipStream_t s;
  explicit Marks(hipStream_t stream) : s(stream) {
    for (auto& x : e) x.create(true);
  }
  void mark(int i) { G16_HIP(hipEventRecord(e[i].e, s)); }
  void collect() {
    G16_HIP(hipEventSynchronize(e[T_COUNT].e));
    t_phase.take(Stored::ADD, e, {{0, 1, T_IN}, {1, 2, T_MID}, {2, 3, T_MSM}, {3, 4, T_OUT}});
  }
};

g16_status kz_fail(g16_status code, const std::string& msg) {
  set_create_error(msg);
  return code;
}

constexpr uint32_t KZ_BLOCK = 256;

// rho_m: rho_i as Montgomery Fr.  s1 = rho_i (i < n) | rho_i z_i (n + i); s2 = -rho_i; prod = rho_i y_i.  A stored
// value unpacked without a conversion is v R; rho in the internal form (x 2^261) times it is (rho v) R again.
__global__ void __launch_bounds__(KZ_BLOCK) k_kzg_scalars(const Fr* rho_m, const Fr* z, const Fr* y, uint32_t n, Fr* s1,
                                                          Fr* s2, Fr* prod) {
  const uint32_t i = blockIdx.x * KZ_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Fr r = rho_m[i];
  const Fr29 ri = Fr29::from_mont256(r);
  Fr o;
  s1[i] = r;
  (ri * Fr29::unpack(z[i].v)).canonical().pack(o.v);
  s1[n + i] = o;
  (ri * Fr29::unpack(y[i].v)).canonical().pack(o.v);
  prod[i] = o;
  (Fr29::zero() - Fr29::unpack(r.v)).canonical().pack(o.v);
  s2[i] = o;
}

// one block: *out = -sum_i prod[i], lane t sums the entries t, t + 256, .. in order, then a fixed tree
__global__ void __launch_bounds__(KZ_BLOCK) k_kzg_sum(const Fr* prod, uint32_t n, Fr* out) {
  __shared__ int32_t sh[KZ_BLOCK * f29::N];
  const uint32_t t = threadIdx.x;
  Fr29 acc = Fr29::zero();
#pragma unroll 1
  for (uint32_t i = t; i < n; i += KZ_BLOCK) acc = (acc + Fr29::unpack(prod[i].v)).canonical();
#pragma unroll 1
  for (uint32_t s = KZ_BLOCK / 2; s > 0; s >>= 1) {
#pragma unroll
    for (int k = 0; k < f29::N; ++k) sh[t * f29::N + k] = acc.l[k];
    __syncthreads();
    if (t < s) {
      Fr29 b;
#pragma unroll
      for (int k = 0; k < f29::N; ++k) b.l[k] = sh[(t + s) * f29::N + k];
      acc = (acc + b).canonical();
    }
    __syncthreads();
  }
  if (t == 0) {
    Fr o;
    (Fr29::zero() - acc).canonical().pack(o.v);
    *out = o;
  }
}

}  // namespace

extern "C" g16_status g16_kzg_key_create(int device, const g16_srs_desc* srs, size_t max_len, const g16_msm_options* opt,
                                         g16_kzg_key** out) {
  if (!out) return kz_fail(G16_ERR_INVALID, "g16_kzg_key_create: null argument");
  *out = nullptr;
  if (!srs || !srs->tau_g1 || !srs->tau_g2) return kz_fail(G16_ERR_INVALID, "g16_kzg_key_create: null argument");
  if (srs->n_tau < 2) return kz_fail(G16_ERR_INVALID, "g16_kzg_key_create: the string has no tau_g2[1]");
  if (max_len == 0) max_len = srs->n_tau_g1;
  if (max_len < 1 || max_len > srs->n_tau_g1)
    return kz_fail(G16_ERR_INVALID, "g16_kzg_key_create: max_len exceeds the entries of tau_g1");
  g16_msm_options o{0, 0, 1, 0};
  if (opt) o = *opt;
  o.validate = 0;  // the string is taken as it comes: g16_srs_check verifies one
  std::unique_ptr<g16_kzg_key> k(new g16_kzg_key);
  const g16_status st = g16_msm_bases_create(device, G16_GROUP_G1, srs->tau_g1, max_len, 0, &o, &k->bases);
  if (st != G16_OK) return st;
  const g16_status made = guarded_call([&] {
    memcpy(k->tau_g2, srs->tau_g2 + 128, 128);
    k->max_len = (uint32_t)max_len;
    const size_t b = k->bases->batch;
    k->cstage.alloc(b * max_len);
    k->quot.alloc(b * max_len);
    k->zdev.alloc(b);
    k->rem.alloc(b);
    k->bad.alloc(2);
    k->ws.reserve(max_len, b);
  }, kz_fail);
  if (made != G16_OK) return made;
  *out = k.release();
  return G16_OK;
}

extern "C" void g16_kzg_key_destroy(g16_kzg_key* k) {
  if (!k) return;
  (void)hipSetDevice(k->bases->device);
  if (k->bases->stream) (void)hipStreamSynchronize(k->bases->stream);
  delete k;
}

extern "C" g16_status g16_kzg_key_info(const g16_kzg_key* k, uint32_t out[8]) {
  if (!k || !out) return G16_ERR_INVALID;
  return g16_msm_bases_info(k->bases, out);
}

extern "C" g16_status g16_kzg_commit(g16_kzg_key* k, const void* coeffs, size_t len, size_t count, size_t stride,
                                     uint32_t flags, uint8_t* out) {
  if (!k) return kz_fail(G16_ERR_INVALID, "g16_kzg_commit: null argument");
  if (len > k->max_len) return kz_fail(G16_ERR_INVALID, "g16_kzg_commit: more coefficients than the key holds powers");
  return g16_msm(k->bases, coeffs, len, count, stride, flags, out);
}

extern "C" g16_status g16_kzg_open(g16_kzg_key* k, const void* coeffs, size_t len, size_t count, size_t stride,
                                   const void* z, uint32_t flags, uint64_t* y_out, uint8_t* proof_out) {
  if (!k) return kz_fail(G16_ERR_INVALID, "g16_kzg_open: null argument");
  if (count == 0) return G16_OK;
  if (!coeffs || !z || !y_out || !proof_out) return kz_fail(G16_ERR_INVALID, "g16_kzg_open: null argument");
  if (len < 1) return kz_fail(G16_ERR_INVALID, "g16_kzg_open: a polynomial has at least one coefficient");
  if (len > k->max_len) return kz_fail(G16_ERR_INVALID, "g16_kzg_open: more coefficients than the key holds powers");
  if (count > 1 && stride < len) return kz_fail(G16_ERR_INVALID, "g16_kzg_open: stride below len");
  if (count == 1) stride = len;
  const bool canon = (flags & G16_MSM_SCALARS_CANONICAL) != 0, on_dev = (flags & G16_MSM_SCALARS_DEVICE) != 0;
  g16_msm_bases* h = k->bases;
  std::lock_guard<std::mutex> lock(h->mu);
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    t_phase.clear();
    Marks ev(s);
    const Fr* in = (const Fr*)coeffs;
    const Fr* zin = (const Fr*)z;
    for (size_t k0 = 0; k0 < count; k0 += h->batch) {
      const uint32_t b = (uint32_t)std::min<size_t>(h->batch, count - k0);
      const Fr* src = in + k0 * stride;
      size_t st = stride;
      unsigned long long bad[2] = {INGEST_NONE, INGEST_NONE};
      ev.mark(T_IN);
      if (canon || !on_dev) {
        for (uint32_t j = 0; j < b; ++j)
          G16_HIP(hipMemcpyAsync(k->cstage.p + (size_t)j * len, in + (k0 + j) * stride, len * sizeof(Fr),
                                 on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        src = k->cstage.p;
        st = len;
      }
      G16_HIP(hipMemcpyAsync(k->zdev.p, zin + k0, b * sizeof(Fr), hipMemcpyHostToDevice, s));
      if (canon) {
        G16_HIP(hipMemcpyAsync(k->bad.p, bad, 16, hipMemcpyHostToDevice, s));
        fr_from_canonical_enqueue(k->cstage.p, k->cstage.p, (size_t)b * len, k->bad.p, s);
        fr_from_canonical_enqueue(k->zdev.p, k->zdev.p, b, k->bad.p + 1, s);
      }
      ev.mark(T_MID);
      poly_divide_enqueue(src, st, len, b, k->zdev.p, k->quot.p, len, k->rem.p, k->ws, s);
      ev.mark(T_MSM);
      msm_bases_chunk(h, k->quot.p, (uint32_t)len - 1, b, len);  // len == 1: the point at infinity
      ev.mark(T_OUT);
      if (canon) G16_HIP(hipMemcpyAsync(bad, k->bad.p, 16, hipMemcpyDeviceToHost, s));
      G16_HIP(hipMemcpyAsync(y_out + 4 * k0, k->rem.p, b * sizeof(Fr), hipMemcpyDeviceToHost, s));
      G16_HIP(hipMemcpyAsync(proof_out + 64 * k0, h->out_dev.p, (size_t)b * 64, hipMemcpyDeviceToHost, s));
      ev.mark(T_COUNT);
      G16_HIP(hipStreamSynchronize(s));
      ev.collect();
      if (bad[0] != INGEST_NONE) {
        const unsigned long long at = (unsigned long long)k0 * len + bad[0];
        return kz_fail(G16_ERR_INVALID, "g16_kzg_open: coefficient " + std::to_string(at) + " (polynomial " +
                                            std::to_string(at / len) + ", index " + std::to_string(at % len) +
                                            ") is >= the field modulus");
      }
      if (bad[1] != INGEST_NONE)
        return kz_fail(G16_ERR_INVALID, "g16_kzg_open: point " + std::to_string(k0 + bad[1]) + " is >= the field modulus");
    }
    return G16_OK;
  }, kz_fail);
}

extern "C" g16_status g16_kzg_verify(int device, const uint8_t tau_g2[128], const uint8_t* commitments, const uint64_t* z,
                                     const uint64_t* y, const uint8_t* proofs, size_t n, const uint64_t* rho,
                                     uint8_t* ok_out) {
  if (!ok_out) return kz_fail(G16_ERR_INVALID, "g16_kzg_verify: null argument");
  *ok_out = 0;
  if (n == 0) {
    *ok_out = 1;
    return G16_OK;
  }
  if (!tau_g2 || !commitments || !z || !y || !proofs) return kz_fail(G16_ERR_INVALID, "g16_kzg_verify: null argument");
  if (n >= ((size_t)1 << 26)) return kz_fail(G16_ERR_INVALID, "g16_kzg_verify: 2^26 openings or more");
  if (!rho_all_nonzero(rho, n)) return kz_fail(G16_ERR_INVALID, "g16_kzg_verify: a rho entry is zero");
  if (const g16_status ds = device_ok(device)) return kz_fail(ds, "g16_kzg_verify: no usable device (there is no CPU fallback)");
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    t_phase.clear();
    Marks ev(nullptr);
    const uint32_t nn = (uint32_t)n;
    // rho as canonical 32-byte integers: the conversion kernel of g16_fr_convert makes them Montgomery
    std::vector<uint64_t> hr(4 * n, 0);
    if (rho) {
      for (size_t i = 0; i < n; ++i) hr[4 * i] = rho[2 * i], hr[4 * i + 1] = rho[2 * i + 1];
    } else {
      std::vector<uint64_t> d(2 * n);
      if (!draw_rho(d.data(), n)) return kz_fail(G16_ERR_INTERNAL, "g16_kzg_verify: the operating system gave no randomness");
      for (size_t i = 0; i < n; ++i) hr[4 * i] = d[2 * i], hr[4 * i + 1] = d[2 * i + 1];
    }
    DevBuf<G1Affine> dP;  // C_0 .. | pi_0 .. | G
    DevBuf<Fr> drho, dz, dy, s1, s2, prod;
    DevBuf<uint8_t> dflags;
    DevBuf<unsigned long long> dbad;
    dP.alloc(2 * n + 1);
    drho.alloc(n);
    dz.alloc(n);
    dy.alloc(n);
    s1.alloc(2 * n + 1);
    s2.alloc(n);
    prod.alloc(n);
    dflags.alloc(2 * n);
    dbad.alloc(1);
    ev.mark(T_IN);
    const Fq one = Fq::one();
    const G1Affine gen{one, one + one};
    unsigned long long bad = INGEST_NONE;
    G16_HIP(hipMemcpy(dP.p, commitments, n * 64, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dP.p + n, proofs, n * 64, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dP.p + 2 * n, &gen, 64, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dz.p, z, n * 32, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dy.p, y, n * 32, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(drho.p, hr.data(), n * 32, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dbad.p, &bad, 8, hipMemcpyHostToDevice));
    fr_from_canonical_enqueue(drho.p, drho.p, n, dbad.p, nullptr);  // 128-bit values: always below r
    // canonical words and the curve, for every commitment and proof: the predicates of g16_key_check
    G16_LAUNCH(k_chk_flags_g1, ceil_div(2 * n, KC_BLOCK), KC_BLOCK, 0, nullptr, (const G1Affine*)dP.p, 2 * nn, dflags.p);
    std::vector<uint8_t> hf(2 * n);
    G16_HIP(hipMemcpy(hf.data(), dflags.p, 2 * n, hipMemcpyDeviceToHost));
    ev.mark(T_MID);
    bool structural = true;
    for (uint8_t f : hf) structural = structural && !(f & ~KC_INF);
    uint8_t ok = 0;
    if (structural) {
      G16_LAUNCH(k_kzg_scalars, ceil_div(n, KZ_BLOCK), KZ_BLOCK, 0, nullptr, (const Fr*)drho.p, (const Fr*)dz.p,
                 (const Fr*)dy.p, nn, s1.p, s2.p, prod.p);
      G16_LAUNCH(k_kzg_sum, 1, KZ_BLOCK, 0, nullptr, (const Fr*)prod.p, nn, s1.p + 2 * n);
      G16_HIP(hipGetLastError());
      G16_HIP(hipStreamSynchronize(nullptr));
    }
    ev.mark(T_MSM);
    uint8_t g1[2 * 64], g2[2 * 128];
    if (structural) {
      const uint32_t fl = G16_MSM_POINTS_DEVICE | G16_MSM_SCALARS_DEVICE;
      g16_status st = g16_msm_once(device, G16_GROUP_G1, dP.p, s1.p, 2 * n + 1, fl, g1);
      if (st == G16_OK) st = g16_msm_once(device, G16_GROUP_G1, dP.p + n, s2.p, n, fl, g1 + 64);
      if (st != G16_OK) return st;
    }
    ev.mark(T_OUT);
    if (structural) {
      memcpy(g2, G2_GEN_WORDS, 128);
      memcpy(g2 + 128, tau_g2, 128);
      const g16_status st = g16_pairing_check(device, g1, g2, 2, &ok);
      if (st != G16_OK) return kz_fail(st, "g16_kzg_verify: the pairing check failed to run");
    }
    ev.mark(T_COUNT);
    ev.collect();
    *ok_out = ok;
    return G16_OK;
  }, kz_fail);
}

extern "C" g16_status g16_kzg_times(float* ms, uint32_t cap) {
  return t_phase.read(ms, cap);
}
