// rerandomize.hip -- Groth16 proof re-randomisation (g16_proofs_rerandomize, g16_proofs_rerandomize_keys): what
// ark_groth16::Groth16::rerandomize_proof does for ONE proof on the host, for a whole batch with one lane per proof.
// For a proof (A, B, C) under a key with delta in G2, and r1 != 0, r2 in Fr:
//   A' = r1^-1 A        B' = r1 B + (r1 r2) delta        C' = C + r2 A
// (A', B', C') verifies for exactly the public inputs (A, B, C) verifies for.  No witness, no proving key.
//
// Kernels, all one lane per proof (or per point), no atomics, the same bytes on every run:
//   k_rr_check    the structural tests, before any arithmetic: every stored coordinate < q, A and C on the curve,
//                 B on the twist.  The prime-order subgroup test of B is NOT applied (include/g16_amd.h says why).
//   k_rr_scalars  (r1, r2) -> the canonical 256-bit integers of r1^-1, r1, r1 r2, r2; the inversion (Fermat) runs
//                 on the device, one per lane.
//   k_rr_g1       grid.y = 0: r1^-1 A.  grid.y = 1: r2 A, then one mixed addition of C.  The ladder of
//                 srs_contribute.hip's k_sx_mul: 256 positions, a doubling at each, a mixed addition of the affine A
//                 predicated on the lane's own bit.
//   k_rr_g2       ONE joint ladder for r1 B + (r1 r2) delta: one doubling chain of 256 positions, at each a mixed
//                 addition of B on the bit of r1 and a mixed addition of delta on the bit of r1 r2 -- half the
//                 doublings of two ladders.  B lives in the lane's registers; delta is the same for every lane of a
//                 block (a block never spans two groups) and is read through a block-uniform pointer, so it sits in
//                 scalar registers, not in the lane's.
//   k_xyzz_to_affine<F>  (toaffine.h) back to canonical affine with one inversion per run of 8 points, written
//                 straight into the 256-byte output records: A and C of record i are points i and n + i of one array.
// XYZZ::madd handles equal, opposite and infinite operands, so B = +-delta, C = +-A and points at infinity (all
// reachable from untrusted input) take the doubling / cancelling branches and need nothing of their own here.
// The G1 kernels and the G2 kernels run on two streams: a small batch pays the G2 ladder's latency once.
#include <stdlib.h>

#include "keycheck.h"
#include "toaffine.h"

namespace g16 {
namespace {

constexpr uint32_t RR_REC = G16_PROOF_BYTES;
constexpr uint32_t RR_OFF_B = 64, RR_OFF_C = 192;

enum { T_UPLOAD = 0, T_PREPARE, T_MUL_G1, T_MUL_G2, T_AFFINE, T_DOWNLOAD, T_COUNT };
thread_local PhaseTimes<T_COUNT> t_phase;

// one block of the ladder kernels: `count` <= KC_BLOCK consecutive proofs from `first`, all under key `key`
struct Tile {
  uint32_t first, count, key, pad;
};

G16_HD const G1Affine* rec_a(const uint8_t* recs, uint32_t i) { return (const G1Affine*)(recs + (size_t)i * RR_REC); }
G16_HD const G2Affine* rec_b(const uint8_t* recs, uint32_t i) {
  return (const G2Affine*)(recs + (size_t)i * RR_REC + RR_OFF_B);
}
G16_HD const G1Affine* rec_c(const uint8_t* recs, uint32_t i) {
  return (const G1Affine*)(recs + (size_t)i * RR_REC + RR_OFF_C);
}

__global__ void __launch_bounds__(256) k_rr_check(const uint8_t* recs, uint32_t n, Fq2 b_twist, uint8_t* ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Affine a = *rec_a(recs, i), c = *rec_c(recs, i);
  const G2Affine b = *rec_b(recs, i);
  bool good = fq_words_canonical(a.x) && fq_words_canonical(a.y) && fq_words_canonical(c.x) &&
              fq_words_canonical(c.y) && fq2_words_canonical(b.x) && fq2_words_canonical(b.y);
  good = good && on_curve_g1(a) && on_curve_g1(c);
  good = good && (b.is_inf() || b.y.sqr() == b.x.sqr() * b.x + b_twist);
  ok[i] = good ? 1 : 0;
}

// rs: n x (r1, r2) Montgomery; out: four planes of n canonical integers: r1^-1, r1, r1 r2, r2
__global__ void __launch_bounds__(256) k_rr_scalars(const Fr* rs, uint32_t n, U256* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr r1 = rs[2 * (size_t)i], r2 = rs[2 * (size_t)i + 1];
  out[i] = r1.inv().to_canonical();
  out[(size_t)n + i] = r1.to_canonical();
  out[2 * (size_t)n + i] = (r1 * r2).to_canonical();
  out[3 * (size_t)n + i] = r2.to_canonical();
}

// work[i] = r1^-1 A_i (blockIdx.y == 0), work[n + i] = C_i + r2 A_i (blockIdx.y == 1)
__global__ void __launch_bounds__(KC_BLOCK) k_rr_g1(const uint8_t* recs, const uint8_t* ok, const U256* sc, uint32_t n,
                                                     G1XYZZ* work) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const bool with_c = blockIdx.y != 0;
  G1XYZZ* dst = work + (with_c ? (size_t)n + i : (size_t)i);
  if (!ok[i]) {
    *dst = G1XYZZ::infinity();
    return;
  }
  const G1Affine p = *rec_a(recs, i);
  const uint32_t* k = sc[(with_c ? 3 * (size_t)n : (size_t)0) + i].v;
  G1XYZZ acc = G1XYZZ::infinity();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    uint32_t kw = k[w];
#pragma unroll 1
    for (int b = 0; b < 32; ++b, kw <<= 1) {
      acc.dbl_in_place();
      if (kw >> 31) acc.madd(p);
    }
  }
  if (with_c) acc.madd(*rec_c(recs, i));
  *dst = acc;
}

// work[i] = r1 B_i + (r1 r2) delta_key(i): the joint ladder, one block per tile
__global__ void __launch_bounds__(KC_BLOCK) k_rr_g2(const uint8_t* recs, const uint8_t* ok, const U256* sc, uint32_t n,
                                                     const Tile* __restrict__ tiles,
                                                     const G2Affine* __restrict__ deltas, G2XYZZ* work) {
  const Tile t = tiles[blockIdx.x];
  if (threadIdx.x >= t.count) return;
  const uint32_t i = t.first + threadIdx.x;
  if (!ok[i]) {
    work[i] = G2XYZZ::infinity();
    return;
  }
  const G2Affine* __restrict__ dp = deltas + t.key;  // block-uniform
  const G2Affine p = *rec_b(recs, i);
  const uint32_t* kb = sc[(size_t)n + i].v;
  const uint32_t* kd = sc[2 * (size_t)n + i].v;
  G2XYZZ acc = G2XYZZ::infinity();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    uint32_t wb = kb[w], wd = kd[w];
#pragma unroll 1
    for (int b = 0; b < 32; ++b, wb <<= 1, wd <<= 1) {
      acc.dbl_in_place();
      if (wb >> 31) acc.madd(p);
      if (wd >> 31) acc.madd(*dp);
    }
  }
  work[i] = acc;
}

// the (r1, r2) of the call on the host, and the pool the drawn ones come from: wiped on every way out
struct Secret {
  std::vector<Fr> rs;
  FrPool pool;
  ~Secret() {
    if (!rs.empty()) wipe(rs.data(), rs.size() * sizeof(Fr));
  }
};

enum { E_UP0 = 0, E_UP1, E_PREP, E_G1A, E_G1B, E_G1C, E_G2A, E_G2B, E_G2C, E_DN0, E_DN1, E_COUNT };

g16_status rerandomize(int device, const uint8_t* deltas, const uint32_t* counts, uint32_t n_keys,
                       const uint8_t* proofs, const uint64_t* scalars, uint8_t* proofs_out, uint8_t* ok_out) {
  if (n_keys == 0) return G16_OK;
  if (!counts) return G16_ERR_INVALID;
  uint64_t total = 0;
  for (uint32_t k = 0; k < n_keys; ++k) total += counts[k];
  if (total > 0xffffffffull / RR_REC) return G16_ERR_INVALID;
  const uint32_t n = (uint32_t)total;
  if (n == 0) return G16_OK;
  if (!deltas || !proofs || !proofs_out) return G16_ERR_INVALID;
  Secret sec;
  sec.rs.resize(2 * (size_t)n);
  if (scalars) {
    memcpy(sec.rs.data(), scalars, sec.rs.size() * sizeof(Fr));
    for (uint32_t i = 0; i < n; ++i)
      if (!fr_words_canonical(sec.rs[2 * (size_t)i]) || sec.rs[2 * (size_t)i].is_zero() ||
          !fr_words_canonical(sec.rs[2 * (size_t)i + 1]))
        return G16_ERR_INVALID;
  }
  if (const g16_status ds = device_ok(device)) return ds;
  if (!scalars)
    for (uint32_t i = 0; i < n; ++i)
      if (!(sec.pool.draw_fr(&sec.rs[2 * (size_t)i], true) && sec.pool.draw_fr(&sec.rs[2 * (size_t)i + 1], false)))
        return G16_ERR_INTERNAL;  // never a fixed fallback

  return guarded_call([&]() -> g16_status {
    // a block of the G2 ladder never spans two groups: its delta is block-uniform
    std::vector<Tile> tiles;
    tiles.reserve((size_t)n / KC_BLOCK + n_keys);
    {
      uint32_t at = 0;
      for (uint32_t k = 0; k < n_keys; ++k) {
        for (uint32_t done = 0; done < counts[k]; done += KC_BLOCK) {
          const uint32_t left = counts[k] - done;
          tiles.push_back(Tile{at + done, left < KC_BLOCK ? left : KC_BLOCK, k, 0});
        }
        at += counts[k];
      }
    }
    const size_t bytes = (size_t)n * RR_REC;

    G16_HIP(hipSetDevice(device));
    PinnedBuf pin;
    DevBuf<uint8_t> din, dout, dok;
    DevBuf<G2Affine> ddelta;
    DevBuf<Tile> dtiles;
    DevBuf<Fr> drs;
    DevBuf<U256> dsc;
    DevBuf<G1XYZZ> dw1;
    DevBuf<G2XYZZ> dw2;
    StreamBox s1, s2;
    EventBox ev[E_COUNT];
    pin.alloc(bytes);
    din.alloc(bytes);
    dout.alloc(bytes);
    dok.alloc(n);
    ddelta.alloc(n_keys);
    dtiles.alloc(tiles.size());
    drs.alloc(sec.rs.size());
    dsc.alloc(4 * (size_t)n);
    dw1.alloc(2 * (size_t)n);
    dw2.alloc(n);
    s1.create();
    s2.create();
    for (auto& e : ev) e.create(true);

    memcpy(pin.p, proofs, bytes);
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s1.s);
    G16_HIP(hipEventRecord(ev[E_UP0].e, s1.s));
    G16_HIP(hipMemcpyAsync(din.p, pin.p, bytes, hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipMemcpyAsync(ddelta.p, deltas, ddelta.bytes(), hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipMemcpyAsync(dtiles.p, tiles.data(), dtiles.bytes(), hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipMemcpyAsync(drs.p, sec.rs.data(), drs.bytes(), hipMemcpyHostToDevice, s1.s));
    G16_HIP(hipEventRecord(ev[E_UP1].e, s1.s));
    G16_LAUNCH(k_rr_check, ceil_div(n, 256), 256, 0, s1.s, (const uint8_t*)din.p, n, host_consts().b_twist, dok.p);
    G16_LAUNCH(k_rr_scalars, ceil_div(n, 256), 256, 0, s1.s, (const Fr*)drs.p, n, dsc.p);
    G16_HIP(hipEventRecord(ev[E_PREP].e, s1.s));

    // G2 on its own stream, beside the G1 work
    G16_HIP(hipStreamWaitEvent(s2.s, ev[E_PREP].e, 0));
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s2.s);
    G16_HIP(hipEventRecord(ev[E_G2A].e, s2.s));
    G16_LAUNCH(k_rr_g2, (uint32_t)tiles.size(), KC_BLOCK, 0, s2.s, (const uint8_t*)din.p, (const uint8_t*)dok.p,
               (const U256*)dsc.p, n, (const Tile*)dtiles.p, (const G2Affine*)ddelta.p, dw2.p);
    G16_HIP(hipEventRecord(ev[E_G2B].e, s2.s));
    xyzz_to_affine<Fq2>(dw2.p, n, n, RR_OFF_B, RR_OFF_B, RR_REC, dout.p, s2.s);
    G16_HIP(hipEventRecord(ev[E_G2C].e, s2.s));

    G16_HIP(hipEventRecord(ev[E_G1A].e, s1.s));
    G16_LAUNCH(k_rr_g1, dim3(ceil_div(n, KC_BLOCK), 2), KC_BLOCK, 0, s1.s, (const uint8_t*)din.p,
               (const uint8_t*)dok.p, (const U256*)dsc.p, n, dw1.p);
    G16_HIP(hipEventRecord(ev[E_G1B].e, s1.s));
    xyzz_to_affine<Fq>(dw1.p, 2 * n, n, 0u, RR_OFF_C, RR_REC, dout.p, s1.s);
    G16_HIP(hipEventRecord(ev[E_G1C].e, s1.s));

    G16_HIP(hipStreamWaitEvent(s1.s, ev[E_G2C].e, 0));
    G16_LAUNCH(k_phase_mark<>, 1, 1, 0, s1.s);
    G16_HIP(hipEventRecord(ev[E_DN0].e, s1.s));
    G16_HIP(hipMemcpyAsync(pin.p, dout.p, bytes, hipMemcpyDeviceToHost, s1.s));
    G16_HIP(hipEventRecord(ev[E_DN1].e, s1.s));
    std::vector<uint8_t> ok(ok_out ? n : 0);
    if (ok_out) G16_HIP(hipMemcpyAsync(ok.data(), dok.p, n, hipMemcpyDeviceToHost, s1.s));
    // nothing derived from the scalars outlives the call on the device
    G16_HIP(hipMemsetAsync(drs.p, 0, drs.bytes(), s1.s));
    G16_HIP(hipMemsetAsync(dsc.p, 0, dsc.bytes(), s1.s));
    G16_HIP(hipMemsetAsync(dw1.p, 0, dw1.bytes(), s1.s));
    G16_HIP(hipMemsetAsync(dw2.p, 0, dw2.bytes(), s1.s));
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(s1.s));
    G16_HIP(hipStreamSynchronize(s2.s));
    memcpy(proofs_out, pin.p, bytes);
    if (ok_out) memcpy(ok_out, ok.data(), n);

    t_phase.take(Stored::REPLACE, ev,
                 {{E_UP0, E_UP1, T_UPLOAD}, {E_UP1, E_PREP, T_PREPARE}, {E_G1A, E_G1B, T_MUL_G1},
                  {E_G2A, E_G2B, T_MUL_G2}, {E_G1B, E_G1C, T_AFFINE},   {E_G2B, E_G2C, T_AFFINE},
                  {E_DN0, E_DN1, T_DOWNLOAD}});
    return G16_OK;
  });
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" g16_status g16_proofs_rerandomize_keys(int device, const uint8_t* delta_g2s, const uint32_t* counts,
                                                  uint32_t n_keys, const uint8_t* proofs, const uint64_t* scalars,
                                                  uint8_t* proofs_out, uint8_t* ok_out) {
  return rerandomize(device, delta_g2s, counts, n_keys, proofs, scalars, proofs_out, ok_out);
}

extern "C" g16_status g16_proofs_rerandomize(int device, const uint8_t delta_g2[128], const uint8_t* proofs,
                                             uint32_t n_proofs, const uint64_t* scalars, uint8_t* proofs_out,
                                             uint8_t* ok_out) {
  return rerandomize(device, delta_g2, &n_proofs, 1, proofs, scalars, proofs_out, ok_out);
}

extern "C" g16_status g16_proofs_rerandomize_times(float* ms, uint32_t cap) {
  return t_phase.read(ms, cap);
}
