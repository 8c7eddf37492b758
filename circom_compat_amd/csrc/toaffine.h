// toaffine.h -- XYZZ -> canonical affine by runs, the last kernel of g16_key_contribute (contribute.hip),
// g16_srs_contribute (srs_contribute.hip) and g16_proofs_rerandomize (rerandomize.hip).  ONE Fermat inversion per
// TA_RUN points (Montgomery's trick down each lane's run): 3 multiplications per point for the shared inverse instead
// of ~380.  One copy; each including file gets its own instance of the kernel (anonymous namespace, as in keycheck.h).
// The lazy-limb k_affine of gtransform.h and the one-inversion-per-point kernels (k_mb_affine, k_sums_to_affine,
// k_vp_inputs_affine) have other inputs and stay where they are.
#pragma once
#include "common.h"

namespace g16 {
namespace {

constexpr uint32_t TA_BLOCK = 64;  // lanes per block: one wave
constexpr uint32_t TA_RUN = 8;     // points per lane: one inversion per TA_RUN points

// Slots lie `stride` bytes apart.  Point j < n goes to slot j at byte `off0`, point j >= n to slot j - n at byte
// `off1`; nothing wraps, the caller sizes `out` for max(min(total, n), total - n) slots.  Contiguous Affine<F> is
// n = total, stride = sizeof(Affine<F>), off0 = 0; the 256-byte proof records take A and C from one array of 2 n
// points.  Lane t of block g owns the points
// g * 64 * TA_RUN + k * 64 + t, k < TA_RUN (neighbouring lanes, neighbouring points).  Prefix products of the ZZZ down
// the run (an infinite point counts as 1), one inversion, then back up: 1/ZZZ_k = inv(prefix_k ZZZ_k) prefix_k and
// 1/ZZ = (ZZ / ZZZ)^2 as in XYZZ::to_affine.  The prefixes wait in the x half of the output slot they belong to
// (written here, read back by the same lane): a register array of TA_RUN field elements would be indexed by the
// loop counter and end up in scratch.  A point at infinity leaves as all-zero bytes.
template <class F>
__global__ void __launch_bounds__(TA_BLOCK) k_xyzz_to_affine(const XYZZ<F>* work, uint32_t total, uint32_t n,
                                                             uint32_t off0, uint32_t off1, uint32_t stride,
                                                             uint8_t* out) {
  const uint32_t first = blockIdx.x * (TA_BLOCK * TA_RUN) + threadIdx.x;
  auto slot = [&](uint32_t j) -> Affine<F>* {
    const bool hi = j >= n;
    return (Affine<F>*)(out + (size_t)(hi ? j - n : j) * stride + (hi ? off1 : off0));
  };
  F run = F::one();
  uint32_t cnt = 0;
#pragma unroll 1
  for (uint32_t j = first; cnt < TA_RUN && j < total; ++cnt, j += TA_BLOCK) {
    slot(j)->x = run;
    const F z = work[j].zzz;
    if (!z.is_zero()) run = run * z;
  }
  F inv = run.inv();
#pragma unroll 1
  for (; cnt > 0; --cnt) {
    const uint32_t j = first + (cnt - 1) * TA_BLOCK;
    const XYZZ<F> P = work[j];
    Affine<F>* o = slot(j);
    if (P.zzz.is_zero()) {
      *o = Affine<F>::infinity();
      continue;
    }
    const F iz3 = inv * o->x;
    inv = inv * P.zzz;
    const F iz2 = (iz3 * P.zz).sqr();
    *o = Affine<F>{P.x * iz2, P.y * iz3};
  }
}

template <class F>
void xyzz_to_affine(const XYZZ<F>* work, uint32_t total, uint32_t n, uint32_t off0, uint32_t off1, uint32_t stride,
                    uint8_t* out, hipStream_t s) {
  if (total)
    G16_LAUNCH((k_xyzz_to_affine<F>), ceil_div(total, TA_BLOCK * TA_RUN), TA_BLOCK, 0, s, work, total, n, off0, off1,
               stride, out);
}

// contiguous Affine<F>; out may be the buffer the points came from before they became `work`
template <class F>
void xyzz_to_affine(const XYZZ<F>* work, uint32_t total, Affine<F>* out, hipStream_t s) {
  xyzz_to_affine(work, total, total, 0u, 0u, (uint32_t)sizeof(Affine<F>), (uint8_t*)out, s);
}

}  // namespace
}  // namespace g16
