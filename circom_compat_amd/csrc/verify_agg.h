// verify_agg.h -- the device helpers the aggregate verifiers share: verify.hip (one key per call) and
// verify_keys.hip (many keys per call).  The scheme they serve is described at k_agg_front in verify.hip.
#pragma once
#include "pairing.h"

namespace g16 {
namespace {

constexpr uint32_t AGG_BLOCK = 64;

struct AggKey {
  G1Affine p[3];  // G1 sides paired with beta, gamma, delta
};

// sh[0] <- sum of sh[0 .. AGG_BLOCK): every lane of the block calls it, v = the lane's own term
__device__ __forceinline__ void block_sum_g1(G1XYZZ* sh, G1XYZZ v) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
#pragma unroll 1
  for (uint32_t s = AGG_BLOCK / 2; s > 0; s >>= 1) {
    __syncthreads();  // lanes < s read the upper half [s, 2s) and write the lower: one barrier per round
    if (t < s) {
      v.add(sh[t + s]);
      sh[t] = v;
    }
  }
  __syncthreads();
}

}  // namespace
}  // namespace g16
