// poly.h -- division of polynomials over Fr by (X - z) on the device (poly.hip): the quotient a KZG opening commits
// to.  g16_poly_divide_linear (include/g16_amd.h) is the host-to-host form; kzg.hip enqueues the device form and hands
// the quotients to the MSM without a copy.
#pragma once
#include "../../include/g16_amd.h"

#include "common.h"

namespace g16 {

constexpr uint32_t PD_RUN = G16_POLY_RUN;      // coefficients per thread
constexpr uint32_t PD_BLOCK = G16_POLY_BLOCK;  // threads per block
constexpr uint32_t PD_TILE = PD_RUN * PD_BLOCK;
constexpr size_t PD_MAX_N = (size_t)1 << 27;
constexpr uint32_t PD_TABLE = 1 + PD_BLOCK + PD_BLOCK + 1;  // z | w^0 .. w^(BLOCK-1) | V^0 .. V^BLOCK  (w = z^RUN, V = w^BLOCK)

// everything a division of `count` polynomials of up to n coefficients needs besides its inputs and outputs
struct PolyDivScratch {
  DevBuf<int32_t> table;  // [count][PD_TABLE][9]
  DevBuf<int32_t> local;  // [count][9][threads]: every run's carry from the runs to its right inside its block
  DevBuf<int32_t> btot;   // [count][blocks][9]: every block's value
  DevBuf<int32_t> bcar;   // [count][blocks][9]: every block's carry from the blocks to its right
  size_t cap_n = 0, cap_count = 0;
  void reserve(size_t n, size_t count);
  static size_t bytes_for(size_t n, size_t count);
};

// Enqueues the division of `count` (<= 65535) polynomials of n >= 1 coefficients (4 x u64 Montgomery, device memory),
// polynomial k at coeffs + k * in_stride with its point z_dev[k]: quotient k (n - 1 coefficients) at
// quot + k * q_stride, remainder at rem[k].  quot may not overlap coeffs.  Four launches, no host round trip.
void poly_divide_enqueue(const Fr* coeffs, size_t in_stride, size_t n, size_t count, const Fr* z_dev, Fr* quot,
                         size_t q_stride, Fr* rem, PolyDivScratch& ws, hipStream_t s);

}  // namespace g16
