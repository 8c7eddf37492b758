// keygen.h -- what the two key generators share: the g16_setup handle (keygen.hip fills it from toxic waste,
// setup_srs.hip from a powers-of-tau string) and keygen.hip's power / fixed-base kernels behind host calls.
#pragma once
#include "msm.h"
#include "spmv.h"

struct g16_setup {
  uint32_t n_vars = 0, n_public = 0, domain = 0;
  std::vector<uint8_t> a, b1, b2, l, h, ic;
  uint8_t alpha1[64], beta1[64], delta1[64], beta2[128], gamma2[128], delta2[128];
  std::string err;
};

namespace g16 {

// The transposed matrices both key generators take (n_vars rows each, a column is a constraint), checked on the
// host before anything is allocated, copied or launched (csr_check, spmv.h).  A column indexes the Lagrange basis
// of the domain: `at` carries the n_public + 1 rows snarkjs appends behind the constraints and may name
// num_constraints + n_public + 1 of them, bt and ct only the num_constraints proper -- both within the domain.
// NULL when all three are sound, else what is wrong.
const char* setup_matrices_check(const g16_csr* at, const g16_csr* bt, const g16_csr* ct, uint32_t n_vars,
                                 uint32_t n_public, uint32_t num_constraints);

G1Affine g1_generator();
G2Affine g2_generator();

// out[i] = scale * base^i for i < count, 0 for count <= i < total (k_powers; base^i by 28 squarings: i < 2^28)
void fr_powers(const Fr& base, const Fr& scale, Fr* out, uint32_t count, uint32_t total, hipStream_t s);

// the 8-bit windowed tables of the two generators (k_fb_table) and out[i] = scalars[i] * G (k_fb_mul)
struct FixedBase {
  DevBuf<G1Affine> tab1;
  DevBuf<G2Affine> tab2;
  void build(hipStream_t s);
  void mul_g1(const Fr* scalars, uint32_t n, G1Affine* out, hipStream_t s) const;
  void mul_g2(const Fr* scalars, uint32_t n, G2Affine* out, hipStream_t s) const;
};

}  // namespace g16
