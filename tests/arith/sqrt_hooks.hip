// sqrt_hooks.hip -- TEST INFRASTRUCTURE ONLY: one-thread-per-case kernels around fq_sqrt / fq2_sqrt of
// csrc/arkser.h (Montgomery words in, the root's Montgomery words and the verdict out), so that pytest can check
// the square roots of the ark-serialize codec alone, against Python's pow.
//
// Built twice from this one file (csrc/Makefile): with g++ against the SIMT emulator into
// tests/emu/libg16_emu.so and with hipcc and the product flags into tests/arith/libg16_sqrt_gpu.so.  Never linked
// into, loaded by or reachable from libg16_amd.so.
//
// Every wrapper returns 0 or a HIP error code.
#include "arkser.h"
#include "common.h"

using namespace g16;

namespace {

constexpr int SQ_BLOCK = 64;  // the tests use case counts that are no multiple of it: the tail guard runs

template <class F>
__global__ void __launch_bounds__(SQ_BLOCK) k_sqrt_hook(const F* in, uint32_t n, F* root, uint8_t* ok) {
  const uint32_t i = blockIdx.x * SQ_BLOCK + threadIdx.x;
  if (i >= n) return;
  F r;
  bool good;
  if constexpr (sizeof(F) == sizeof(Fq)) good = fq_sqrt(in[i], &r);
  else good = fq2_sqrt(in[i], &r);
  root[i] = r;
  ok[i] = good ? 1 : 0;
}

template <class F>
int run_sqrt(const uint32_t* in, uint32_t n, uint32_t* root_out, uint8_t* ok_out) {
  if (!n) return 0;
  try {
    DevBuf<F> din, droot;
    DevBuf<uint8_t> dok;
    din.alloc(n);
    droot.alloc(n);
    dok.alloc(n);
    G16_HIP(hipMemcpy(din.p, in, (size_t)n * sizeof(F), hipMemcpyHostToDevice));
    G16_LAUNCH((k_sqrt_hook<F>), ceil_div(n, SQ_BLOCK), SQ_BLOCK, 0, 0, (const F*)din.p, n, droot.p, dok.p);
    G16_HIP(hipGetLastError());
    G16_HIP(hipDeviceSynchronize());
    G16_HIP(hipMemcpy(root_out, droot.p, (size_t)n * sizeof(F), hipMemcpyDeviceToHost));
    G16_HIP(hipMemcpy(ok_out, dok.p, n, hipMemcpyDeviceToHost));
    return 0;
  } catch (const HipError& e) {
    return e.code ? e.code : -1;
  }
}

}  // namespace

extern "C" int g16_test_fq_sqrt(const uint32_t* in, uint32_t n, uint32_t* root_out, uint8_t* ok_out) {
  return run_sqrt<Fq>(in, n, root_out, ok_out);
}
extern "C" int g16_test_fq2_sqrt(const uint32_t* in, uint32_t n, uint32_t* root_out, uint8_t* ok_out) {
  return run_sqrt<Fq2>(in, n, root_out, ok_out);
}
