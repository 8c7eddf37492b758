// poly.hip -- p(X) = q(X) (X - z) + y for many polynomials over Fr, on the lazy 9 x 29-bit limbs of field29.h.
//
// The quotient is the suffix recurrence s_i = a_i + z s_(i+1): q_(i-1) = s_i, y = s_0.  A serial chain of n products
// as it stands; cut into runs it is a scan with the uniform weight w = z^RUN:
//   k_pd_setup   one block per polynomial: z in the internal form, w^j for j < BLOCK, V^j for j <= BLOCK (V = w^BLOCK),
//                every power by square-and-multiply in its own lane (a chain of <= 42 dependent products in all)
//   k_pd_runs    lane g runs Horner over the coefficients [g RUN, (g + 1) RUN): h_g.  The block's h are combined by a
//                Hillis-Steele suffix scan in LDS with the weights w^1, w^2, w^4 ..: x_t = sum_(j >= t) w^(j-t) h_j.
//                Lane t keeps x_(t+1), the carry from its right inside the block; x_0 is the block's value
//   k_pd_blocks  one block per polynomial: the same scan over the block values, 256 at a time from the right, with
//                the weights V^1, V^2, V^4 ..: every block's carry from the blocks to its right
//   k_pd_quot    lane g seeds its run with local carry + w^(BLOCK-1-t) x block carry, runs Horner again and writes
//                the quotient (lane 0 of block 0: the remainder)
// (RUN + log2 BLOCK) + (1 + RUN) products per RUN coefficients, 32 B read twice and 32 B written per coefficient; the
// scratch is 36 B per RUN coefficients.  No atomics and one fixed combination order: the bytes never change.
//
// Domains.  A stored coefficient a is canonical a' R (R = 2^256); unpacked into limbs WITHOUT a conversion it is a
// lazy value a' R.  z, w^j, V^j are kept in the internal form (x 2^261), so a product s * z has the value s' z' R
// again: the recurrence runs on stored values as they are and canonical().pack() of a result IS its storage form.
// Bounds (field29.h contract; checked by the emulator build): a Horner value is a + product: in (-p, 3p), limbs
// below 2^30; a scan adds one product in (-p, 2p) per step and carries: after the 8 + 8 steps of the two scans and
// the seed |value| < 40 p, so every product has |value x value| < 80 p^2 (169 p^2 allowed) and canonical() (< 32 p)
// only ever sees Horner values.
#include "poly.h"

#include <algorithm>

#include "field29.h"
#include "hostcall.h"
#include "wtns_ingest.h"

namespace g16 {
namespace {

constexpr int PD_L = f29::N;
constexpr uint32_t TB_Z = 0, TB_W = 1, TB_V = 1 + PD_BLOCK;
static_assert((PD_BLOCK & (PD_BLOCK - 1)) == 0 && PD_BLOCK <= 256, "the scans assume a power-of-two block of <= 256 lanes");

__device__ __forceinline__ Fr29 ld9(const int32_t* p) {
  Fr29 x;
#pragma unroll
  for (int k = 0; k < PD_L; ++k) x.l[k] = p[k];
  return x;
}
__device__ __forceinline__ void st9(int32_t* p, const Fr29& x) {
#pragma unroll
  for (int k = 0; k < PD_L; ++k) p[k] = x.l[k];
}
// LDS image of the scans: limb k of lane t at sh[t * 9 + k] (9 is odd: the 64 lanes of a wave hit 64 banks)
__device__ __forceinline__ Fr29 lds_get(const int32_t* sh, uint32_t t) { return ld9(sh + t * PD_L); }
__device__ __forceinline__ void lds_put(int32_t* sh, uint32_t t, const Fr29& x) { st9(sh + t * PD_L, x); }

// base^e for e < 2^9 by square-and-multiply from e's top bit; base in the internal form
__device__ __forceinline__ Fr29 pd_pow(const Fr29& base, uint32_t e) {
  if (e == 0) return Fr29::one();
  int b = 8;
  while (!((e >> b) & 1)) --b;
  Fr29 r = base;
#pragma unroll 1
  for (--b; b >= 0; --b) {
    r = r * r;
    if ((e >> b) & 1) r = r * base;
  }
  return r;
}

__global__ void __launch_bounds__(PD_BLOCK) k_pd_setup(const Fr* z, int32_t* table) {
  const uint32_t t = threadIdx.x;
  int32_t* tb = table + (size_t)blockIdx.x * PD_TABLE * PD_L;
  const Fr29 zi = Fr29::from_mont256(z[blockIdx.x]);
  const Fr29 w = pd_pow(zi, PD_RUN);
  const Fr29 v = pd_pow(w, PD_BLOCK);
  st9(tb + (size_t)(TB_W + t) * PD_L, pd_pow(w, t));
  st9(tb + (size_t)(TB_V + t + 1) * PD_L, pd_pow(v, t + 1));
  if (t == 0) {
    st9(tb + (size_t)TB_Z * PD_L, zi);
    st9(tb + (size_t)TB_V * PD_L, Fr29::one());
  }
}

// x_t <- sum_(j >= t) wt^(j - t) x_j over the lanes of the block; pw[d] = wt^d for d = 1, 2, 4 ..  Every lane calls it.
__device__ __forceinline__ Fr29 pd_suffix_scan(Fr29 x, int32_t* sh, const int32_t* pw) {
  const uint32_t t = threadIdx.x;
  lds_put(sh, t, x);
#pragma unroll 1
  for (uint32_t d = 1; d < PD_BLOCK; d <<= 1) {
    __syncthreads();
    const bool has = t + d < PD_BLOCK;
    const Fr29 y = has ? lds_get(sh, t + d) : Fr29::zero();
    __syncthreads();
    if (has) {
      x = (x + ld9(pw + (size_t)d * PD_L) * y).carry();
      lds_put(sh, t, x);
    }
  }
  __syncthreads();
  return x;
}

// Horner over the run [base, base + RUN) from the top, seeded with s; WRITE: the quotient / remainder leave here
template <bool WRITE>
__device__ __forceinline__ Fr29 pd_run(const Fr* __restrict__ a, size_t n, size_t base, const Fr29& zi, Fr29 s,
                                       Fr* __restrict__ q, Fr* __restrict__ rem) {
#pragma unroll
  for (int j = (int)PD_RUN - 1; j >= 0; --j) {
    const size_t i = base + (size_t)j;
    if (i < n) {
      s = Fr29::unpack(a[i].v) + zi * s;
      if (WRITE) {
        Fr o;
        s.canonical().pack(o.v);
        if (i) q[i - 1] = o;
        else *rem = o;
      }
    }
  }
  return s;
}

__global__ void __launch_bounds__(PD_BLOCK) k_pd_runs(const Fr* __restrict__ coeffs, size_t in_stride, size_t n,
                                                      const int32_t* __restrict__ table, int32_t* __restrict__ local,
                                                      int32_t* __restrict__ btot) {
  __shared__ int32_t sh[PD_BLOCK * PD_L];
  const uint32_t t = threadIdx.x, k = blockIdx.y, nblk = gridDim.x;
  const size_t g = (size_t)blockIdx.x * PD_BLOCK + t, threads = (size_t)nblk * PD_BLOCK;
  const int32_t* tb = table + (size_t)k * PD_TABLE * PD_L;
  const Fr29 zi = ld9(tb + (size_t)TB_Z * PD_L);
  Fr29 x = pd_run<false>(coeffs + (size_t)k * in_stride, n, g * PD_RUN, zi, Fr29::zero(), nullptr, nullptr).carry();
  x = pd_suffix_scan(x, sh, tb + (size_t)TB_W * PD_L);
  const Fr29 right = t + 1 < PD_BLOCK ? lds_get(sh, t + 1) : Fr29::zero();
  int32_t* lo = local + (size_t)k * PD_L * threads;
#pragma unroll
  for (int j = 0; j < PD_L; ++j) lo[(size_t)j * threads + g] = right.l[j];
  if (t == 0) st9(btot + ((size_t)k * nblk + blockIdx.x) * PD_L, x);
}

__global__ void __launch_bounds__(PD_BLOCK) k_pd_blocks(const int32_t* __restrict__ btot, uint32_t nblk,
                                                        const int32_t* __restrict__ table, int32_t* __restrict__ bcar) {
  __shared__ int32_t sh[PD_BLOCK * PD_L];
  const uint32_t t = threadIdx.x, k = blockIdx.x;
  const int32_t* tb = table + (size_t)k * PD_TABLE * PD_L;
  const int32_t* bt = btot + (size_t)k * nblk * PD_L;
  int32_t* bc = bcar + (size_t)k * nblk * PD_L;
  Fr29 carry = Fr29::zero();  // the suffix value at the right end of the chunk
#pragma unroll 1
  for (uint32_t hi = nblk; hi > 0;) {
    const uint32_t lo = hi > PD_BLOCK ? hi - PD_BLOCK : 0, m = hi - lo;
    Fr29 x = t < m ? ld9(bt + (size_t)(lo + t) * PD_L) : Fr29::zero();
    x = pd_suffix_scan(x, sh, tb + (size_t)TB_V * PD_L);
    if (t < m) x = (x + ld9(tb + (size_t)(TB_V + m - t) * PD_L) * carry).carry();
    lds_put(sh, t, x);
    __syncthreads();
    if (t < m) st9(bc + (size_t)(lo + t) * PD_L, t + 1 < m ? lds_get(sh, t + 1) : carry);
    carry = lds_get(sh, 0);
    __syncthreads();
    hi = lo;
  }
}

__global__ void __launch_bounds__(PD_BLOCK) k_pd_quot(const Fr* __restrict__ coeffs, size_t in_stride, size_t n,
                                                      const int32_t* __restrict__ table,
                                                      const int32_t* __restrict__ local,
                                                      const int32_t* __restrict__ bcar, Fr* __restrict__ quot,
                                                      size_t q_stride, Fr* __restrict__ rem) {
  const uint32_t t = threadIdx.x, k = blockIdx.y, nblk = gridDim.x;
  const size_t g = (size_t)blockIdx.x * PD_BLOCK + t, threads = (size_t)nblk * PD_BLOCK;
  if (g * PD_RUN >= n) return;
  const int32_t* tb = table + (size_t)k * PD_TABLE * PD_L;
  const Fr29 zi = ld9(tb + (size_t)TB_Z * PD_L);
  const int32_t* lo = local + (size_t)k * PD_L * threads;
  Fr29 s;
#pragma unroll
  for (int j = 0; j < PD_L; ++j) s.l[j] = lo[(size_t)j * threads + g];
  s = s + ld9(tb + (size_t)(TB_W + PD_BLOCK - 1 - t) * PD_L) * ld9(bcar + ((size_t)k * nblk + blockIdx.x) * PD_L);
  pd_run<true>(coeffs + (size_t)k * in_stride, n, g * PD_RUN, zi, s, quot + (size_t)k * q_stride, rem + k);
}

uint32_t pd_blocks(size_t n) { return (uint32_t)((n + PD_TILE - 1) / PD_TILE); }

}  // namespace

size_t PolyDivScratch::bytes_for(size_t n, size_t count) {
  const size_t nb = pd_blocks(n ? n : 1);
  return count * 4 * PD_L * ((size_t)PD_TABLE + nb * PD_BLOCK + 2 * nb);
}

void PolyDivScratch::reserve(size_t n, size_t count) {
  if (n <= cap_n && count <= cap_count) return;
  n = std::max(n, cap_n);
  count = std::max(count, cap_count);
  const size_t nb = pd_blocks(n ? n : 1);
  table.alloc(count * PD_TABLE * PD_L);
  local.alloc(count * PD_L * nb * PD_BLOCK);
  btot.alloc(count * nb * PD_L);
  bcar.alloc(count * nb * PD_L);
  cap_n = n;
  cap_count = count;
}

void poly_divide_enqueue(const Fr* coeffs, size_t in_stride, size_t n, size_t count, const Fr* z_dev, Fr* quot,
                         size_t q_stride, Fr* rem, PolyDivScratch& ws, hipStream_t s) {
  if (!count) return;
  if (n < 1 || n > PD_MAX_N || count > 65535) throw std::runtime_error("poly_divide_enqueue: size out of range");
  ws.reserve(n, count);
  const uint32_t nb = pd_blocks(n);
  G16_LAUNCH(k_pd_setup, (uint32_t)count, PD_BLOCK, 0, s, z_dev, ws.table.p);
  G16_LAUNCH(k_pd_runs, dim3(nb, (uint32_t)count), PD_BLOCK, 0, s, coeffs, in_stride, n, (const int32_t*)ws.table.p,
             ws.local.p, ws.btot.p);
  G16_LAUNCH(k_pd_blocks, (uint32_t)count, PD_BLOCK, 0, s, (const int32_t*)ws.btot.p, nb, (const int32_t*)ws.table.p,
             ws.bcar.p);
  G16_LAUNCH(k_pd_quot, dim3(nb, (uint32_t)count), PD_BLOCK, 0, s, coeffs, in_stride, n, (const int32_t*)ws.table.p,
             (const int32_t*)ws.local.p, (const int32_t*)ws.bcar.p, quot, q_stride, rem);
  G16_HIP(hipGetLastError());
}

}  // namespace g16

using namespace g16;

static g16_status pd_fail(g16_status code, const std::string& msg) {
  set_create_error(msg);
  return code;
}

extern "C" g16_status g16_poly_divide_linear(int device, const void* coeffs, size_t n, size_t count, const void* z,
                                             uint32_t flags, void* quot_out, uint64_t* rem_out) {
  if (count == 0) return G16_OK;
  if (n < 1 || n > PD_MAX_N) return pd_fail(G16_ERR_INVALID, "g16_poly_divide_linear: n must be 1 .. 2^27");
  if (count > 65535) return pd_fail(G16_ERR_INVALID, "g16_poly_divide_linear: more than 65535 polynomials");
  if (!coeffs || !z || !rem_out || (n > 1 && !quot_out)) return pd_fail(G16_ERR_INVALID, "g16_poly_divide_linear: null argument");
  if (const g16_status ds = device_ok(device))
    return ds == G16_ERR_INVALID ? pd_fail(ds, "g16_poly_divide_linear: device out of range") : ds;
  const bool canon = (flags & G16_MSM_SCALARS_CANONICAL) != 0, on_dev = (flags & G16_MSM_SCALARS_DEVICE) != 0;
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    const size_t total = n * count, qn = (n - 1) * count;
    DevBuf<Fr> din, dq, dz, drem;
    DevBuf<unsigned long long> dbad;
    PolyDivScratch ws;
    const Fr* src = (const Fr*)coeffs;
    if (!on_dev || canon) {
      din.alloc(total);
      G16_HIP(hipMemcpy(din.p, coeffs, total * sizeof(Fr), on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
      src = din.p;
    }
    dz.alloc(count);
    drem.alloc(count);
    G16_HIP(hipMemcpy(dz.p, z, count * sizeof(Fr), hipMemcpyHostToDevice));
    if (canon) {
      unsigned long long bad[2] = {INGEST_NONE, INGEST_NONE};
      dbad.alloc(2);
      G16_HIP(hipMemcpy(dbad.p, bad, 16, hipMemcpyHostToDevice));
      fr_from_canonical_enqueue(din.p, din.p, total, dbad.p, nullptr);
      fr_from_canonical_enqueue(dz.p, dz.p, count, dbad.p + 1, nullptr);
      G16_HIP(hipMemcpy(bad, dbad.p, 16, hipMemcpyDeviceToHost));
      if (bad[0] != INGEST_NONE)
        return pd_fail(G16_ERR_INVALID, "g16_poly_divide_linear: coefficient " + std::to_string(bad[0]) + " is >= the field modulus");
      if (bad[1] != INGEST_NONE)
        return pd_fail(G16_ERR_INVALID, "g16_poly_divide_linear: point " + std::to_string(bad[1]) + " is >= the field modulus");
    }
    Fr* q = (Fr*)quot_out;
    if (!on_dev) {
      dq.alloc(qn ? qn : 1);
      q = dq.p;
    }
    poly_divide_enqueue(src, n, n, count, dz.p, q, n - 1, drem.p, ws, nullptr);
    if (!on_dev && qn) G16_HIP(hipMemcpy(quot_out, dq.p, qn * sizeof(Fr), hipMemcpyDeviceToHost));
    G16_HIP(hipMemcpy(rem_out, drem.p, count * sizeof(Fr), hipMemcpyDeviceToHost));
    return G16_OK;
  }, pd_fail);
}
