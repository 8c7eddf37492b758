// arith_hooks.hip -- TEST INFRASTRUCTURE ONLY: one-thread-per-case kernels around single operations of
// field29.h / ec29.h (raw limbs in, RAW result limbs out, so that pytest can check the output classes the
// headers document) and of field.h / ec.h (storage form in and out); and the launcher of toaffine.h as the product
// calls it.
//
// Built twice from this one file (csrc/Makefile): with g++ against the SIMT emulator into
// tests/emu/libg16_emu.so, where the F29_CHECK input asserts stay on, and with hipcc and the product flags
// into tests/arith/libg16_arith_gpu.so.  Never linked into, loaded by or reachable from libg16_amd.so.
//
// Every wrapper returns 0, a HIP error code, or -1 for an operation the chosen field / curve does not have.
#include "common.h"
#include "ec29.h"
#include "toaffine.h"

using namespace g16;

namespace {

constexpr int BLOCK = 64;        // the tests use case counts that are no multiple of it: the tail guard runs
constexpr int CHAIN_STEPS = 32;

#define ARITH_HIP(expr)                     \
  do {                                      \
    hipError_t _e = (expr);                 \
    if (_e != hipSuccess) return (int)_e;   \
  } while (0)

struct Dev {
  void* p = nullptr;
  ~Dev() {
    if (p) (void)hipFree(p);
  }
  int upload(const void* src, size_t bytes) {
    if (!bytes) return 0;
    ARITH_HIP(hipMalloc(&p, bytes));
    if (src) ARITH_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    else ARITH_HIP(hipMemset(p, 0, bytes));
    return 0;
  }
  int download(void* dst, size_t bytes) const {
    if (bytes) ARITH_HIP(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return 0;
  }
};
#define ARITH_TRY(expr)       \
  do {                        \
    int _s = (expr);          \
    if (_s) return _s;        \
  } while (0)

static int finish_launch() {
  ARITH_HIP(hipGetLastError());
  ARITH_HIP(hipDeviceSynchronize());
  return 0;
}

// ---- raw limb / word access ---------------------------------------------------------------------
template <class T> struct Shape;
template <class P> struct Shape<F29<P>> {
  static constexpr int W = 9, WORDS = 8;
  static constexpr bool X2 = false;
};
template <class P> struct Shape<F29x2<P>> {
  static constexpr int W = 18, WORDS = 16;
  static constexpr bool X2 = true;
};

template <class P> G16_HD void ld_limbs(F29<P>& f, const int32_t* s) {
  for (int i = 0; i < 9; ++i) f.l[i] = s[i];
}
template <class P> G16_HD void ld_limbs(F29x2<P>& f, const int32_t* s) {
  ld_limbs(f.c0, s);
  ld_limbs(f.c1, s + 9);
}
template <class P> G16_HD void st_limbs(int32_t* d, const F29<P>& f) {
  for (int i = 0; i < 9; ++i) d[i] = f.l[i];
}
template <class P> G16_HD void st_limbs(int32_t* d, const F29x2<P>& f) {
  st_limbs(d, f.c0);
  st_limbs(d + 9, f.c1);
}
template <class P> G16_HD void ld_words(Fp<P>& f, const int32_t* s) {
  for (int i = 0; i < 8; ++i) f.v[i] = (uint32_t)s[i];
}
G16_HD void ld_words(Fq2& f, const int32_t* s) {
  ld_words(f.c0, s);
  ld_words(f.c1, s + 8);
}
template <class P> G16_HD void st_words(int32_t* d, const Fp<P>& f) {
  for (int i = 0; i < 8; ++i) d[i] = (int32_t)f.v[i];
}
G16_HD void st_words(int32_t* d, const Fq2& f) {
  st_words(d, f.c0);
  st_words(d + 8, f.c1);
}

// ---- field29.h -------------------------------------------------------------------------------------
enum FieldOp {
  F_MUL = 0, F_SQR, F_MUL2, F_MUL_SUB, F_CARRY, F_CANONICAL, F_IS_ZERO, F_MAYBE_ZERO, F_PACK, F_UNPACK, F_FROM_MONT,
  F_TO_MONT, F_PACK_INTERNAL, F_LOAD_PACKED, F_STORE_PACKED, F_INV, F_INV_VARTIME, F_COUNT
};

// in: n x 4 operands x W limbs (words, where the operation reads words, in operand 0); out: n x W; flag: n
template <class LF, class Store, bool HAS_LAZY>
__global__ void __launch_bounds__(BLOCK) k_field(int op, const int32_t* in, int32_t* out, int32_t* flag, size_t n) {
  constexpr int W = Shape<LF>::W;
  constexpr bool X2 = Shape<LF>::X2;
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t* s = in + i * 4 * W;
  int32_t* o = out + i * W;
  LF a, b, c, d;
  ld_limbs(a, s);
  ld_limbs(b, s + W);
  ld_limbs(c, s + 2 * W);
  ld_limbs(d, s + 3 * W);
  int32_t fl = 0;
  switch (op) {
    case F_MUL: st_limbs(o, a * b); break;
    case F_SQR: st_limbs(o, a.sqr()); break;
    case F_MUL_SUB: st_limbs(o, LF::mul_sub(a, b, c, d)); break;
    case F_CARRY: st_limbs(o, a.carry()); break;
    case F_CANONICAL: st_limbs(o, a.canonical()); break;
    case F_IS_ZERO: fl = a.is_zero_mod_p(); break;
    case F_MAYBE_ZERO: fl = a.maybe_zero_mod_p(); break;
    case F_FROM_MONT: {
      Store w;
      ld_words(w, s);
      st_limbs(o, LF::from_mont256(w));
      break;
    }
    case F_TO_MONT: st_words(o, a.to_mont256()); break;
    case F_INV: st_limbs(o, f29_inv(a)); break;
    case F_INV_VARTIME: st_limbs(o, f29_inv_vartime(a)); break;
    default: break;
  }
  if constexpr (!X2) {
    switch (op) {
      case F_MUL2: st_limbs(o, LF::mul2(a, b, c, d)); break;
      case F_PACK: {
        Store w;
        a.pack(w.v);
        st_words(o, w);
        break;
      }
      case F_UNPACK: {
        Store w;
        ld_words(w, s);
        st_limbs(o, LF::unpack(w.v));
        break;
      }
      case F_PACK_INTERNAL: {
        Store w;
        a.pack_internal(w.v);
        st_words(o, w);
        break;
      }
      default: break;
    }
  }
  if constexpr (HAS_LAZY) {
    if (op == F_LOAD_PACKED) {
      Store w;
      ld_words(w, s);
      st_limbs(o, Lazy<Store>::load_packed(w));
    } else if (op == F_STORE_PACKED) {
      st_words(o, Lazy<Store>::store_packed(a));
    }
  }
  flag[i] = fl;
}

template <class LF, class Store, bool HAS_LAZY>
int run_field(int op, const int32_t* in, int32_t* out, int32_t* flag, size_t n) {
  constexpr int W = Shape<LF>::W;
  if (op < 0 || op >= F_COUNT) return -1;
  if (Shape<LF>::X2 && (op == F_MUL2 || op == F_PACK || op == F_UNPACK || op == F_PACK_INTERNAL)) return -1;
  if (!HAS_LAZY && (op == F_LOAD_PACKED || op == F_STORE_PACKED)) return -1;
  if (!n) return 0;
  Dev din, dout, dflag;
  ARITH_TRY(din.upload(in, n * 4 * W * sizeof(int32_t)));
  ARITH_TRY(dout.upload(nullptr, n * W * sizeof(int32_t)));
  ARITH_TRY(dflag.upload(nullptr, n * sizeof(int32_t)));
  G16_LAUNCH((k_field<LF, Store, HAS_LAZY>), ceil_div(n, BLOCK), BLOCK, 0, (hipStream_t)0, op, (const int32_t*)din.p,
             (int32_t*)dout.p, (int32_t*)dflag.p, n);
  ARITH_TRY(finish_launch());
  ARITH_TRY(dout.download(out, n * W * sizeof(int32_t)));
  return dflag.download(flag, n * sizeof(int32_t));
}

// ---- ec29.h ----------------------------------------------------------------------------------------
enum EcOp {
  E_MADD = 0, E_MADD_SELECT, E_MADD_RARE, E_ADD, E_DBL, E_DBL_AFFINE, E_NEG, E_FROM_AFFINE, E_TO_AFFINE,
  E_TO_AFFINE_VARTIME, E_AFFINE_FROM_MONT, E_XYZZ_TO_MONT, E_STORE_PACKED_AFFINE, E_LOAD_PACKED_AFFINE, E_CHAIN,
  E_COUNT
};

template <class LF> G16_HD void ld_xyzz(XYZZ29<LF>& a, const int32_t* s) {
  constexpr int W = Shape<LF>::W;
  ld_limbs(a.x, s);
  ld_limbs(a.y, s + W);
  ld_limbs(a.zz, s + 2 * W);
  ld_limbs(a.zzz, s + 3 * W);
}
template <class LF> G16_HD void st_xyzz(int32_t* d, const XYZZ29<LF>& a) {
  constexpr int W = Shape<LF>::W;
  st_limbs(d, a.x);
  st_limbs(d + W, a.y);
  st_limbs(d + 2 * W, a.zz);
  st_limbs(d + 3 * W, a.zzz);
}

// in: n x (acc: 4 W | q: 4 W | p: 2 W | p.inf) limbs -- Affine<F> words in the p slot for the two loads;
// out: n x 4 W (XYZZ29 limbs; Aff29 limbs or storage words from the front), E_CHAIN: n x 32 x 4 W;
// flag: special / handled / inf, by operation
template <class F>
__global__ void __launch_bounds__(BLOCK) k_ec29(int op, const int32_t* in, int32_t* out, int32_t* flag, size_t n) {
  using LF = typename Lazy<F>::type;
  using Acc = XYZZ29<LF>;
  constexpr int W = Shape<LF>::W, WORDS = Shape<LF>::WORDS;
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t* s = in + i * (10 * W + 1);
  int32_t* o = out + i * 4 * W * (op == E_CHAIN ? CHAIN_STEPS : 1);
  Acc acc, q;
  Aff29<LF> p;
  ld_xyzz(acc, s);
  ld_xyzz(q, s + 4 * W);
  ld_limbs(p.x, s + 8 * W);
  ld_limbs(p.y, s + 9 * W);
  p.inf = s[10 * W] != 0;
  int32_t fl = 0;
  switch (op) {
    case E_MADD:
      acc.madd(p);
      st_xyzz(o, acc);
      break;
    case E_MADD_SELECT: {
      bool special;
      st_xyzz(o, Acc::madd_select(acc, p, &special));
      fl = special;
      break;
    }
    case E_MADD_RARE: {  // Pp and R travel in the accumulator's x and y
      bool handled;
      st_xyzz(o, Acc::madd_rare(p, acc.x, acc.y, &handled));
      fl = handled;
      break;
    }
    case E_ADD:
      acc.add(q);
      st_xyzz(o, acc);
      break;
    case E_DBL:
      acc.dbl_in_place();
      st_xyzz(o, acc);
      break;
    case E_DBL_AFFINE: st_xyzz(o, Acc::dbl_affine(p)); break;
    case E_NEG: st_xyzz(o, acc.neg()); break;
    case E_FROM_AFFINE: st_xyzz(o, Acc::from_affine(p)); break;
    case E_TO_AFFINE:
    case E_TO_AFFINE_VARTIME: {
      Aff29<LF> r = op == E_TO_AFFINE ? acc.template to_affine<false>() : acc.template to_affine<true>();
      st_limbs(o, r.x);
      st_limbs(o + W, r.y);
      fl = r.inf;
      break;
    }
    case E_AFFINE_FROM_MONT:
    case E_LOAD_PACKED_AFFINE: {
      Affine<F> raw;
      ld_words(raw.x, s + 8 * W);
      ld_words(raw.y, s + 8 * W + WORDS);
      Aff29<LF> r = op == E_AFFINE_FROM_MONT ? affine_from_mont256<F>(raw) : load_packed_affine<F>(raw);
      st_limbs(o, r.x);
      st_limbs(o + W, r.y);
      fl = r.inf;
      break;
    }
    case E_XYZZ_TO_MONT: {
      XYZZ<F> r = xyzz_to_mont256<F>(acc);
      st_words(o, r.x);
      st_words(o + WORDS, r.y);
      st_words(o + 2 * WORDS, r.zz);
      st_words(o + 3 * WORDS, r.zzz);
      break;
    }
    case E_STORE_PACKED_AFFINE: {
      Affine<F> r = store_packed_affine<F>(p);
      st_words(o, r.x);
      st_words(o + WORDS, r.y);
      break;
    }
    case E_CHAIN:  // the accumulator after every step: madd p, add q, double, ...
      for (int step = 0; step < CHAIN_STEPS; ++step) {
        if (step % 3 == 0) acc.madd(p);
        else if (step % 3 == 1) acc.add(q);
        else acc.dbl_in_place();
        st_xyzz(o + step * 4 * W, acc);
      }
      break;
    default: break;
  }
  flag[i] = fl;
}

template <class F>
int run_ec29(int op, const int32_t* in, int32_t* out, int32_t* flag, size_t n) {
  constexpr int W = Shape<typename Lazy<F>::type>::W;
  if (op < 0 || op >= E_COUNT) return -1;
  if (!n) return 0;
  const size_t out_ints = n * 4 * W * (op == E_CHAIN ? CHAIN_STEPS : 1);
  Dev din, dout, dflag;
  ARITH_TRY(din.upload(in, n * (10 * W + 1) * sizeof(int32_t)));
  ARITH_TRY(dout.upload(nullptr, out_ints * sizeof(int32_t)));
  ARITH_TRY(dflag.upload(nullptr, n * sizeof(int32_t)));
  G16_LAUNCH(k_ec29<F>, ceil_div(n, BLOCK), BLOCK, 0, (hipStream_t)0, op, (const int32_t*)din.p, (int32_t*)dout.p,
             (int32_t*)dflag.p, n);
  ARITH_TRY(finish_launch());
  ARITH_TRY(dout.download(out, out_ints * sizeof(int32_t)));
  return dflag.download(flag, n * sizeof(int32_t));
}

// ---- field.h / ec.h (storage form, Montgomery R = 2^256) -------------------------------------------
template <class F>
__global__ void __launch_bounds__(BLOCK) k_fp_op(int op, const F* a, const F* b, F* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  F x = a[i], y = b ? b[i] : F::zero(), r;
  switch (op) {
    case 0: r = x * y; break;
    case 1: r = x + y; break;
    case 2: r = x - y; break;
    case 3: r = x.neg(); break;
    case 4: r = x.inv(); break;
    case 5: r = x.sqr(); break;
    case 6: {
      U256 u = x.to_canonical();
      for (int k = 0; k < 8; ++k) r.v[k] = u.v[k];
      break;
    }
    case 7: {
      U256 u;
      for (int k = 0; k < 8; ++k) u.v[k] = x.v[k];
      r = F::from_canonical(u);
      break;
    }
    case 8: r = x.dbl(); break;
    default: r = F::zero();
  }
  out[i] = r;
}

__global__ void __launch_bounds__(BLOCK) k_fq2_op(int op, const Fq2* a, const Fq2* b, Fq2* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  Fq2 x = a[i], y = b ? b[i] : Fq2::zero(), r;
  switch (op) {
    case 0: r = x * y; break;
    case 1: r = x + y; break;
    case 2: r = x - y; break;
    case 3: r = x.neg(); break;
    case 4: r = x.inv(); break;
    case 5: r = x.sqr(); break;
    default: r = Fq2::zero();
  }
  out[i] = r;
}

template <class F>
G16_HD XYZZ<F> scaled(const Affine<F>& p, const F& lam) {
  if (p.is_inf()) return XYZZ<F>::infinity();
  F l2 = lam.sqr(), l3 = l2 * lam;
  return XYZZ<F>{p.x * l2, p.y * l3, l2, l3};
}

// op 0: scaled(P,l1) + scaled(Q,l2) (add)   1: scaled(P,l1) madd Q   2: dbl scaled(P,l1)
// op 3: k * P (k = canonical 256-bit at `k`)  4: dbl_affine(P)         5: mul_u32(k[0])
template <class F>
__global__ void __launch_bounds__(BLOCK) k_ec_op(int op, const Affine<F>* P, const Affine<F>* Q, const F* l1, const F* l2, const U256* k,
                        Affine<F>* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  Affine<F> p = P[i], q = Q ? Q[i] : Affine<F>::infinity();
  F a = l1 ? l1[i] : F::one(), b = l2 ? l2[i] : F::one();
  XYZZ<F> r;
  switch (op) {
    case 0: r = scaled(p, a); r.add(scaled(q, b)); break;
    case 1: r = scaled(p, a); r.madd(q); break;
    case 2: r = scaled(p, a); r.dbl_in_place(); break;
    case 3: r = k ? scaled(p, a).mul(k[i]) : XYZZ<F>::infinity(); break;
    case 4: r = XYZZ<F>::dbl_affine(p); break;
    case 5: r = k ? scaled(p, a).mul_u32(k[i].v[0]) : XYZZ<F>::infinity(); break;
    default: r = XYZZ<F>::infinity();
  }
  out[i] = r.to_affine();
}

template <class F>
int run_fp_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (!n) return 0;
  Dev da, db, dout;
  ARITH_TRY(da.upload(a, n * sizeof(F)));
  if (b) ARITH_TRY(db.upload(b, n * sizeof(F)));
  ARITH_TRY(dout.upload(nullptr, n * sizeof(F)));
  G16_LAUNCH(k_fp_op<F>, ceil_div(n, BLOCK), BLOCK, 0, (hipStream_t)0, op, (const F*)da.p, (const F*)db.p, (F*)dout.p,
             n);
  ARITH_TRY(finish_launch());
  return dout.download(out, n * sizeof(F));
}

template <class F>
int run_ec_op(int op, const uint8_t* P, const uint8_t* Q, const uint8_t* l1, const uint8_t* l2, const uint8_t* k,
              uint8_t* out, size_t n) {
  if (!n) return 0;
  Dev dP, dQ, d1, d2, dk, dout;
  ARITH_TRY(dP.upload(P, n * sizeof(Affine<F>)));
  if (Q) ARITH_TRY(dQ.upload(Q, n * sizeof(Affine<F>)));
  if (l1) ARITH_TRY(d1.upload(l1, n * sizeof(F)));
  if (l2) ARITH_TRY(d2.upload(l2, n * sizeof(F)));
  if (k) ARITH_TRY(dk.upload(k, n * sizeof(U256)));
  ARITH_TRY(dout.upload(nullptr, n * sizeof(Affine<F>)));
  G16_LAUNCH(k_ec_op<F>, ceil_div(n, BLOCK), BLOCK, 0, (hipStream_t)0, op, (const Affine<F>*)dP.p,
             (const Affine<F>*)dQ.p, (const F*)d1.p, (const F*)d2.p, (const U256*)dk.p, (Affine<F>*)dout.p, n);
  ARITH_TRY(finish_launch());
  return dout.download(out, n * sizeof(Affine<F>));
}

// out: out_bytes the caller has filled (guard pattern and all); the kernel writes its slots into it
template <class F>
int run_to_affine(const uint8_t* work, uint32_t total, uint32_t n, uint32_t off0, uint32_t off1, uint32_t stride,
                  uint8_t* out, size_t out_bytes) {
  Dev dwork, dout;
  ARITH_TRY(dwork.upload(work, (size_t)total * sizeof(XYZZ<F>)));
  ARITH_TRY(dout.upload(out, out_bytes));
  xyzz_to_affine<F>((const XYZZ<F>*)dwork.p, total, n, off0, off1, stride, (uint8_t*)dout.p, (hipStream_t)0);
  ARITH_TRY(finish_launch());
  return dout.download(out, out_bytes);
}

}  // namespace

extern "C" {
// toaffine.h's launcher.  g2: 0 = Fq, 1 = Fq2.  Every slot must lie inside out_bytes: checked here, -2 if not.
int arith_to_affine(int g2, const uint8_t* work, uint32_t total, uint32_t n, uint32_t off0, uint32_t off1,
                    uint32_t stride, uint8_t* out, size_t out_bytes) {
  const size_t pt = g2 ? sizeof(G2Affine) : sizeof(G1Affine);
  const uint64_t lo = total < n ? total : n, hi = total > n ? total - n : 0;
  if (lo && (uint64_t)(lo - 1) * stride + off0 + pt > out_bytes) return -2;
  if (hi && (uint64_t)(hi - 1) * stride + off1 + pt > out_bytes) return -2;
  return g2 ? run_to_affine<Fq2>(work, total, n, off0, off1, stride, out, out_bytes)
            : run_to_affine<Fq>(work, total, n, off0, off1, stride, out, out_bytes);
}
// field: 0 = Fq29, 1 = Fr29, 2 = Fq2x29 (18 limbs per operand)
int arith_f29_op(int field, int op, const int32_t* in, int32_t* out, int32_t* flag, size_t n) {
  switch (field) {
    case 0: return run_field<Fq29, Fq, true>(op, in, out, flag, n);
    case 1: return run_field<Fr29, Fr, false>(op, in, out, flag, n);
    case 2: return run_field<Fq2x29, Fq2, true>(op, in, out, flag, n);
    default: return -1;
  }
}
// curve: 0 = G1XYZZ29, 1 = G2XYZZ29
int arith_ec29_op(int curve, int op, const int32_t* in, int32_t* out, int32_t* flag, size_t n) {
  switch (curve) {
    case 0: return run_ec29<Fq>(op, in, out, flag, n);
    case 1: return run_ec29<Fq2>(op, in, out, flag, n);
    default: return -1;
  }
}
int arith_fp_op(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  return field == 0 ? run_fp_op<Fr>(op, a, b, out, n) : run_fp_op<Fq>(op, a, b, out, n);
}
int arith_fq2_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (!n) return 0;
  Dev da, db, dout;
  ARITH_TRY(da.upload(a, n * sizeof(Fq2)));
  if (b) ARITH_TRY(db.upload(b, n * sizeof(Fq2)));
  ARITH_TRY(dout.upload(nullptr, n * sizeof(Fq2)));
  G16_LAUNCH(k_fq2_op, ceil_div(n, BLOCK), BLOCK, 0, (hipStream_t)0, op, (const Fq2*)da.p, (const Fq2*)db.p,
             (Fq2*)dout.p, n);
  ARITH_TRY(finish_launch());
  return dout.download(out, n * sizeof(Fq2));
}
int arith_g1_op(int op, const uint8_t* P, const uint8_t* Q, const uint8_t* l1, const uint8_t* l2, const uint8_t* k,
                uint8_t* out, size_t n) {
  return run_ec_op<Fq>(op, P, Q, l1, l2, k, out, n);
}
int arith_g2_op(int op, const uint8_t* P, const uint8_t* Q, const uint8_t* l1, const uint8_t* l2, const uint8_t* k,
                uint8_t* out, size_t n) {
  return run_ec_op<Fq2>(op, P, Q, l1, l2, k, out, n);
}
}
