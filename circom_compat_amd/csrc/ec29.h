// ec29.h -- BN254 G1 / G2 accumulator arithmetic over the lazy 9 x 29-bit limbs of field29.h.
//
// Same group law and coordinates as ec.h (extended Jacobian XYZZ, a = 0; the results are group
// elements, hence identical to ark-ec's whatever the representation), re-derived with explicit
// limb/value bookkeeping so that no operation needs a modular correction:
//
//   products ("M class")        :  limbs 0..7 in [0, 2^29), value in (-p, 2p)
//   stored x                    :  limbs 0..7 in [-8, 2^29 + 8), |value| < 8 p
//   stored y                    :  limbs 0..7 in [-8, 2^29 + 8), |value| < 3 p
//   stored zz, zzz              :  M class
//
// The Fq2 squarings (F29x2::sqr, (c0 + c1)(c0 - c1)) multiply the carried SUM of the two components by their
// difference: with stored-class components that is limbs within [-4, 2^29 + 4) against +-(2^30 + 16), and
// values |c0^2 - c1^2| <= max(|c0|, |c1|)^2 < 100 p^2 for the Pp and R below -- the classes are unchanged.
//
// Every formula below lists the classes it produces; F29_CHECK (emulator build) asserts the
// column and value bounds on every product actually formed in the test-suite.
// The point at infinity is the exact all-zero limb pattern of zz (a valid zz is != 0 mod p, so it
// never has all-zero limbs).
#pragma once
#include "ec.h"
#include "field29.h"

namespace g16 {

template <class LF>
struct Aff29 {
  LF x, y;  // M class (loaded canonical)
  bool inf;
};

template <class LF>
struct XYZZ29 {
  LF x, y, zz, zzz;

  static G16_HD XYZZ29 infinity() { return XYZZ29{LF::zero(), LF::zero(), LF::zero(), LF::zero()}; }
  G16_HD bool is_inf() const { return zz.limbs_all_zero(); }
  static G16_HD XYZZ29 from_affine(const Aff29<LF>& p) {
    if (p.inf) return infinity();
    return XYZZ29{p.x, p.y, LF::one(), LF::one()};
  }
  G16_HD XYZZ29 neg() const { return XYZZ29{x, y.neg().carry(), zz, zzz}; }

  // mdbl-2008-s-1 on an affine point (rare path of madd)
  static G16_HD XYZZ29 dbl_affine(const Aff29<LF>& p) {
    if (p.inf) return infinity();
    LF U = p.y.dbl().carry();        // |v| < 4p
    LF V = U.sqr();                  // M
    LF W = U * V;                    // M
    LF S = p.x * V;                  // M
    LF X2 = p.x.sqr();               // M
    LF Mm = (X2.dbl() + X2).carry();  // |v| < 6p
    LF X3 = (Mm.sqr() - S.dbl()).carry();            // (-5p, 4p)
    // Y3: limbs of Mm in [-8, 2^29 + 8), of S - X3 within +-(2^29 + 8), W and p.y products (p.y possibly negated
    // and carried); values |Mm| < 6p, S - X3 in (-5p, 7p), |W| < 2p, |p.y| < 2p: 42 + 4 = 46 p^2 in G1, and per
    // component of Fq2 2 * 42 + 2 * 4 = 92 p^2 < 168.9 p^2 (mul4: 337 p^2)
    LF Y3 = LF::mul_sub_y3(Mm, S - X3, W, p.y);      // M
    return XYZZ29{X3, Y3, V, W};
  }
  // dbl-2008-s-1
  G16_HD void dbl_in_place() {
    if (is_inf()) return;
    LF U = y.dbl().carry();          // |v| < 6p
    LF V = U.sqr();                  // M
    LF W = U * V;                    // M
    LF S = x * V;                    // M
    LF X2 = x.sqr();                 // M
    LF Mm = (X2.dbl() + X2).carry();  // (-3p, 6p), limbs in [-8, 2^29 + 8)
    LF X3 = (Mm.sqr() - S.dbl()).carry();            // (-5p, 4p)
    // Y3: S - X3 in (-5p, 7p) with limbs within +-(2^29 + 8); W a product, y stored (limbs in [-8, 2^29 + 8),
    // |v| < 3p): 6 * 7 + 2 * 3 = 48 p^2 in G1, per component of Fq2 2 * 42 + 2 * 6 = 96 p^2 < 168.9 p^2
    // (mul4 allows 337 p^2): mul_sub_y3 would be inside its contract here.  NOT used: with the merged form in add
    // and dbl_in_place k_bucket_reduce<Fq2>, already at 512 registers, goes from 34 to 59 spilled VGPRs (80 to 156
    // bytes of scratch, profiles/r09_acc_diet_resource_usage.txt) -- the two keep mul_sub, the split form for Fq2.
    LF Y3 = LF::mul_sub(Mm, S - X3, W, y);
    zz = V * zz;
    zzz = W * zzz;
    x = X3;
    y = Y3;
  }
  // rare tail of madd: x(P) == x(Q) exactly?  Kept out of line so that the hot loop's register
  // allocation and instruction footprint do not pay for it.
  static G16_NOINLINE XYZZ29 madd_rare(Aff29<LF> p, LF Pp, LF R, bool* handled) {
    if (!Pp.is_zero_mod_p()) {
      *handled = false;
      return infinity();
    }
    *handled = true;
    if (R.is_zero_mod_p()) return dbl_affine(p);
    return infinity();
  }
  // madd-2008-s: this += affine p.  8M + 2S, one merged reduction for Y3 in G1.
  G16_HD void madd(const Aff29<LF>& p) {
    if (p.inf) return;
    if (is_inf()) {
      x = p.x;
      y = p.y;
      zz = LF::one();
      zzz = LF::one();
      return;
    }
    LF U2 = p.x * zz;   // M
    LF S2 = p.y * zzz;  // M
    LF Pp = U2 - x;     // limbs within +-(2^29+8); |v| < 10p
    LF R = S2 - y;      // same; |v| < 10p
    if (Pp.maybe_zero_mod_p()) {  // ~2^-23 of the calls: exact test and the P = +-Q cases, out of line
      bool handled;
      XYZZ29 r = madd_rare(p, Pp, R, &handled);
      if (handled) {
        *this = r;
        return;
      }
    }
    LF PP = Pp.sqr();                              // M
    LF PPP = Pp * PP;                              // M
    LF Q = x * PP;                                 // M
    LF X3 = (R.sqr() - PPP - Q.dbl()).carry();     // S: (-7p, 5p)
    // Y3: |R| < 10p against Q - X3 in (-6p, 9p), |y| < 3p against |PPP| < 2p: 96 p^2 in G1, per component of Fq2
    // 2 * 90 + 2 * 6 = 192 p^2 < 337 p^2 (mul4); all limbs within +-(2^29 + 8)
    LF Y3 = LF::mul_sub_y3(R, Q - X3, y, PPP);     // M (stored-y class for Fq2: (-2p, 3p))
    zz = zz * PP;
    zzz = zzz * PPP;
    x = X3;
    y = Y3;
  }
  // The general formula of madd alone: no infinity test, no select, no branch (the accumulation loop of
  // msm_curve.inc.h keeps the infinity cases out of its per-iteration path).  PRECONDITION for a meaningful result:
  // neither operand is infinite.  *x_may_coincide reports the 2^-23 filter on Pp (the caller then redoes the
  // addition exactly, or defers it).  Infinite operands have all-zero coordinates and a dead lane hands in a stale
  // finite point: every product formed then has a zero or an in-class factor, so the column and value bounds hold
  // whatever comes in (F29_CHECK sees those calls too); the result is simply not a group element.
  static G16_HD XYZZ29 madd_core(const XYZZ29& acc, const Aff29<LF>& p, bool* x_may_coincide) {
    LF U2 = p.x * acc.zz;   // M
    LF S2 = p.y * acc.zzz;  // M
    LF Pp = U2 - acc.x;     // limbs within +-(2^29+8); |v| < 10p
    LF R = S2 - acc.y;      // same
    *x_may_coincide = Pp.maybe_zero_mod_p();
    LF PP = Pp.sqr();
    LF PPP = Pp * PP;
    LF Q = acc.x * PP;
    LF X3 = (R.sqr() - PPP - Q.dbl()).carry();       // (-7p, 5p)
    LF Y3 = LF::mul_sub_y3(R, Q - X3, acc.y, PPP);   // as in madd: 192 p^2 per component of Fq2
    return XYZZ29{X3, Y3, acc.zz * PP, acc.zzz * PPP};
  }
  // The exact answer for an addition that madd_core flagged (same precondition): res = madd_core(acc, p) unless the
  // x-coordinates really coincide -- then the doubling or the point at infinity, exactly what madd() returns (its
  // formula is madd_core's).  Forms Pp and R again (two products on a 2^-23 path) and shares madd()'s out-of-line
  // tail, so the caller's loop holds ONE copy of the general formula: with w.acc.madd(p) in its place the G2
  // accumulation kernel grew from 7.7 K to 12.1 K instructions and from 90 to 190 AGPRs
  // (profiles/r09_acc_diet_resource_usage.txt).
  static G16_HD XYZZ29 madd_resolve(const XYZZ29& acc, const Aff29<LF>& p, const XYZZ29& res) {
    LF Pp = p.x * acc.zz - acc.x;
    LF R = p.y * acc.zzz - acc.y;
    bool handled;
    XYZZ29 r = madd_rare(p, Pp, R, &handled);
    return handled ? r : res;
  }
  // Branch-free madd for software-pipelined callers (two independent additions per lane
  // in ONE basic block so the scheduler can interleave their dependent multiply chains):
  // returns acc + p by the general formula and reports through *special when the x-coordinates
  // may coincide (~2^-23 of calls: the caller then redoes this addition with madd()).  The
  // infinity cases are resolved by selects, not branches.
  static G16_HD XYZZ29 madd_select(const XYZZ29& acc, const Aff29<LF>& p, bool* special) {
    const bool acc_inf = acc.is_inf();
    bool x_may_coincide;
    // an infinite accumulator has all-zero coordinates: harmless to the formulas
    XYZZ29 r = madd_core(acc, p, &x_may_coincide);
    *special = !acc_inf && !p.inf && x_may_coincide;
    if (acc_inf) r = XYZZ29{p.x, p.y, LF::one(), LF::one()};
    if (p.inf) r = acc;
    return r;
  }
  // add-2008-s: this += q.  12M + 2S
  G16_HD void add(const XYZZ29& q) {
    if (q.is_inf()) return;
    if (is_inf()) {
      *this = q;
      return;
    }
    LF U1 = x * q.zz;
    LF U2 = q.x * zz;
    LF S1 = y * q.zzz;
    LF S2 = q.y * zzz;
    LF Pp = U2 - U1;  // limbs in (-2^29, 2^29), |v| < 3p
    LF R = S2 - S1;
    if (Pp.is_zero_mod_p()) {
      if (R.is_zero_mod_p()) {
        dbl_in_place();
      } else {
        *this = infinity();
      }
      return;
    }
    LF PP = Pp.sqr();
    LF PPP = Pp * PP;
    LF Q = U1 * PP;
    LF X3 = (R.sqr() - PPP - Q.dbl()).carry();
    // Y3: Pp, R differences of two products: limbs in (-2^29, 2^29), |v| < 3p; X3 in (-7p, 5p) carried, so Q - X3
    // in (-6p, 9p) with limbs within +-(2^29 + 8); S1, PPP products: 3 * 9 + 2 * 2 = 31 p^2 in G1, per component
    // of Fq2 2 * 27 + 2 * 4 = 62 p^2 < 168.9 p^2 (mul4 allows 337 p^2): inside mul_sub_y3's contract, but mul_sub
    // stays (see dbl_in_place: the registers of k_bucket_reduce<Fq2>)
    LF Y3 = LF::mul_sub(R, Q - X3, S1, PPP);
    zz = (zz * q.zz) * PP;
    zzz = (zzz * q.zzz) * PPP;
    x = X3;
    y = Y3;
  }
  // x = X/ZZ, y = Y/ZZZ (one inversion), result canonical in the INTERNAL Montgomery form.
  // VARTIME: binary-GCD inversion (single-lane callers only, see f29_inv_vartime)
  template <bool VARTIME = false>
  G16_HD Aff29<LF> to_affine() const {
    if (is_inf()) return Aff29<LF>{LF::zero(), LF::zero(), true};
    LF iz3 = VARTIME ? f29_inv_vartime(zzz) : f29_inv(zzz);
    LF iz2 = iz3.sqr() * zz.sqr();
    return Aff29<LF>{(x * iz2).canonical(), (y * iz3).canonical(), false};
  }
};

// ---- HBM forms ---------------------------------------------------------------------------------
// precomputed points: Affine<F> containers holding the PACKED INTERNAL form (see Lazy<F>);
// all-zero = infinity, as in the reference's encoding (src/zkey.rs:343-348).
template <class F>
G16_HD Aff29<typename Lazy<F>::type> load_packed_affine(const Affine<F>& raw) {
  using LF = typename Lazy<F>::type;
  Aff29<LF> p;
  p.inf = raw.is_inf();
  p.x = Lazy<F>::load_packed(raw.x);
  p.y = Lazy<F>::load_packed(raw.y);
  return p;
}
template <class F>
G16_HD Affine<F> store_packed_affine(const Aff29<typename Lazy<F>::type>& p) {
  if (p.inf) return Affine<F>::infinity();
  return Affine<F>{Lazy<F>::store_packed(p.x), Lazy<F>::store_packed(p.y)};
}
// storage form (Montgomery-256 affine, the zkey encoding) -> lazy registers
template <class F>
G16_HD Aff29<typename Lazy<F>::type> affine_from_mont256(const Affine<F>& a) {
  using LF = typename Lazy<F>::type;
  if (a.is_inf()) return Aff29<LF>{LF::zero(), LF::zero(), true};
  return Aff29<LF>{LF::from_mont256(a.x), LF::from_mont256(a.y), false};
}
// lazy accumulator -> legacy XYZZ in storage form (what finalize.hip consumes)
template <class F>
G16_HD XYZZ<F> xyzz_to_mont256(const XYZZ29<typename Lazy<F>::type>& a) {
  if (a.is_inf()) return XYZZ<F>::infinity();
  return XYZZ<F>{a.x.to_mont256(), a.y.to_mont256(), a.zz.to_mont256(), a.zzz.to_mont256()};
}

using G1XYZZ29 = XYZZ29<Fq29>;
using G2XYZZ29 = XYZZ29<Fq2x29>;

}  // namespace g16
