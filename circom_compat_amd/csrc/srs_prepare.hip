// srs_prepare.hip -- prepared powers of tau (`snarkjs powersoftau prepare phase2`): the Lagrange sections 12-15 of a
// .ptau built (g16_srs_prepare) and checked against the monomial arrays (g16_srs_lagrange_check).  The layout of a
// Lagrange set, the algebra of the check and its soundness are in include/g16_amd.h; g16_setup_from_prepared, which
// USES a set, is setup_srs.hip's body with the transforms skipped.
//
// g16_srs_prepare: level by level (p = 0 .. P+1), the twiddle schedules of size 2^p once, then the group transform
// of gtransform.h on the first 2^p points of each array, the affine pass with the bit reversal folded in, and the
// download of the level.  Nothing but one level is resident.
//
// g16_srs_lagrange_check, per array (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1):
//   k_lc_rho_fr + ntt29_dif + k_lc_accum   C = sum_p iNTT_{2^p}(rho^(p)): the level's 128-bit coefficients as Fr,
//                                the inverse Fr transform of the witness map (ntt29.h, 1/2^p fused), and the
//                                bit-reversed result added into C[0 .. 2^p)
//   k_chk_flags_g1 / _g2         one reason byte per point: the predicates of keycheck.h (monomial G2 points: canonical
//                                and on the curve only -- the string is expected to have passed g16_srs_check)
//   k_lc_rho                     Lagrange side: one lane per point, rho P by a 128-step double-and-add of mixed
//                                additions on the lazy limbs of ec29.h, then the block's sum (kc_block_sum)
//   k_lc_coeff                   monomial side: one lane per point, C_i P by a NAF ladder over the full width
//   k_chk_fold                   one block: the chunk's block sums into the running sum of the side
//   k_chk_collect                one block: counts the flags, appends the bad points in index order (a scan)
// and once at the end k_lc_final: the two sums of every array compared as group elements (their difference is the
// point at infinity), the report and the bad-point list assembled on the device.  The arrays are STREAMED through
// the CheckStage of keycheck.h: two page-locked host slots and two device slots of `chunk` points, the copy of chunk
// k + 1 under the kernels of chunk k.  One synchronisation precedes the download of the report.  No atomics anywhere.
#include "gtransform.h"
#include "keycheck.h"
#include "ntt29.h"

namespace g16 {
namespace {

constexpr uint32_t LC_DEFAULT_CHUNK = 1u << 18;
constexpr uint32_t LC_N = G16_LAGRANGE_N_ARRAYS;

thread_local PhaseTimes<7> t_prepare;  // the phases of g16_setup_from_srs_times

struct LcState {  // device-resident for the whole call
  CheckTally tally;
  G1XYZZ29 sum1[3][2];  // [tau_g1, alpha_tau_g1, beta_tau_g1][Lagrange side, monomial side]
  G2XYZZ29 sum2[2];
  g16_srs_lagrange_report report;
};

// part[block] = sum over the block of rho_i P_i, rho_i = rho[2i] + 2^64 rho[2i + 1].  A malformed or infinite
// point is left out (the relations are not reported when a point is malformed).
template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_lc_rho(const Affine<F>* pts, const uint64_t* rho, const uint8_t* flags,
                                                     uint32_t n, XYZZ29<typename Lazy<F>::type>* part) {
  using P = XYZZ29<typename Lazy<F>::type>;
  __shared__ P sh[KC_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  P acc = P::infinity();
  if (i < n && !flags[i]) {
    const uint64_t lo = rho[2 * (size_t)i], hi = rho[2 * (size_t)i + 1];
    const Aff29<typename Lazy<F>::type> p = affine_from_mont256<F>(pts[i]);
#pragma unroll 1
    for (int b = 127; b >= 0; --b) {
      acc.dbl_in_place();
      const uint64_t w = b >= 64 ? hi : lo;
      if ((w >> (b & 63)) & 1) acc.madd(p);
    }
  }
  kc_block_sum(sh, acc);
  if (t == 0) part[blockIdx.x] = sh[0];
}

// part[block] = sum over the block of coeff[i] P_i, coeff full-width Montgomery Fr: the NAF ladder of comb_term
// (setup_srs.hip), mixed additions of +-P from the top word down
template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_lc_coeff(const Affine<F>* pts, const Fr* coeff, const uint8_t* flags,
                                                       uint32_t n, XYZZ29<typename Lazy<F>::type>* part) {
  using LF = typename Lazy<F>::type;
  using P = XYZZ29<LF>;
  __shared__ P sh[KC_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  P acc = P::infinity();
  if (i < n && !flags[i]) {
    const Aff29<LF> p = affine_from_mont256<F>(pts[i]);
    const Naf s = naf_of(coeff[i].to_canonical());
    const LF ny = p.y.neg().carry();
#pragma unroll 1
    for (int w = 7; w >= 0; --w) {
      const uint32_t pw = s.pos[w], nw = s.neg[w];
      if (!(pw | nw) && acc.is_inf()) continue;
#pragma unroll 1
      for (int b = 31; b >= 0; --b) {
        acc.dbl_in_place();
        const uint32_t m = 1u << b;
        if ((pw | nw) & m) acc.madd(Aff29<LF>{p.x, (nw & m) ? ny : p.y, false});
      }
    }
  }
  kc_block_sum(sh, acc);
  if (t == 0) part[blockIdx.x] = sh[0];
}

// rho (2 x u64, a plain integer < 2^128) -> Montgomery Fr
__global__ void __launch_bounds__(256) k_lc_rho_fr(const uint64_t* rho, uint32_t n, Fr* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = Fr::from_canonical(rho_u256(rho, i));
}

// c[bitrev_k(i)] += v[i]: the transform's output is bit-reversed; one lane per entry, every entry touched once
__global__ void __launch_bounds__(256) k_lc_accum(const Fr* v, uint32_t n, int k, Fr* c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = k > 0 ? __brev(i) >> (32 - k) : i;
  c[d] = c[d] + v[i];
}

// the sums of each array compared (their difference is the point at infinity), then the report and the list
__global__ void __launch_bounds__(KC_BLOCK) k_lc_final(LcState* st, const g16_key_bad_point* lists, uint32_t cap,
                                                       g16_key_bad_point* out_list) {
  __shared__ uint32_t sh_off[LC_N + 2];
  const bool bad = chk_offsets(&st->tally, LC_N, cap, sh_off);
  if (threadIdx.x == 0) {
    g16_srs_lagrange_report r;
    memset(&r, 0, sizeof r);
    r.relations_checked = bad ? 0 : 1;
    if (!bad) {
      for (uint32_t a = 0; a < 3; ++a) {
        G1XYZZ29 d = st->sum1[a][0];
        d.add(st->sum1[a][1].neg());
        const uint32_t q = a == 0 ? G16_SRS_Q_TAU_G1 : a == 1 ? G16_SRS_Q_ALPHA_TAU_G1 : G16_SRS_Q_BETA_TAU_G1;
        if (!d.is_inf()) r.relations_failed |= 1u << q;
      }
      G2XYZZ29 d2 = st->sum2[0];
      d2.add(st->sum2[1].neg());
      if (!d2.is_inf()) r.relations_failed |= 1u << G16_SRS_Q_TAU_G2;
    }
    r.ok = (!bad && !r.relations_failed) ? 1 : 0;
    chk_counts(&r, &st->tally, LC_N);
    r.n_listed = sh_off[LC_N];
    st->report = r;
  }
  chk_emit_lists(sh_off, LC_N, lists, cap, out_list);
}

struct LcArray {
  bool g2;
  uint32_t query, which;  // which: index into LcState::sum1
  int top;                // highest level
  const uint8_t* lag;     // the Lagrange section: 2^(top+1) - 1 points
  const uint8_t* mono;    // the monomial array
  uint64_t n_mono;        // monomial points that enter (the pad of tau_g1's top level does not)
};

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" {

g16_status g16_srs_prepare(int device, const g16_srs_desc* srs, uint32_t power, uint8_t* tau_g1_out,
                           uint8_t* tau_g2_out, uint8_t* alpha_tau_g1_out, uint8_t* beta_tau_g1_out) {
  if (!srs || !tau_g1_out || !tau_g2_out || !alpha_tau_g1_out || !beta_tau_g1_out) return G16_ERR_INVALID;
  if (power > 27) return G16_ERR_DOMAIN_TOO_LARGE;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  const uint32_t nP = 1u << power, n_top = 2 * nP;
  if ((uint64_t)srs->n_tau_g1 < (uint64_t)n_top - 1 || srs->n_tau < nP) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    t_prepare.clear();
    PhaseClock clk(t_prepare.ms, s);
    DevBuf<G1Affine> in1, o1;
    DevBuf<G2Affine> in2, o2;
    DevBuf<G1XYZZ29> w1;
    DevBuf<G2XYZZ29> w2;
    DevBuf<Fr> tmp;
    in1.alloc(n_top);
    o1.alloc(n_top);
    w1.alloc(n_top);
    in2.alloc(nP);
    o2.alloc(nP);
    w2.alloc(nP);
    tmp.alloc(nP);  // n / 2 scalars of the largest level
    const uint8_t* g1_src[3] = {srs->tau_g1, srs->alpha_tau_g1, srs->beta_tau_g1};
    uint8_t* g1_dst[3] = {tau_g1_out, alpha_tau_g1_out, beta_tau_g1_out};
    for (uint32_t p = 0; p <= power + 1; ++p) {
      const uint32_t n = 1u << p;
      const size_t at = (size_t)n - 1;  // the level's offset in points
      Twiddles T;
      build_twiddles(T, (int)p, false, tmp.p, s);
      clk.lap(0);
      for (int q = 0; q < 3; ++q) {
        if (q && p > power) break;  // only tau_g1 has level P+1
        const uint32_t have = p > power ? n - 1 : n;  // level P+1 reads M[2^(P+1) - 1] as infinity
        G16_HIP(hipMemcpyAsync(in1.p, g1_src[q], (size_t)have * 64, hipMemcpyHostToDevice, s));
        if (have < n) G16_HIP(hipMemsetAsync(in1.p + have, 0, 64, s));
        G16_LAUNCH((k_load_affine<Fq>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G1Affine*)in1.p, n, w1.p);
        clk.lap(0);
        group_intt<Fq29>(w1.p, (int)p, T, true, s);
        clk.lap(1);
        to_affine<Fq, false>(w1.p, n, (int)p, o1.p, s);
        clk.lap(4);
        G16_HIP(hipMemcpy(g1_dst[q] + at * 64, o1.p, (size_t)n * 64, hipMemcpyDeviceToHost));
        clk.lap(6);
      }
      if (p <= power) {
        G16_HIP(hipMemcpyAsync(in2.p, srs->tau_g2, (size_t)n * 128, hipMemcpyHostToDevice, s));
        G16_LAUNCH((k_load_affine<Fq2>), ceil_div(n, SS_BLOCK), SS_BLOCK, 0, s, (const G2Affine*)in2.p, n, w2.p);
        clk.lap(0);
        group_intt<Fq2x29>(w2.p, (int)p, T, true, s);
        clk.lap(2);
        to_affine<Fq2, false>(w2.p, n, (int)p, o2.p, s);
        clk.lap(4);
        G16_HIP(hipMemcpy(tau_g2_out + at * 128, o2.p, (size_t)n * 128, hipMemcpyDeviceToHost));
        clk.lap(6);
      }
    }
    return G16_OK;
  });
}

g16_status g16_srs_prepare_times(float* ms, uint32_t cap) {
  return t_prepare.read(ms, cap);
}

g16_status g16_srs_lagrange_check(int device, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                  const uint64_t* rho, g16_key_bad_point* bad_out, uint32_t bad_cap,
                                  g16_srs_lagrange_report* report) {
  if (!srs || !lag || !report || (bad_cap && !bad_out)) return G16_ERR_INVALID;
  if (lag->power > 27) return G16_ERR_DOMAIN_TOO_LARGE;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return G16_ERR_INVALID;
  if (!lag->tau_g1 || !lag->tau_g2 || !lag->alpha_tau_g1 || !lag->beta_tau_g1) return G16_ERR_INVALID;
  const uint32_t P = lag->power;
  const uint64_t nP = (uint64_t)1 << P, n_top = 2 * nP;
  if ((uint64_t)srs->n_tau_g1 < n_top - 1 || srs->n_tau < nP) return G16_ERR_INVALID;
  const uint64_t m1 = 2 * n_top - 1, m2 = n_top - 1;  // points of section 12 / of sections 13-15
  if (!rho_all_nonzero(rho, m1 + 3 * m2)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&]() -> g16_status {
    const uint32_t chunk = chunk_from_env("G16_LAGCHECK_CHUNK", LC_DEFAULT_CHUNK, m1);
    const uint32_t nb_max = ceil_div(chunk, KC_BLOCK);

    const LcArray arrays[LC_N] = {
        {false, G16_SRS_Q_TAU_G1, 0, (int)P + 1, lag->tau_g1, srs->tau_g1, n_top - 1},
        {true, G16_SRS_Q_TAU_G2, 0, (int)P, lag->tau_g2, srs->tau_g2, nP},
        {false, G16_SRS_Q_ALPHA_TAU_G1, 1, (int)P, lag->alpha_tau_g1, srs->alpha_tau_g1, nP},
        {false, G16_SRS_Q_BETA_TAU_G1, 2, (int)P, lag->beta_tau_g1, srs->beta_tau_g1, nP}};

    G16_HIP(hipSetDevice(device));
    std::unique_ptr<LcState> hs(new LcState());
    memset(hs.get(), 0, sizeof(LcState));
    uint64_t* n_points = hs->tally.n_points;
    n_points[G16_SRS_Q_TAU_G1] = m1;
    n_points[G16_SRS_Q_TAU_G2] = n_points[G16_SRS_Q_ALPHA_TAU_G1] = n_points[G16_SRS_Q_BETA_TAU_G1] = m2;

    // every allocation of the call but the transform plans: nothing else is allocated inside the loops
    const size_t off_rho = (size_t)chunk * 128;  // a slot: points | chunk coefficients
    CheckStage stage(off_rho + (size_t)chunk * 16, chunk, LC_N, bad_cap);
    DevBuf<LcState> dst;
    DevBuf<G1XYZZ29> dpart1;
    DevBuf<G2XYZZ29> dpart2;
    DevBuf<Fr> dC, dv;
    DevBuf<uint64_t> drho_lvl;
    DevBuf<int32_t> dplanes;
    dst.alloc(1);
    dpart1.alloc(nb_max);
    dpart2.alloc(nb_max);
    dC.alloc(n_top);
    dv.alloc(n_top);
    drho_lvl.alloc(2 * n_top);
    dplanes.alloc((size_t)NTT29_LIMBS * n_top);
    G16_HIP(hipMemcpy(dst.p, hs.get(), sizeof(LcState), hipMemcpyHostToDevice));
    const hipStream_t copy = stage.copy.s, comp = stage.comp.s;

    std::vector<uint64_t> drawn;  // the array's rho when the caller gave none
    const uint64_t* rho_at = rho;
    for (uint32_t a = 0; a < LC_N; ++a) {
      const LcArray& A = arrays[a];
      const uint64_t m = ((uint64_t)2 << A.top) - 1;
      const uint64_t* r = rho_at;
      if (!rho) {
        // the slots in flight do not read `drawn`, but the level uploads below do: they are synchronous
        drawn.resize(2 * m);
        if (!draw_rho(drawn.data(), (size_t)m)) {
          stage.drain();
          return G16_ERR_INTERNAL;
        }
        r = drawn.data();
      } else {
        rho_at += 2 * m;
      }

      // ---- C = sum_p iNTT_{2^p}(rho^(p)), on the compute stream behind the array before
      G16_HIP(hipMemsetAsync(dC.p, 0, ((size_t)1 << A.top) * sizeof(Fr), comp));
      for (int p = 0; p <= A.top; ++p) {
        const uint32_t n = 1u << p;
        Ntt29Plan plan;
        plan.build(p, comp);
        G16_HIP(hipMemcpyAsync(drho_lvl.p, r + 2 * ((size_t)n - 1), (size_t)n * 16, hipMemcpyHostToDevice, comp));
        G16_LAUNCH(k_lc_rho_fr, ceil_div(n, 256), 256, 0, comp, (const uint64_t*)drho_lvl.p, n, dv.p);
        ntt29_to_planes(dv.p, dplanes.p, n, comp);
        ntt29_dif(plan, dplanes.p, (size_t)NTT29_LIMBS * n, 1, true, NTT_FUSE_SCALE, comp);
        ntt29_from_planes(dplanes.p, dv.p, n, comp);
        G16_LAUNCH(k_lc_accum, ceil_div(n, 256), 256, 0, comp, (const Fr*)dv.p, n, p, dC.p);
        G16_HIP(hipStreamSynchronize(comp));  // the plan's tables are released at the end of this scope
      }

      // ---- the two sides: the Lagrange section under rho, then the monomial array under C
      for (int side = 0; side < 2; ++side) {
        const uint64_t total = side ? A.n_mono : m;
        const uint8_t* src = side ? A.mono : A.lag;
        const size_t w = A.g2 ? 128 : 64;
        for (uint64_t base = 0; base < total; base += chunk) {
          const uint32_t n = (uint32_t)(total - base < chunk ? total - base : chunk);
          const auto [h, d] = stage.begin();
          memcpy(h, src + base * w, (size_t)n * w);
          G16_HIP(hipMemcpyAsync(d, h, (size_t)n * w, hipMemcpyHostToDevice, copy));
          if (!side) {
            memcpy(h + off_rho, r + 2 * base, (size_t)n * 16);
            G16_HIP(hipMemcpyAsync(d + off_rho, h + off_rho, (size_t)n * 16, hipMemcpyHostToDevice, copy));
          }
          stage.staged();
          const uint32_t nb = ceil_div(n, KC_BLOCK);
          const uint64_t* drho = (const uint64_t*)(d + off_rho);
          const uint8_t* fl = stage.dflags.p;
          if (A.g2) {
            G16_LAUNCH(k_chk_flags_g2, nb, KC_BLOCK, 0, comp, (const VkDev*)stage.dvk.p, (const G2Affine*)d, n,
                       (uint32_t)(side ? 0 : 1), stage.dflags.p);  // monomial points: no subgroup test
            if (side)
              G16_LAUNCH((k_lc_coeff<Fq2>), nb, KC_BLOCK, 0, comp, (const G2Affine*)d, (const Fr*)(dC.p + base), fl, n,
                         dpart2.p);
            else
              G16_LAUNCH((k_lc_rho<Fq2>), nb, KC_BLOCK, 0, comp, (const G2Affine*)d, drho, fl, n, dpart2.p);
            G16_LAUNCH(k_chk_fold<G2XYZZ29>, 1, KC_BLOCK, 0, comp, (const G2XYZZ29*)dpart2.p, nb, 1u,
                       &dst.p->sum2[side]);
          } else {
            G16_LAUNCH(k_chk_flags_g1, nb, KC_BLOCK, 0, comp, (const G1Affine*)d, n, stage.dflags.p);
            if (side)
              G16_LAUNCH((k_lc_coeff<Fq>), nb, KC_BLOCK, 0, comp, (const G1Affine*)d, (const Fr*)(dC.p + base), fl, n,
                         dpart1.p);
            else
              G16_LAUNCH((k_lc_rho<Fq>), nb, KC_BLOCK, 0, comp, (const G1Affine*)d, drho, fl, n, dpart1.p);
            G16_LAUNCH(k_chk_fold<G1XYZZ29>, 1, KC_BLOCK, 0, comp, (const G1XYZZ29*)dpart1.p, nb, 1u,
                       &dst.p->sum1[A.which][side]);
          }
          if (!side)  // only the Lagrange points are counted and listed
            stage.collect(fl, n, A.query, A.query, (uint32_t)base, &dst.p->tally);
          stage.end();
        }
      }
      // `drawn` is overwritten for the next array: every copy out of it (pinned slots, level uploads) is done
    }
    G16_LAUNCH(k_lc_final, 1, KC_BLOCK, 0, comp, dst.p, (const g16_key_bad_point*)stage.dlists.p, stage.cap,
               stage.dout.p);
    stage.finish(hs.get(), dst.p, report, bad_out);
    return G16_OK;
  });
}

}  // extern "C"
