// contribute.hip -- phase-2 delta contributions: apply one (g16_key_contribute) and verify one
// (g16_key_contribution_check).  What `snarkjs zkey contribute` does to the points of a key and what the
// sameRatio part of `snarkjs zkey verify` checks of them; the section-10 transcript is NOT handled
// (include/g16_amd.h).
//
// g16_key_contribute: delta1' = d delta1, delta2' = d delta2 (two points: on the host, the same field classes),
// and every point of the L and H queries times d^-1 -- the streamed part.  Per chunk of `chunk` points:
//   k_ct_mul     one lane per point: e P for the full-width e = d^-1, the same for every lane.  e is recoded
//                ONCE on the host into its non-adjacent form (digits 0 / +1 / -1, two bit masks read by
//                wave-uniform scalar loads): 254 doublings and ~85 MIXED additions of +-P (8M + 2S each, P
//                stays affine in registers).  No per-lane table: a window of w bits would trade these for
//                2^(w-2) full XYZZ additions (12M + 2S) plus 1 KiB of table per lane, which is scratch.
//                No divergence: the digit schedule is uniform, only lanes at infinity idle.
//   k_xyzz_to_affine  (toaffine.h) back to canonical affine with ONE Fermat inversion per run of 8 points
//                (Montgomery's trick down each lane's run): 3 multiplications per point instead of ~380.
// Two page-locked host slots and two device slots; chunk k + 1 is staged and copied while the kernels of chunk k
// run, and the results of chunk k come back on a third stream under the kernels of chunk k + 1.
//
// g16_key_contribution_check: keycheck.hip's structure on the points a contribution changes.  Per chunk of a
// query (L or H), the AFTER points, the BEFORE points and rho side by side in one slot:
//   k_chk_flags_g1  reason byte per AFTER point    k_cc_rho / k_chk_fold  sum rho_i P_i over both sides
//   k_chk_collect   counts / lists the bad points by a scan (no atomics)
//   k_cc_final      six Miller loops, three final exponentiations, the report and the list.
// The flag, fold and collect kernels, the halves of the final kernel and the staging are those of keycheck.h.
#include "keycheck.h"
#include "toaffine.h"

namespace g16 {
namespace {

constexpr uint32_t CT_DEFAULT_CHUNK = 1u << 18;
constexpr uint32_t CC_SLOT_BYTES_PER_POINT = 64 + 64 + 16;  // AFTER | BEFORE | rho

// e = sum (pos_i - neg_i) 2^i, non-adjacent; top = index of the leading digit (always +1)
struct CtSched {
  uint32_t pos[8], neg[8];
  int32_t top;
};

// non-adjacent form of a canonical e, 0 < e < r < 2^254: at most 255 digits
CtSched naf_of(const U256& e) {
  CtSched s;
  memset(&s, 0, sizeof s);
  uint32_t k[9];
  for (int i = 0; i < 8; ++i) k[i] = e.v[i];
  k[8] = 0;
  s.top = -1;
  for (int bit = 0; bit < 256; ++bit) {
    if (k[0] & 1) {
      if ((k[0] & 3) == 3) {  // digit -1: k += 1
        s.neg[bit >> 5] |= 1u << (bit & 31);
        for (int i = 0; i < 9 && ++k[i] == 0; ++i) {
        }
      } else {  // digit +1: k -= 1
        s.pos[bit >> 5] |= 1u << (bit & 31);
        k[0] &= ~1u;
        s.top = bit;
      }
    }
    for (int i = 0; i < 8; ++i) k[i] = (k[i] >> 1) | (k[i + 1] << 31);
    k[8] >>= 1;
  }
  return s;
}

// ---- g16_key_contribute ------------------------------------------------------------------------------
__global__ void __launch_bounds__(KC_BLOCK) k_ct_mul(const G1Affine* pts, uint32_t n, const CtSched* sched,
                                                     G1XYZZ* work) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G1Affine p = pts[i];
  const G1Affine np = p.neg();
  G1XYZZ acc = G1XYZZ::from_affine(p);  // the leading digit
#pragma unroll 1
  for (int b = sched->top - 1; b >= 0; --b) {
    acc.dbl_in_place();
    const uint32_t m = 1u << (b & 31);
    if (sched->pos[b >> 5] & m) {
      acc.madd(p);
    } else if (sched->neg[b >> 5] & m) {
      acc.madd(np);
    }
  }
  work[i] = acc;
}

// ---- g16_key_contribution_check ----------------------------------------------------------------------
enum { CC_L = 0, CC_H = 1, CC_SINGLES = 2, CC_N = 3 };
constexpr uint32_t CC_QUERY_ID[CC_N] = {G16_KEY_Q_L, G16_KEY_Q_H, G16_KEY_Q_SINGLES};

struct CcKey {
  G1Affine delta_g1_after, g1_neg;
  G2Affine delta_g2_before, delta_g2_after, g2;
};

struct CcState {  // device-resident for the whole call
  CheckTally tally;  // slots CC_L, CC_H, CC_SINGLES
  G1XYZZ sum[2][2];  // [L, H][before, after]: sum rho_i P_i so far
  g16_contribution_report report;
};

// blockIdx.y = 0: part[block] = sum over the block of rho_i BEFORE_i; 1: part[nb + block] = the same over AFTER.
// Entry i is left out on both sides when AFTER_i is malformed: the relations are not reported then anyway.
__global__ void __launch_bounds__(KC_BLOCK) k_cc_rho(const G1Affine* before, const G1Affine* after, const uint64_t* rho,
                                                     const uint8_t* flags, uint32_t n, G1XYZZ* part) {
  __shared__ G1XYZZ sh[KC_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  G1XYZZ acc = G1XYZZ::infinity();
  if (i < n && !(flags[i] & ~KC_INF))
    acc = mul_rho((blockIdx.y ? after : before)[i], rho[2 * (size_t)i], rho[2 * (size_t)i + 1]);
  kc_block_sum(sh, acc);
  if (t == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// lanes 0..5: ML(g2, delta1') ML(delta2', -g1) | ML(delta2, S_L) ML(delta2', -S_L') | the same for H;
// lanes 0..2: product and final exponentiation of one pair each; then the report and the list.
// Nothing is paired when a structural check failed.
__global__ void __launch_bounds__(KC_BLOCK) k_cc_final(const VkDev* vk, const CcKey* key, CcState* st,
                                                       const g16_key_bad_point* lists, uint32_t cap, uint32_t mismatch,
                                                       g16_key_bad_point* out_list) {
  __shared__ F12 sh[6];
  __shared__ uint32_t sh_fail[3];
  __shared__ uint32_t sh_off[CC_N + 2];
  const uint32_t t = threadIdx.x;
  const bool pair = !chk_offsets(&st->tally, CC_N, cap, sh_off);
  G2Affine Q = G2Affine::infinity();
  G1Affine P = G1Affine::infinity();
  if (pair && t < 6) {
    if (t == 0) {
      Q = key->g2;
      P = key->delta_g1_after;
    } else if (t == 1) {
      Q = key->delta_g2_after;
      P = key->g1_neg;
    } else {
      const uint32_t q = (t - 2) >> 1, side = t & 1;
      Q = side ? key->delta_g2_after : key->delta_g2_before;
      P = st->sum[q][side].to_affine();
      if (side) P = P.neg();
    }
  }
  const uint32_t failed = chk_pairs(Q, P, 3, pair, vk, sh, sh_fail);
  if (t == 0) {
    g16_contribution_report r;
    memset(&r, 0, sizeof r);
    r.relations_checked = pair ? 1 : 0;
    r.relations_failed = mismatch ? G16_CONTRIB_UNCHANGED_MISMATCH : 0;
    if (pair) {
      r.relations_failed |= failed * G16_CONTRIB_PAIR_DELTA;  // pairs 0, 1, 2: G16_CONTRIB_PAIR_DELTA, _L, _H
      if (key->delta_g1_after.is_inf() || key->delta_g2_after.is_inf()) r.relations_failed |= G16_CONTRIB_DELTA_INFINITE;
    }
    r.ok = (pair && !r.relations_failed) ? 1 : 0;
    r.n_bad_l = st->tally.n_bad[CC_L];
    r.n_bad_h = st->tally.n_bad[CC_H];
    r.n_listed = sh_off[CC_N];
    st->report = r;
  }
  chk_emit_lists(sh_off, CC_N, lists, cap, out_list);
}

// ---- host side -------------------------------------------------------------------------------------
bool key_shape_ok(const g16_key_desc* k) {
  if (!k || k->n_vars < 1 || (uint64_t)k->n_public + 1 > k->n_vars) return false;
  const uint64_t n_l = (uint64_t)k->n_vars - k->n_public - 1;
  return !(n_l && !k->l_query) && !(k->domain_size && !k->h_query);
}

struct CtItem {
  const uint8_t* src;
  uint8_t* dst;
  uint32_t count;
};

enum { CCK_PAIR = 0, CCK_G1 = 1, CCK_G2 = 2 };
struct CcItem {
  int kind;
  uint32_t q, base, count;
  const uint8_t* after;
  const uint8_t* before;
  const uint64_t* rho;  // NULL: drawn into the slot
};

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" g16_status g16_key_contribute(int device, const g16_key_desc* key, const uint64_t d[4], uint8_t* l_out,
                                         uint8_t* h_out, uint8_t delta_g1_out[64], uint8_t delta_g2_out[128]) {
  if (!key_shape_ok(key) || !delta_g1_out || !delta_g2_out) return G16_ERR_INVALID;
  const uint64_t n_l = (uint64_t)key->n_vars - key->n_public - 1, dom = key->domain_size;
  if ((n_l && !l_out) || (dom && !h_out)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;

  // every copy of d and of what is derived from it lives in this struct and is wiped on every way out
  struct Secret {
    Fr d, d_inv;
    U256 dc, ec;
    CtSched sched;
    ~Secret() { wipe(this, sizeof *this); }
  } sec;
  if (d) {
    memcpy(&sec.d, d, 32);
    if (!fr_words_canonical(sec.d) || sec.d.is_zero()) return G16_ERR_INVALID;
  } else if (!FrPool().draw_fr(&sec.d, true)) {
    return G16_ERR_INTERNAL;  // never a fixed fallback
  }
  sec.d_inv = sec.d.inv();
  sec.dc = sec.d.to_canonical();
  sec.ec = sec.d_inv.to_canonical();
  sec.sched = naf_of(sec.ec);

  return guarded_call([&]() -> g16_status {
    G1Affine d1;
    G2Affine d2;
    memcpy(&d1, key->delta_g1, 64);
    memcpy(&d2, key->delta_g2, 128);
    const G1Affine nd1 = G1XYZZ::from_affine(d1).mul(sec.dc).to_affine();
    const G2Affine nd2 = G2XYZZ::from_affine(d2).mul(sec.dc).to_affine();

    const uint32_t chunk = chunk_from_env("G16_CONTRIB_CHUNK", CT_DEFAULT_CHUNK, n_l > dom ? n_l : dom);
    std::vector<CtItem> items;
    for (uint64_t at = 0; at < n_l; at += chunk)
      items.push_back(CtItem{key->l_query + at * 64, l_out + at * 64, (uint32_t)(n_l - at < chunk ? n_l - at : chunk)});
    for (uint64_t at = 0; at < dom; at += chunk)
      items.push_back(CtItem{key->h_query + at * 64, h_out + at * 64, (uint32_t)(dom - at < chunk ? dom - at : chunk)});

    G16_HIP(hipSetDevice(device));
    // every allocation of the call: nothing is allocated inside the chunk loop
    const size_t slot_bytes = (size_t)chunk * 64;
    PinnedBuf pin[2];
    DevBuf<uint8_t> dslot[2];
    DevBuf<G1XYZZ> dwork;
    DevBuf<CtSched> dsched;
    StreamBox copy, comp, down;
    EventBox copied[2], computed[2], done[2];
    for (int s = 0; s < 2; ++s) {
      pin[s].alloc(slot_bytes);
      dslot[s].alloc(slot_bytes);
      copied[s].create();
      computed[s].create();
      done[s].create();
    }
    dwork.alloc(chunk);
    dsched.alloc(1);
    copy.create();
    comp.create();
    down.create();
    G16_HIP(hipMemcpy(dsched.p, &sec.sched, sizeof(CtSched), hipMemcpyHostToDevice));

    for (size_t k = 0; k < items.size() + 2; ++k) {
      const int s = (int)(k & 1);
      if (k >= 2) {  // the results of the chunk that used this slot two chunks ago
        G16_HIP(hipEventSynchronize(done[s].e));
        memcpy(items[k - 2].dst, pin[s].p, (size_t)items[k - 2].count * 64);
      }
      if (k >= items.size()) continue;
      const CtItem& it = items[k];
      const uint32_t n = it.count;
      const size_t bytes = (size_t)n * 64;
      uint8_t* dv = dslot[s].p;
      memcpy(pin[s].p, it.src, bytes);
      G16_HIP(hipMemcpyAsync(dv, pin[s].p, bytes, hipMemcpyHostToDevice, copy.s));
      G16_HIP(hipEventRecord(copied[s].e, copy.s));
      G16_HIP(hipStreamWaitEvent(comp.s, copied[s].e, 0));
      G16_LAUNCH(k_ct_mul, ceil_div(n, KC_BLOCK), KC_BLOCK, 0, comp.s, (const G1Affine*)dv, n,
                 (const CtSched*)dsched.p, dwork.p);
      xyzz_to_affine<Fq>(dwork.p, n, (G1Affine*)dv, comp.s);
      G16_HIP(hipEventRecord(computed[s].e, comp.s));
      G16_HIP(hipStreamWaitEvent(down.s, computed[s].e, 0));
      G16_HIP(hipMemcpyAsync(pin[s].p, dv, bytes, hipMemcpyDeviceToHost, down.s));
      G16_HIP(hipEventRecord(done[s].e, down.s));
    }
    G16_HIP(hipMemsetAsync(dsched.p, 0, sizeof(CtSched), comp.s));  // the recoded d^-1 does not outlive the call
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(comp.s));
    G16_HIP(hipStreamSynchronize(down.s));
    memcpy(delta_g1_out, &nd1, 64);
    memcpy(delta_g2_out, &nd2, 128);
    return G16_OK;
  });
}

extern "C" g16_status g16_key_contribution_check(int device, const g16_key_desc* before, const g16_key_desc* after,
                                                 const uint64_t* rho, g16_key_bad_point* bad_out, uint32_t bad_cap,
                                                 g16_contribution_report* report) {
  if (!report || (bad_cap && !bad_out) || !key_shape_ok(before) || !key_shape_ok(after)) return G16_ERR_INVALID;
  if (!before->a_query || !before->b_g1_query || !before->b_g2_query || !after->a_query || !after->b_g1_query ||
      !after->b_g2_query)
    return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  memset(report, 0, sizeof *report);
  // 1. what a contribution must leave alone: compared as bytes on the host
  if (before->n_vars != after->n_vars || before->n_public != after->n_public ||
      before->domain_size != after->domain_size) {
    report->relations_failed = G16_CONTRIB_UNCHANGED_MISMATCH;  // not the same key: nothing to pair entry by entry
    return G16_OK;
  }
  const uint64_t N = before->n_vars, n_l = N - before->n_public - 1, dom = before->domain_size;
  if (!rho_all_nonzero(rho, n_l + dom)) return G16_ERR_INVALID;
  const uint32_t mismatch =
      (memcmp(before->alpha_g1, after->alpha_g1, 64) || memcmp(before->beta_g1, after->beta_g1, 64) ||
       memcmp(before->beta_g2, after->beta_g2, 128) || memcmp(before->a_query, after->a_query, N * 64) ||
       memcmp(before->b_g1_query, after->b_g1_query, N * 64) || memcmp(before->b_g2_query, after->b_g2_query, N * 128))
          ? 1
          : 0;
  return guarded_call([&]() -> g16_status {
    const uint32_t chunk = chunk_from_env("G16_CONTRIB_CHUNK", CT_DEFAULT_CHUNK, n_l > dom ? n_l : dom);
    const uint32_t nb_max = ceil_div(chunk, KC_BLOCK);

    std::vector<CcItem> items;
    auto add_pairs = [&](uint32_t q, const uint8_t* a, const uint8_t* b, uint64_t count, const uint64_t* r) {
      for (uint64_t at = 0; at < count; at += chunk)
        items.push_back(CcItem{CCK_PAIR, q, (uint32_t)at, (uint32_t)(count - at < chunk ? count - at : chunk),
                               a + at * 64, b + at * 64, r ? r + 2 * at : nullptr});
    };
    add_pairs(CC_L, after->l_query, before->l_query, n_l, rho);
    add_pairs(CC_H, after->h_query, before->h_query, dom, rho ? rho + 2 * n_l : nullptr);
    // the single points under the indices g16_key_check gives them
    items.push_back(CcItem{CCK_G1, CC_SINGLES, 2, 1, after->delta_g1, nullptr, nullptr});
    items.push_back(CcItem{CCK_G2, CC_SINGLES, 4, 1, after->delta_g2, nullptr, nullptr});

    G16_HIP(hipSetDevice(device));
    CcKey hk;
    memcpy(&hk.delta_g1_after, after->delta_g1, 64);
    memcpy(&hk.delta_g2_before, before->delta_g2, 128);
    memcpy(&hk.delta_g2_after, after->delta_g2, 128);
    hk.g1_neg = G1Affine{Fq::one(), Fq::from_u32(2)}.neg();
    memcpy(&hk.g2, G2_GEN_WORDS, 128);
    std::unique_ptr<CcState> hs(new CcState());
    memset(hs.get(), 0, sizeof(CcState));

    size_t slot_bytes = (size_t)chunk * CC_SLOT_BYTES_PER_POINT;
    if (slot_bytes < 128) slot_bytes = 128;  // delta_g2 alone
    CheckStage stage(slot_bytes, chunk, CC_N, bad_cap);
    DevBuf<CcKey> dkey;
    DevBuf<CcState> dst;
    DevBuf<G1XYZZ> dpart;
    dkey.alloc(1);
    dst.alloc(1);
    dpart.alloc(2 * (size_t)nb_max);
    G16_HIP(hipMemcpy(dkey.p, &hk, sizeof hk, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dst.p, hs.get(), sizeof(CcState), hipMemcpyHostToDevice));
    const hipStream_t copy = stage.copy.s, comp = stage.comp.s;
    uint8_t* flags = stage.dflags.p;

    const size_t off_before = (size_t)chunk * 64, off_rho = (size_t)chunk * 128;
    for (const CcItem& it : items) {
      const auto [h, dv] = stage.begin();
      const uint32_t n = it.count;
      const uint32_t nb = ceil_div(n, KC_BLOCK);
      if (it.kind == CCK_PAIR) {
        memcpy(h, it.after, (size_t)n * 64);
        memcpy(h + off_before, it.before, (size_t)n * 64);
        uint64_t* hr = (uint64_t*)(h + off_rho);
        if (it.rho) {
          memcpy(hr, it.rho, (size_t)n * 16);
        } else if (!draw_rho(hr, n)) {  // drawn chunk by chunk, straight into the staging slot
          stage.drain();
          return G16_ERR_INTERNAL;
        }
        G16_HIP(hipMemcpyAsync(dv, h, (size_t)n * 64, hipMemcpyHostToDevice, copy));
        G16_HIP(hipMemcpyAsync(dv + off_before, h + off_before, (size_t)n * 64, hipMemcpyHostToDevice, copy));
        G16_HIP(hipMemcpyAsync(dv + off_rho, h + off_rho, (size_t)n * 16, hipMemcpyHostToDevice, copy));
      } else {
        const size_t bytes = (size_t)n * (it.kind == CCK_G2 ? 128 : 64);
        memcpy(h, it.after, bytes);
        G16_HIP(hipMemcpyAsync(dv, h, bytes, hipMemcpyHostToDevice, copy));
      }
      stage.staged();
      if (it.kind == CCK_G2) {
        G16_LAUNCH(k_chk_flags_g2, nb, KC_BLOCK, 0, comp, (const VkDev*)stage.dvk.p, (const G2Affine*)dv, n, 1u, flags);
      } else {
        G16_LAUNCH(k_chk_flags_g1, nb, KC_BLOCK, 0, comp, (const G1Affine*)dv, n, flags);
      }
      if (it.kind == CCK_PAIR) {
        G16_LAUNCH(k_cc_rho, dim3(nb, 2), KC_BLOCK, 0, comp, (const G1Affine*)(dv + off_before), (const G1Affine*)dv,
                   (const uint64_t*)(dv + off_rho), (const uint8_t*)flags, n, dpart.p);
        G16_LAUNCH(k_chk_fold<G1XYZZ>, 1, KC_BLOCK, 0, comp, (const G1XYZZ*)dpart.p, nb, 2u, dst.p->sum[it.q]);
      }
      stage.collect(flags, n, it.q, CC_QUERY_ID[it.q], it.base, &dst.p->tally);
      stage.end();
    }
    G16_LAUNCH(k_cc_final, 1, KC_BLOCK, 0, comp, (const VkDev*)stage.dvk.p, (const CcKey*)dkey.p, dst.p,
               (const g16_key_bad_point*)stage.dlists.p, stage.cap, mismatch, stage.dout.p);
    stage.finish(hs.get(), dst.p, report, bad_out);
    return G16_OK;
  });
}
