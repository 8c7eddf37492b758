// keycheck.hip -- validation of a proving key on the GPU before it is used (g16_key_check).
//
// The loaders copy the point sections of a .zkey as they come, exactly like the reference's
// deserialize_g1 / deserialize_g2 (src/zkey.rs:328-360: `new_unchecked`, no curve and no subgroup
// check).  A key with a flipped bit, a point of b_g2_query outside G2 or a b_g1_query that does not
// match b_g2_query still builds a ctx and proves at full speed -- every proof is garbage.  This file
// is the key-side counterpart of what verify.hip does for the three points of a proof:
//
//   structural   every point of every query, one lane per point: the stored words are canonical (< q),
//                the point is on its curve, a G2 point is in the r-torsion of the twist ([r] P = infinity,
//                a 254-bit double-and-add per point: the long kernel).  All-zero = infinity: valid, counted.
//   relations    e(beta_g1, g2) = e(g1, beta_g2), e(delta_g1, g2) = e(g1, delta_g2) and, with 128-bit
//                coefficients rho_i, e(sum rho_i B1_i, g2) = e(g1, sum rho_i B2_i): b_g1_query and b_g2_query
//                hold the same scalars (the small-exponent test g16_verify_aggregate uses for proofs).
//                Miller loop and final exponentiation are those of pairing.h.
//
// The queries are STREAMED through the CheckStage of keycheck.h: two page-locked host slots and two device slots
// of `chunk` points; the host fills slot k + 1 and its copy runs while the kernels of slot k do.  Device memory
// is fixed by the chunk, not by the key.  Per chunk:
//   k_chk_flags_g1 / _g2  one reason byte per point
//   k_kc_rho              (B chunks) rho_i B1_i and rho_i B2_i per lane, per-block sums through LDS trees
//   k_kc_fold             one block: the chunk's block sums into the running sums of the call
//   k_chk_collect         one block: counts the flags and appends the bad points, in index order, to the
//                         query's list
// and once at the end
//   k_kc_final            six Miller loops in six lanes, three final exponentiations in three, then the report
//                         and the bad-point list, concatenated in (query, index) order, assembled on the device.
// One synchronisation precedes the download of the report and the list.
#include "keycheck.h"

namespace g16 {
namespace {

constexpr uint32_t KC_DEFAULT_CHUNK = 1u << 18;
constexpr uint32_t KC_SLOT_BYTES_PER_POINT = 128 + 64 + 16;  // a B chunk: B2 | B1 | rho

struct KcKey {  // the six pairs of the three relations
  G1Affine beta_g1, delta_g1, g1_neg;
  G2Affine beta_g2, delta_g2, g2;
};

struct KcState {  // device-resident for the whole call
  CheckTally tally;
  G1XYZZ sum_b1;  // sum rho_i B1_i so far
  G2XYZZ sum_b2;  // sum rho_i B2_i so far
  g16_key_report report;
};

// blockIdx.y = 0: part1[block] = sum over the block of rho_i B1_i; 1: part2[block] = the same over B2.
// A malformed point is left out: the relations are not reported then anyway.
__global__ void __launch_bounds__(KC_BLOCK) k_kc_rho(const G1Affine* b1, const G2Affine* b2, const uint64_t* rho,
                                                     const uint8_t* f1, const uint8_t* f2, uint32_t n,
                                                     G1XYZZ* part1, G2XYZZ* part2) {
  __shared__ G1XYZZ sh1[KC_BLOCK];
  __shared__ G2XYZZ sh2[KC_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * KC_BLOCK + t;
  const bool live = i < n;
  const uint64_t lo = live ? rho[2 * (size_t)i] : 0, hi = live ? rho[2 * (size_t)i + 1] : 0;
  if (blockIdx.y == 0) {
    G1XYZZ acc = G1XYZZ::infinity();
    if (live && !(f1[i] & ~KC_INF)) acc = mul_rho(b1[i], lo, hi);
    kc_block_sum(sh1, acc);
    if (t == 0) part1[blockIdx.x] = sh1[0];
  } else {
    G2XYZZ acc = G2XYZZ::infinity();
    if (live && !(f2[i] & ~KC_INF)) acc = mul_rho(b2[i], lo, hi);
    kc_block_sum(sh2, acc);
    if (t == 0) part2[blockIdx.x] = sh2[0];
  }
}

// one block: the chunk's nb block sums, then into the running sums
__global__ void __launch_bounds__(KC_BLOCK) k_kc_fold(const G1XYZZ* part1, const G2XYZZ* part2, uint32_t nb, KcState* st) {
  __shared__ G1XYZZ sh1[KC_BLOCK];
  __shared__ G2XYZZ sh2[KC_BLOCK];
  chk_fold(part1, nb, &st->sum_b1, sh1);
  chk_fold(part2, nb, &st->sum_b2, sh2);
}

// lanes 0..5: the Miller loops  ML(g2, beta_g1) ML(beta_g2, -g1) | ML(g2, delta_g1) ML(delta_g2, -g1) |
// ML(g2, sum rho B1) ML(sum rho B2, -g1); lanes 0..2: product and final exponentiation of one pair each;
// then the report and the list.  Nothing is paired when a structural check failed.
__global__ void __launch_bounds__(KC_BLOCK) k_kc_final(const VkDev* vk, const KcKey* key, KcState* st,
                                                       const g16_key_bad_point* lists, uint32_t cap,
                                                       uint32_t vk_mismatch, g16_key_bad_point* out_list) {
  __shared__ F12 sh[6];
  __shared__ uint32_t sh_fail[3];
  __shared__ uint32_t sh_off[G16_KEY_N_QUERIES + 2];
  const uint32_t t = threadIdx.x;
  const bool pair = !chk_offsets(&st->tally, G16_KEY_N_QUERIES, cap, sh_off);
  G2Affine Q = G2Affine::infinity();
  G1Affine P = G1Affine::infinity();
  if (pair && t < 6) {
    if (t & 1) {
      P = key->g1_neg;
      Q = t == 1 ? key->beta_g2 : t == 3 ? key->delta_g2 : st->sum_b2.to_affine();
    } else {
      Q = key->g2;
      P = t == 0 ? key->beta_g1 : t == 2 ? key->delta_g1 : st->sum_b1.to_affine();
    }
  }
  const uint32_t failed = chk_pairs(Q, P, 3, pair, vk, sh, sh_fail);  // bits G16_KEY_PAIR_BETA, _DELTA, _B
  if (t == 0) {
    g16_key_report r;
    memset(&r, 0, sizeof r);
    r.relations_checked = pair ? 1 : 0;
    r.relations_failed = pair ? (failed | (vk_mismatch ? G16_KEY_VK_MISMATCH : 0)) : 0;
    r.ok = (pair && !r.relations_failed) ? 1 : 0;
    chk_counts(&r, &st->tally, G16_KEY_N_QUERIES);
    r.n_listed = sh_off[G16_KEY_N_QUERIES];
    st->report = r;
  }
  chk_emit_lists(sh_off, G16_KEY_N_QUERIES, lists, cap, out_list);
}

// ---- host side -------------------------------------------------------------------------------------

enum { KC_G1 = 0, KC_G2 = 1, KC_B = 2 };
struct Item {
  int kind;
  uint32_t query, base, count;
  const uint8_t* src;   // G1 / G2 points; B: b_g1_query
  const uint8_t* src2;  // B: b_g2_query
};

void add_items(std::vector<Item>& items, int kind, uint32_t query, const uint8_t* src, const uint8_t* src2,
               uint64_t count, uint32_t chunk, uint32_t base0 = 0) {
  const size_t w = kind == KC_G2 ? 128 : 64;
  for (uint64_t at = 0; at < count; at += chunk) {
    const uint32_t c = (uint32_t)(count - at < chunk ? count - at : chunk);
    items.push_back(Item{kind, query, base0 + (uint32_t)at, c, src + at * w, src2 ? src2 + at * 128 : nullptr});
  }
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" g16_status g16_key_check(int device, const g16_key_desc* key, const g16_vk_desc* vk, const uint64_t* rho,
                                    g16_key_bad_point* bad_out, uint32_t bad_cap, g16_key_report* report) {
  if (!key || !report || (bad_cap && !bad_out)) return G16_ERR_INVALID;
  const uint64_t N = key->n_vars, p = key->n_public, dom = key->domain_size;
  if (N < 1 || p + 1 > N) return G16_ERR_INVALID;
  const uint64_t n_l = N - p - 1;
  if (!key->a_query || !key->b_g1_query || !key->b_g2_query || (n_l && !key->l_query) || (dom && !key->h_query))
    return G16_ERR_INVALID;
  if (vk && (!vk->ic || vk->ic_count < 1)) return G16_ERR_INVALID;
  if (!rho_all_nonzero(rho, N)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&]() -> g16_status {
    uint64_t longest = N > dom ? N : dom;
    if (vk && vk->ic_count > longest) longest = vk->ic_count;
    if (longest < 3) longest = 3;  // the single points
    const uint32_t chunk = chunk_from_env("G16_KEYCHECK_CHUNK", KC_DEFAULT_CHUNK, longest);
    const uint32_t nb_max = ceil_div(chunk, KC_BLOCK);

    // what the key and the verifying key must agree on: compared as bytes
    uint32_t vk_mismatch = 0;
    if (vk) {
      if (memcmp(vk->alpha_g1, key->alpha_g1, 64) || memcmp(vk->beta_g2, key->beta_g2, 128) ||
          memcmp(vk->delta_g2, key->delta_g2, 128) || (uint64_t)vk->ic_count != p + 1)
        vk_mismatch = 1;
    }
    uint8_t singles_g1[3 * 64], singles_g2[3 * 128];
    memcpy(singles_g1, key->alpha_g1, 64);
    memcpy(singles_g1 + 64, key->beta_g1, 64);
    memcpy(singles_g1 + 128, key->delta_g1, 64);
    memcpy(singles_g2, key->beta_g2, 128);
    memcpy(singles_g2 + 128, key->delta_g2, 128);
    if (vk) memcpy(singles_g2 + 256, vk->gamma_g2, 128);

    std::vector<Item> items;
    add_items(items, KC_G1, G16_KEY_Q_A, key->a_query, nullptr, N, chunk);
    add_items(items, KC_B, G16_KEY_Q_B1, key->b_g1_query, key->b_g2_query, N, chunk);
    add_items(items, KC_G1, G16_KEY_Q_L, key->l_query, nullptr, n_l, chunk);
    add_items(items, KC_G1, G16_KEY_Q_H, key->h_query, nullptr, dom, chunk);
    if (vk) add_items(items, KC_G1, G16_KEY_Q_IC, vk->ic, nullptr, vk->ic_count, chunk);
    add_items(items, KC_G1, G16_KEY_Q_SINGLES, singles_g1, nullptr, 3, chunk, 0);
    add_items(items, KC_G2, G16_KEY_Q_SINGLES, singles_g2, nullptr, vk ? 3 : 2, chunk, 3);

    G16_HIP(hipSetDevice(device));
    KcKey hk;
    memcpy(&hk.beta_g1, key->beta_g1, 64);
    memcpy(&hk.delta_g1, key->delta_g1, 64);
    memcpy(&hk.beta_g2, key->beta_g2, 128);
    memcpy(&hk.delta_g2, key->delta_g2, 128);
    hk.g1_neg = G1Affine{Fq::one(), Fq::from_u32(2)}.neg();
    memcpy(&hk.g2, G2_GEN_WORDS, 128);
    std::unique_ptr<KcState> hs(new KcState());
    memset(hs.get(), 0, sizeof(KcState));
    uint64_t* n_points = hs->tally.n_points;
    n_points[G16_KEY_Q_A] = n_points[G16_KEY_Q_B1] = n_points[G16_KEY_Q_B2] = N;
    n_points[G16_KEY_Q_L] = n_l;
    n_points[G16_KEY_Q_H] = dom;
    n_points[G16_KEY_Q_IC] = vk ? vk->ic_count : 0;
    n_points[G16_KEY_Q_SINGLES] = vk ? 6 : 5;

    CheckStage stage((size_t)chunk * KC_SLOT_BYTES_PER_POINT, 2 * (size_t)chunk, G16_KEY_N_QUERIES, bad_cap);
    DevBuf<KcKey> dkey;
    DevBuf<KcState> dst;
    DevBuf<G1XYZZ> dpart1;
    DevBuf<G2XYZZ> dpart2;
    dkey.alloc(1);
    dst.alloc(1);
    dpart1.alloc(nb_max);
    dpart2.alloc(nb_max);
    G16_HIP(hipMemcpy(dkey.p, &hk, sizeof hk, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(dst.p, hs.get(), sizeof(KcState), hipMemcpyHostToDevice));
    const hipStream_t copy = stage.copy.s, comp = stage.comp.s;
    const VkDev* dvk = stage.dvk.p;
    CheckTally* tally = &dst.p->tally;

    const size_t off_b1 = (size_t)chunk * 128, off_rho = (size_t)chunk * 192;
    for (const Item& it : items) {
      const auto [h, d] = stage.begin();
      const uint32_t n = it.count;
      if (it.kind == KC_B) {
        memcpy(h, it.src2, (size_t)n * 128);
        memcpy(h + off_b1, it.src, (size_t)n * 64);
        uint64_t* hr = (uint64_t*)(h + off_rho);
        if (rho) {
          memcpy(hr, rho + 2 * (size_t)it.base, (size_t)n * 16);
        } else if (!draw_rho(hr, n)) {  // drawn chunk by chunk, straight into the staging slot
          stage.drain();
          return G16_ERR_INTERNAL;
        }
        G16_HIP(hipMemcpyAsync(d, h, (size_t)n * 128, hipMemcpyHostToDevice, copy));
        G16_HIP(hipMemcpyAsync(d + off_b1, h + off_b1, (size_t)n * 64, hipMemcpyHostToDevice, copy));
        G16_HIP(hipMemcpyAsync(d + off_rho, h + off_rho, (size_t)n * 16, hipMemcpyHostToDevice, copy));
      } else {
        const size_t bytes = (size_t)n * (it.kind == KC_G2 ? 128 : 64);
        memcpy(h, it.src, bytes);
        G16_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, copy));
      }
      stage.staged();
      const uint32_t nb = ceil_div(n, KC_BLOCK);
      uint8_t* f1 = stage.dflags.p;
      uint8_t* f2 = f1 + chunk;
      if (it.kind == KC_B) {
        G16_LAUNCH(k_chk_flags_g1, nb, KC_BLOCK, 0, comp, (const G1Affine*)(d + off_b1), n, f1);
        G16_LAUNCH(k_chk_flags_g2, nb, KC_BLOCK, 0, comp, dvk, (const G2Affine*)d, n, 1u, f2);
        G16_LAUNCH(k_kc_rho, dim3(nb, 2), KC_BLOCK, 0, comp, (const G1Affine*)(d + off_b1), (const G2Affine*)d,
                   (const uint64_t*)(d + off_rho), (const uint8_t*)f1, (const uint8_t*)f2, n, dpart1.p, dpart2.p);
        G16_LAUNCH(k_kc_fold, 1, KC_BLOCK, 0, comp, (const G1XYZZ*)dpart1.p, (const G2XYZZ*)dpart2.p, nb, dst.p);
        stage.collect(f1, n, G16_KEY_Q_B1, G16_KEY_Q_B1, it.base, tally);
        stage.collect(f2, n, G16_KEY_Q_B2, G16_KEY_Q_B2, it.base, tally);
      } else {
        if (it.kind == KC_G2)
          G16_LAUNCH(k_chk_flags_g2, nb, KC_BLOCK, 0, comp, dvk, (const G2Affine*)d, n, 1u, f1);
        else
          G16_LAUNCH(k_chk_flags_g1, nb, KC_BLOCK, 0, comp, (const G1Affine*)d, n, f1);
        stage.collect(f1, n, it.query, it.query, it.base, tally);
      }
      stage.end();
    }
    G16_LAUNCH(k_kc_final, 1, KC_BLOCK, 0, comp, dvk, (const KcKey*)dkey.p, dst.p,
               (const g16_key_bad_point*)stage.dlists.p, stage.cap, vk_mismatch, stage.dout.p);
    stage.finish(hs.get(), dst.p, report, bad_out);
    return G16_OK;
  });
}
