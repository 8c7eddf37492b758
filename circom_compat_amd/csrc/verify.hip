// verify.hip -- Groth16 verification on the GPU, per proof and aggregate, for proofs under one key or under many
// (first half).
//
// Replaces, for a batch of proofs under one verifying key,
//   let pvk = Groth16::<Bn254>::process_vk(&params.vk)?;
//   Groth16::<Bn254>::verify_with_processed_vk(&pvk, &inputs, &proof)?
// (reference call sites src/zkey.rs:868-870,914-916; tests/groth16.rs:33-35): per proof
//   e(A, B) * e(-alpha, beta) * e(-(IC_0 + sum_i pub_i IC_{i+1}), gamma) * e(-C, delta) == 1.
// ark-groth16 / ark-ec are un-vendored, so this restates the published optimal-ate pairing for
// BN254 in the formulation of SURVEY.md Appendix C.3 (the one the test-suite's checker uses, which
// pins it): Fq12 = Fq[w] / (w^12 - 18 w^6 + 82) in the polynomial basis, G2 arithmetic in
// affine Fq2 on the twist, Miller loop over 6x + 2 followed by the two Frobenius steps.  The final
// exponentiation is NOT the checker's plain power but the usual easy part
// (q^6 - 1)(q^2 + 1) followed by the Fuentes-Castaneda hard part (three exponentiations by the BN
// parameter x): it raises to a fixed multiple of (q^12 - 1) / r that is coprime to r, so
// "result == 1" is the same predicate (checked against the plain power in the tests).
//
// Off the proving path and deliberately simple: ONE LANE PER PROOF, saturated-limb field.h
// arithmetic, ~1.4 x 10^5 Fq multiplications per proof -- a throughput kernel for large batches,
// not a latency win over one CPU core for a single proof.
//
// Aggregate verification: the proofs of a GROUP (one key with the proofs under it) in ONE combined
// pairing check.  With coefficients rho_i (128-bit, unknown to whoever made the proofs) the group's
// per-proof equations fold into
//   prod_i ML(B_i, rho_i A_i) * ML(beta, -(sum rho_i) alpha) * ML(gamma, -sum rho_i X_i)
//       * ML(delta, -sum rho_i C_i)   --final exponentiation-->   1,
//   sum_i rho_i X_i = (sum_i rho_i) IC_0 + sum_j (sum_i rho_i pub_ij) IC_{j+1}
// (the small-exponent batch test).  Per proof that is one Miller loop, two 128-bit G1
// multiplications and the structural checks; the key-side Miller loops and the final
// exponentiation are paid once per group.  The long serial pieces sit in separate lanes:
//   k_agg_front   grid (front blocks, 3).  blockIdx.y = 0: structural checks (incl. the 254-bit subgroup
//                 multiplication); 1: P_i = rho_i A_i (affine); 2: rho_i C_i and rho_i pub_ij, summed
//                 per block through LDS, the loop over j bounded by the block's own n_pub
//   k_agg_sums    per group n_pub + 2 blocks over that group's block partials: -sum rho_i C_i, the
//                 columns s_j = sum_i rho_i pub_ij, and one lane for -(sum rho_i) alpha
//   k_agg_x       one block per group over its own IC range: -((sum rho) IC_0 + sum_j s_j IC_{j+1}),
//                 one lane per term, LDS sum
//   k_agg_miller  count + 3 lanes per group, one Miller loop each; per-block product through LDS
//   k_agg_tail    one block per group: product of the group's block products, AND of its structural
//                 flags, final exponentiation in one lane -- all groups side by side
// Per-proof path: k_verify_prepare (ml_alpha_beta, one lane per key), k_verify_batch (one lane per proof,
// the lane's key from front[]).
// What a call costs is a serial chain -- front, one Miller loop, one final exponentiation -- that is
// one lane's work and almost flat in the batch size.  Nothing in the chain depends on the key except
// three G2 points and the IC row, so the groups of a call share every launch: the per-proof lanes of all
// groups run side by side, every reduction is per group, and the K final exponentiations are K lanes of
// one launch.  g16_verify_batch and g16_verify_aggregate are the calls with ONE group.
//
// Host tables (built once per call, uploaded in one copy each):
//   KeyTab[k]      the group's key material offsets (VkDev k, first IC point, n_pub, first public input as
//                  a 64-bit offset), its proofs [first, first + count), its blocks and sum_i rho_i
//   front[b]       (key, first proof, live lanes) of block b of the per-proof front: a group of count
//                  proofs owns ceil(count / AGG_BLOCK) blocks of its own, so NO BLOCK STRADDLES TWO
//                  GROUPS and the LDS tree sums of the front are per group by construction
//   miller[b]      (key, first lane within the group, live lanes) of block b of the Miller lanes: a
//                  non-empty group owns ceil((count + 3) / AGG_BLOCK) blocks -- count proof lanes, then
//                  its three key-side lanes.  Blocks do not mix groups (the block product is NOT
//                  segmented), so a block product belongs to one group's equation
// No atomics: every reduction is a fixed tree over a fixed range, so the bytes of every intermediate
// do not depend on scheduling.  The number of launches, allocations, copies and synchronisations of a
// call does not depend on the number of keys.
#include "../../include/g16_amd.h"

#include <vector>

#include "keycheck.h"
#include "pairing.h"

namespace g16 {
namespace {

constexpr uint32_t AGG_BLOCK = 64;  // lanes per block of every kernel here

struct AggKey {
  G1Affine p[3];  // G1 sides paired with beta, gamma, delta
};

struct KeyTab {
  uint64_t pub_off;    // first Fr of the group's public-input block
  uint64_t spart_off;  // first Fr of the group's per-block column partials (n_pub x nfb, column-major)
  uint32_t ic_off;     // first IC point of the key; also its first scalar in scal[]
  uint32_t n_pub;
  uint32_t first, count;  // the group's proofs
  uint32_t fb0, nfb;      // its blocks of the front
  uint32_t mb0, nmb;      // its blocks of the Miller lanes
  U256 rho_sum;           // sum of its coefficients (an integer < 2^160)
};

struct BlockTab {
  uint32_t key, first, live;
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

// lane k: ml_alpha_beta of key k
__global__ void __launch_bounds__(64) k_verify_prepare(VkDev* vks, const KeyTab* keys, uint32_t n_keys) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_keys || !keys[k].count) return;
  VkDev* vk = vks + k;
  F12 f = f12_one();
  miller_mul(&f, &vk->beta, &vk->alpha_neg, vk);
  vk->ml_alpha_beta = f;
}

// one lane per proof, under the key of its block of front[]
__global__ void __launch_bounds__(64) k_verify_batch(const VkDev* vks, const KeyTab* keys, const BlockTab* blocks,
                                                      const G1Affine* ics, const uint8_t* proofs, const Fr* pubs,
                                                      uint8_t* ok) {
  const BlockTab blk = blocks[blockIdx.x];
  if (threadIdx.x >= blk.live) return;
  const uint32_t i = blk.first + threadIdx.x;
  const KeyTab* kt = keys + blk.key;
  const VkDev* vk = vks + blk.key;
  const uint32_t n_pub = kt->n_pub;
  const G1Affine* ic = ics + kt->ic_off;
  const Fr* pub = pubs + kt->pub_off + (size_t)(i - kt->first) * n_pub;
  G1Affine A, C;
  G2Affine B;
  memcpy(&A, proofs + (size_t)i * G16_PROOF_BYTES, 64);
  memcpy(&B, proofs + (size_t)i * G16_PROOF_BYTES + 64, 128);
  memcpy(&C, proofs + (size_t)i * G16_PROOF_BYTES + 192, 64);
  // what deserialising a Proof enforces in the reference (ark-serialize, Validate::Yes) before any
  // pairing runs: canonical coordinates, points on their curves, B in the prime-order subgroup
  // (G1 has cofactor 1).  Anything else is rejected here, never paired.
  const bool canonical = fq_words_canonical(A.x) && fq_words_canonical(A.y) && fq_words_canonical(C.x) &&
                         fq_words_canonical(C.y) && fq_words_canonical(B.x.c0) && fq_words_canonical(B.x.c1) &&
                         fq_words_canonical(B.y.c0) && fq_words_canonical(B.y.c1);
  if (!(canonical && on_curve_g1(A) && on_curve_g1(C) && on_curve_g2(B, vk) && g2_in_subgroup(B))) {
    ok[i] = 0;
    return;
  }
  // prepared inputs: IC_0 + sum_j pub_j IC_{j+1}   (ark-groth16 prepare_inputs)
  XYZZ<Fq> acc = XYZZ<Fq>::from_affine(ic[0]);
#pragma unroll 1
  for (uint32_t j = 0; j < n_pub; ++j) {
    const U256 s = pub[j].to_canonical();
    XYZZ<Fq> t = XYZZ<Fq>::from_affine(ic[j + 1]).mul(s);
    acc.add(t);
  }
  G1Affine vkx = acc.to_affine().neg();
  G1Affine Cn = C.neg();
  F12 f = vk->ml_alpha_beta;
  miller_mul(&f, &B, &A, vk);
  miller_mul(&f, &vk->gamma, &vkx, vk);
  miller_mul(&f, &vk->delta, &Cn, vk);
  ok[i] = final_exp_is_one(&f, vk) ? 1 : 0;
}

// block b of front[], blockIdx.y = its role: structural[i] | P[i] | c_part[b], s_part[spart_off + j * nfb + (block - fb0)]
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_front(const VkDev* vks, const KeyTab* keys, const BlockTab* blocks,
                                                          const uint8_t* proofs, const Fr* pubs, const uint64_t* rho,
                                                          uint8_t* structural, G1Affine* P, G1XYZZ* c_part,
                                                          Fr* s_part) {
  __shared__ G1XYZZ sh_c[AGG_BLOCK];
  __shared__ Fr sh_s[AGG_BLOCK];
  const BlockTab blk = blocks[blockIdx.x];
  const uint32_t t = threadIdx.x, i = blk.first + t;
  const bool live = t < blk.live;
  const uint8_t* proof = proofs + (size_t)(live ? i : blk.first) * G16_PROOF_BYTES;
  if (blockIdx.y == 0) {  // what k_verify_batch checks before it pairs
    if (!live) return;
    G1Affine A, C;
    G2Affine B;
    memcpy(&A, proof, 64);
    memcpy(&B, proof + 64, 128);
    memcpy(&C, proof + 192, 64);
    const bool canonical = fq_words_canonical(B.x.c0) && fq_words_canonical(B.x.c1) &&
                           fq_words_canonical(B.y.c0) && fq_words_canonical(B.y.c1);
    structural[i] = (canonical && g1_well_formed(A) && g1_well_formed(C) && on_curve_g2(B, vks + blk.key) &&
                     g2_in_subgroup(B)) ? 1 : 0;
    return;
  }
  if (blockIdx.y == 1) {  // a malformed A is never paired (k_agg_miller skips the proof): any value will do
    if (!live) return;
    G1Affine A;
    memcpy(&A, proof, 64);
    P[i] = g1_well_formed(A) ? G1XYZZ::from_affine(A).mul(rho_u256(rho, i)).to_affine() : G1Affine::infinity();
    return;
  }
  // a malformed proof makes the verdict 0 whatever the sums are: a malformed C is left out of them
  G1XYZZ acc = G1XYZZ::infinity();
  Fr rf = Fr::zero();
  if (live) {
    G1Affine C;
    memcpy(&C, proof + 192, 64);
    const U256 k = rho_u256(rho, i);
    if (g1_well_formed(C)) acc = G1XYZZ::from_affine(C).mul(k);
    rf = Fr::from_canonical(k);
  }
  block_sum_g1(sh_c, acc);
  if (t == 0) c_part[blockIdx.x] = sh_c[0];
  const KeyTab* kt = keys + blk.key;
  const uint32_t n_pub = kt->n_pub, nfb = kt->nfb;
  const Fr* pub = pubs + kt->pub_off + (size_t)(i - kt->first) * n_pub;  // read by live lanes only
  Fr* part = s_part + kt->spart_off + (blockIdx.x - kt->fb0);
#pragma unroll 1
  for (uint32_t j = 0; j < n_pub; ++j) {
    Fr v = live ? rf * pub[j] : Fr::zero();
    sh_s[t] = v;
#pragma unroll 1
    for (uint32_t s = AGG_BLOCK / 2; s > 0; s >>= 1) {
      __syncthreads();
      if (t < s) {
        v = v + sh_s[t + s];
        sh_s[t] = v;
      }
    }
    if (t == 0) part[(size_t)j * nfb] = v;
    __syncthreads();
  }
}

// block k * stride + b of group k: b = 0: -sum rho_i C_i; b = 1 + j: s_j (canonical, the scalar of IC_{j+1});
// b = n_pub + 1: -(sum rho) alpha; above (a key with fewer inputs than the widest) and empty groups: nothing
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_sums(const VkDev* vks, const KeyTab* keys, uint32_t stride,
                                                         const G1XYZZ* c_part, const Fr* s_part, AggKey* key,
                                                         U256* scal) {
  __shared__ G1XYZZ sh_c[AGG_BLOCK];
  __shared__ Fr sh_s[AGG_BLOCK];
  const uint32_t t = threadIdx.x, g = blockIdx.x / stride, b = blockIdx.x % stride;
  const KeyTab* kt = keys + g;
  const uint32_t n_pub = kt->n_pub, nb = kt->nfb;
  if (!kt->count || b > n_pub + 1) return;
  if (b == 0) {
    const G1XYZZ* cp = c_part + kt->fb0;
    G1XYZZ acc = G1XYZZ::infinity();
#pragma unroll 1
    for (uint32_t k = t; k < nb; k += AGG_BLOCK) acc.add(cp[k]);
    block_sum_g1(sh_c, acc);
    if (t == 0) key[g].p[2] = sh_c[0].to_affine().neg();
  } else if (b <= n_pub) {
    const Fr* sp = s_part + kt->spart_off + (size_t)(b - 1) * nb;
    Fr v = Fr::zero();
#pragma unroll 1
    for (uint32_t k = t; k < nb; k += AGG_BLOCK) v = v + sp[k];
    sh_s[t] = v;
#pragma unroll 1
    for (uint32_t s = AGG_BLOCK / 2; s > 0; s >>= 1) {
      __syncthreads();
      if (t < s) {
        v = v + sh_s[t + s];
        sh_s[t] = v;
      }
    }
    if (t == 0) scal[kt->ic_off + b] = v.to_canonical();
  } else if (t == 0) {
    key[g].p[0] = G1XYZZ::from_affine(vks[g].alpha_neg).mul(kt->rho_sum).to_affine();
    scal[kt->ic_off] = kt->rho_sum;  // the scalar of IC_0
  }
}

// block g: -(sum_j scal_j IC_j) over the key's own IC range, j = 0 .. n_pub
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_x(const KeyTab* keys, const G1Affine* ics, const U256* scal,
                                                      AggKey* key) {
  __shared__ G1XYZZ sh_c[AGG_BLOCK];
  const uint32_t t = threadIdx.x;
  const KeyTab* kt = keys + blockIdx.x;
  if (!kt->count) return;
  const G1Affine* ic = ics + kt->ic_off;
  const U256* sc = scal + kt->ic_off;
  const uint32_t n_pub = kt->n_pub;
  G1XYZZ acc = G1XYZZ::infinity();
#pragma unroll 1
  for (uint32_t j = t; j <= n_pub; j += AGG_BLOCK) acc.add(G1XYZZ::from_affine(ic[j]).mul(sc[j]));
  block_sum_g1(sh_c, acc);
  if (t == 0) key[blockIdx.x].p[1] = sh_c[0].to_affine().neg();
}

// lane l = blk.first + t of the block's group: l < count: ML(B_i, P_i) of proof first + l, or 1 for a malformed
// proof; l = count, count + 1, count + 2: the group's key side.  f_part[block] = product of the block's lanes
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_miller(const VkDev* vks, const KeyTab* keys,
                                                           const BlockTab* blocks, const uint8_t* proofs,
                                                           const G1Affine* P, const uint8_t* structural,
                                                           const AggKey* key, F12* f_part) {
  __shared__ F12 sh[AGG_BLOCK];
  const BlockTab blk = blocks[blockIdx.x];
  const uint32_t t = threadIdx.x;
  const VkDev* vk = vks + blk.key;
  const uint32_t count = keys[blk.key].count;
  G2Affine Q = G2Affine::infinity();
  G1Affine p = G1Affine::infinity();
  if (t < blk.live) {
    const uint32_t l = blk.first + t;
    if (l < count) {
      const uint32_t i = keys[blk.key].first + l;
      if (structural[i]) {
        memcpy(&Q, proofs + (size_t)i * G16_PROOF_BYTES + 64, 128);
        p = P[i];
      }
    } else {
      const uint32_t k = l - count;
      Q = k == 0 ? vk->beta : k == 1 ? vk->gamma : vk->delta;
      p = key[blk.key].p[k];
    }
  }
  F12 f = f12_one();
  miller_mul(&f, &Q, &p, vk);  // one call site for proof and key lanes: no divergent copies of the loop
  sh[t] = f;
#pragma unroll 1
  for (uint32_t s = AGG_BLOCK / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      f12_mul(&f, &f, &sh[t + s]);
      sh[t] = f;
    }
  }
  if (t == 0) f_part[blockIdx.x] = f;
}

// block g: the verdict of group g (an empty group: 1)
__global__ void __launch_bounds__(AGG_BLOCK) k_agg_tail(const VkDev* vks, const KeyTab* keys, const F12* f_part,
                                                         const uint8_t* structural, uint8_t* ok) {
  __shared__ F12 sh[AGG_BLOCK];
  __shared__ uint32_t sh_ok[AGG_BLOCK];
  const uint32_t t = threadIdx.x;
  const KeyTab* kt = keys + blockIdx.x;
  const uint32_t nb = kt->nmb, n = kt->count;
  if (!n) {
    if (t == 0) ok[blockIdx.x] = 1;
    return;
  }
  const F12* fp = f_part + kt->mb0;
  const uint8_t* st = structural + kt->first;
  F12 f = f12_one();
#pragma unroll 1
  for (uint32_t k = t; k < nb; k += AGG_BLOCK) f12_mul(&f, &f, &fp[k]);
  uint32_t sound = 1;
#pragma unroll 1
  for (uint32_t k = t; k < n; k += AGG_BLOCK) sound &= st[k];
  sh[t] = f;
  sh_ok[t] = sound;
#pragma unroll 1
  for (uint32_t s = AGG_BLOCK / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      f12_mul(&f, &f, &sh[t + s]);
      sh[t] = f;
      sound &= sh_ok[t + s];
      sh_ok[t] = sound;
    }
  }
  if (t == 0) ok[blockIdx.x] = (sound && final_exp_is_one(&f, vks + blockIdx.x)) ? 1 : 0;
}

// ---- host side ---------------------------------------------------------------------------------
// what both entry points refuse; *n_total = sum of counts
g16_status check_groups(const g16_vk_desc* const* vks, const uint32_t* counts, uint32_t n_keys,
                        const uint8_t* proofs, const uint64_t* public_inputs, uint64_t* n_total) {
  *n_total = 0;
  if (!n_keys) return G16_OK;
  if (!vks || !counts) return G16_ERR_INVALID;
  uint64_t n = 0, n_ic = 0;
  bool need_pub = false;
  for (uint32_t k = 0; k < n_keys; ++k) {
    if (!vks[k] || !vks[k]->ic || vks[k]->ic_count < 1) return G16_ERR_INVALID;
    n += counts[k];
    n_ic += vks[k]->ic_count;
    if (counts[k] && vks[k]->ic_count > 1) need_pub = true;
  }
  // proof lanes + 3 key-side lanes per group are indexed in 32 bits, and so are the concatenated IC rows
  if (n + 3 * (uint64_t)n_keys > 0xffffffffull || n_ic > 0xffffffffull) return G16_ERR_INVALID;
  if (n && !proofs) return G16_ERR_INVALID;
  if (need_pub && !public_inputs) return G16_ERR_INVALID;
  *n_total = n;
  return G16_OK;
}

struct Plan {
  std::vector<KeyTab> keys;
  std::vector<BlockTab> front, miller;
  std::vector<VkDev> vks;
  std::vector<uint8_t> ic;  // the keys' IC rows, one after the other
  uint64_t n_pub_words = 0;  // Fr in public_inputs
  uint64_t n_spart = 0;      // Fr in s_part
  uint32_t max_pub = 0;
};

// rho: the coefficients of all proofs, or NULL on the per-proof path (rho_sum stays 0, no Miller blocks)
void make_plan(Plan& pl, const g16_vk_desc* const* vks, const uint32_t* counts, uint32_t n_keys,
               const uint64_t* rho) {
  pl.keys.resize(n_keys);
  pl.vks.resize(n_keys);
  uint64_t first = 0, ic_off = 0;
  for (uint32_t k = 0; k < n_keys; ++k) {
    const g16_vk_desc* vk = vks[k];
    VkDev& hv = pl.vks[k];
    G1Affine alpha;
    memcpy(&alpha, vk->alpha_g1, 64);
    hv.alpha_neg = alpha.neg();
    memcpy(&hv.beta, vk->beta_g2, 128);
    memcpy(&hv.gamma, vk->gamma_g2, 128);
    memcpy(&hv.delta, vk->delta_g2, 128);
    vk_consts(&hv);
    hv.ml_alpha_beta = f12_one();  // the per-proof path fills it in k_verify_prepare; the aggregate path does not use it
    pl.ic.insert(pl.ic.end(), vk->ic, vk->ic + (size_t)vk->ic_count * 64);

    KeyTab& kt = pl.keys[k];
    const uint32_t n = counts[k];
    kt.pub_off = pl.n_pub_words;
    kt.spart_off = pl.n_spart;
    kt.ic_off = (uint32_t)ic_off;
    kt.n_pub = vk->ic_count - 1;
    kt.first = (uint32_t)first;
    kt.count = n;
    kt.fb0 = (uint32_t)pl.front.size();
    kt.nfb = ceil_div(n, AGG_BLOCK);
    kt.mb0 = (uint32_t)pl.miller.size();
    kt.nmb = (n && rho) ? ceil_div((uint64_t)n + 3, AGG_BLOCK) : 0;
    for (uint32_t b = 0; b < kt.nfb; ++b) {
      const uint32_t at = b * AGG_BLOCK;
      pl.front.push_back(BlockTab{k, kt.first + at, n - at < AGG_BLOCK ? n - at : AGG_BLOCK});
    }
    for (uint32_t b = 0; b < kt.nmb; ++b) {
      const uint64_t at = (uint64_t)b * AGG_BLOCK, left = (uint64_t)n + 3 - at;
      pl.miller.push_back(BlockTab{k, (uint32_t)at, left < AGG_BLOCK ? (uint32_t)left : AGG_BLOCK});
    }
    // sum of the group's coefficients as an integer: < 2^160, far below r, so it is its own residue
    uint64_t w0 = 0, w1 = 0, hi = 0;
    if (rho)
      for (uint64_t i = first; i < first + n; ++i) {
        unsigned __int128 lo = (unsigned __int128)w0 + rho[2 * i];
        w0 = (uint64_t)lo;
        lo = (lo >> 64) + w1 + rho[2 * i + 1];
        w1 = (uint64_t)lo;
        hi += (uint64_t)(lo >> 64);
      }
    const uint64_t w[4] = {w0, w1, hi, 0};
    for (int q = 0; q < 4; ++q) {
      kt.rho_sum.v[2 * q] = (uint32_t)w[q];
      kt.rho_sum.v[2 * q + 1] = (uint32_t)(w[q] >> 32);
    }
    pl.n_pub_words += (uint64_t)n * kt.n_pub;
    pl.n_spart += (uint64_t)kt.nfb * kt.n_pub;
    if (kt.n_pub > pl.max_pub) pl.max_pub = kt.n_pub;
    first += n;
    ic_off += vk->ic_count;
  }
}

// the device copies both paths need
struct PlanDev {
  DevBuf<VkDev> vks;
  DevBuf<KeyTab> keys;
  DevBuf<BlockTab> front;
  DevBuf<G1Affine> ic;
  DevBuf<uint8_t> proofs;
  DevBuf<Fr> pub;
  void upload(const Plan& pl, const uint8_t* proofs_h, const uint64_t* pubs_h, uint64_t n) {
    vks.alloc(pl.vks.size());
    keys.alloc(pl.keys.size());
    front.alloc(pl.front.size());
    ic.alloc(pl.ic.size() / 64);
    proofs.alloc((size_t)n * G16_PROOF_BYTES);
    pub.alloc(pl.n_pub_words ? pl.n_pub_words : 1);
    G16_HIP(hipMemcpy(vks.p, pl.vks.data(), pl.vks.size() * sizeof(VkDev), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(keys.p, pl.keys.data(), pl.keys.size() * sizeof(KeyTab), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(front.p, pl.front.data(), pl.front.size() * sizeof(BlockTab), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(ic.p, pl.ic.data(), pl.ic.size(), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(proofs.p, proofs_h, (size_t)n * G16_PROOF_BYTES, hipMemcpyHostToDevice));
    if (pl.n_pub_words) G16_HIP(hipMemcpy(pub.p, pubs_h, pl.n_pub_words * 32, hipMemcpyHostToDevice));
  }
};

// g16_verify_batch_keys; g16_verify_batch is the call with one group
g16_status verify_batch_groups(int device, const g16_vk_desc* const* vks, const uint32_t* counts, uint32_t n_keys,
                               const uint8_t* proofs, const uint64_t* public_inputs, uint8_t* ok_out) {
  uint64_t n = 0;
  if (check_groups(vks, counts, n_keys, proofs, public_inputs, &n) != G16_OK || (n && !ok_out))
    return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  if (!n) return G16_OK;
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    Plan pl;
    make_plan(pl, vks, counts, n_keys, nullptr);
    PlanDev d;
    DevBuf<uint8_t> dok;
    d.upload(pl, proofs, public_inputs, n);
    dok.alloc(n);
    G16_LAUNCH(k_verify_prepare, ceil_div(n_keys, 64), 64, 0, nullptr, d.vks.p, (const KeyTab*)d.keys.p, n_keys);
    G16_LAUNCH(k_verify_batch, (uint32_t)pl.front.size(), 64, 0, nullptr, (const VkDev*)d.vks.p,
               (const KeyTab*)d.keys.p, (const BlockTab*)d.front.p, (const G1Affine*)d.ic.p,
               (const uint8_t*)d.proofs.p, (const Fr*)d.pub.p, dok.p);
    G16_HIP(hipGetLastError());
    G16_HIP(hipDeviceSynchronize());
    G16_HIP(hipMemcpy(ok_out, dok.p, n, hipMemcpyDeviceToHost));
    return G16_OK;
  });
}

// g16_verify_aggregate_keys; g16_verify_aggregate is the call with one group
g16_status verify_aggregate_groups(int device, const g16_vk_desc* const* vks, const uint32_t* counts, uint32_t n_keys,
                                   const uint8_t* proofs, const uint64_t* public_inputs, const uint64_t* rho,
                                   uint8_t* ok_out, uint8_t* structural_out) {
  uint64_t n = 0;
  if (check_groups(vks, counts, n_keys, proofs, public_inputs, &n) != G16_OK || (n_keys && !ok_out))
    return G16_ERR_INVALID;
  if (!rho_all_nonzero(rho, n)) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  if (!n_keys) return G16_OK;
  if (!n) {
    memset(ok_out, 1, n_keys);
    return G16_OK;
  }
  return guarded_call([&]() -> g16_status {
    std::vector<uint64_t> drawn;
    if (!rho) {
      drawn.resize(2 * (size_t)n);
      if (!draw_rho(drawn.data(), (size_t)n)) return G16_ERR_INTERNAL;
      rho = drawn.data();
    }
    G16_HIP(hipSetDevice(device));
    Plan pl;
    make_plan(pl, vks, counts, n_keys, rho);
    const uint32_t nb = (uint32_t)pl.front.size(), nbm = (uint32_t)pl.miller.size();
    const uint64_t sum_blocks = (uint64_t)n_keys * ((uint64_t)pl.max_pub + 2);
    if (sum_blocks > 0x7fffffffull) return G16_ERR_INVALID;  // the grid of k_agg_sums
    PlanDev d;
    DevBuf<BlockTab> dmiller;
    DevBuf<G1Affine> dP;
    DevBuf<uint8_t> dstruct, dok;
    DevBuf<Fr> dspart;
    DevBuf<uint64_t> drho;
    DevBuf<G1XYZZ> dcpart;
    DevBuf<U256> dscal;
    DevBuf<AggKey> dkey;
    DevBuf<F12> dfpart;
    d.upload(pl, proofs, public_inputs, n);
    dmiller.alloc(nbm);
    dP.alloc(n);
    dstruct.alloc(n);
    dok.alloc(n_keys);
    dspart.alloc(pl.n_spart ? pl.n_spart : 1);
    drho.alloc(2 * (size_t)n);
    dcpart.alloc(nb);
    dscal.alloc(pl.ic.size() / 64);
    dkey.alloc(n_keys);
    dfpart.alloc(nbm);
    G16_HIP(hipMemcpy(dmiller.p, pl.miller.data(), (size_t)nbm * sizeof(BlockTab), hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(drho.p, rho, (size_t)n * 16, hipMemcpyHostToDevice));
    G16_LAUNCH(k_agg_front, dim3(nb, 3), AGG_BLOCK, 0, nullptr, (const VkDev*)d.vks.p, (const KeyTab*)d.keys.p,
               (const BlockTab*)d.front.p, (const uint8_t*)d.proofs.p, (const Fr*)d.pub.p, (const uint64_t*)drho.p,
               dstruct.p, dP.p, dcpart.p, dspart.p);
    G16_LAUNCH(k_agg_sums, (uint32_t)sum_blocks, AGG_BLOCK, 0, nullptr, (const VkDev*)d.vks.p,
               (const KeyTab*)d.keys.p, pl.max_pub + 2, (const G1XYZZ*)dcpart.p, (const Fr*)dspart.p, dkey.p,
               dscal.p);
    G16_LAUNCH(k_agg_x, n_keys, AGG_BLOCK, 0, nullptr, (const KeyTab*)d.keys.p, (const G1Affine*)d.ic.p,
               (const U256*)dscal.p, dkey.p);
    G16_LAUNCH(k_agg_miller, nbm, AGG_BLOCK, 0, nullptr, (const VkDev*)d.vks.p, (const KeyTab*)d.keys.p,
               (const BlockTab*)dmiller.p, (const uint8_t*)d.proofs.p, (const G1Affine*)dP.p,
               (const uint8_t*)dstruct.p, (const AggKey*)dkey.p, dfpart.p);
    G16_LAUNCH(k_agg_tail, n_keys, AGG_BLOCK, 0, nullptr, (const VkDev*)d.vks.p, (const KeyTab*)d.keys.p,
               (const F12*)dfpart.p, (const uint8_t*)dstruct.p, dok.p);
    G16_HIP(hipGetLastError());
    G16_HIP(hipDeviceSynchronize());
    G16_HIP(hipMemcpy(ok_out, dok.p, n_keys, hipMemcpyDeviceToHost));
    if (structural_out) G16_HIP(hipMemcpy(structural_out, dstruct.p, n, hipMemcpyDeviceToHost));
    return G16_OK;
  });
}

}  // namespace
}  // namespace g16

using namespace g16;

// A single-key call is the call with one group.  check_groups refuses for that group what these calls always
// refused, before the device is looked at: a NULL vk or ic, ic_count < 1, proofs or public inputs missing where
// n_proofs > 0 needs them.  ok_out: needed by the per-proof call when n_proofs > 0, by the aggregate call always
// (n_proofs == 0 writes 1 there).
extern "C" g16_status g16_verify_batch(int device, const g16_vk_desc* vk, const uint8_t* proofs,
                                       const uint64_t* public_inputs, uint32_t n_proofs, uint8_t* ok_out) {
  return verify_batch_groups(device, &vk, &n_proofs, 1, proofs, public_inputs, ok_out);
}

extern "C" g16_status g16_verify_aggregate(int device, const g16_vk_desc* vk, const uint8_t* proofs,
                                           const uint64_t* public_inputs, uint32_t n_proofs, const uint64_t* rho,
                                           uint8_t* ok_out, uint8_t* structural_out) {
  return verify_aggregate_groups(device, &vk, &n_proofs, 1, proofs, public_inputs, rho, ok_out, structural_out);
}

extern "C" g16_status g16_verify_batch_keys(int device, const g16_vk_desc* const* vks, const uint32_t* counts,
                                            uint32_t n_keys, const uint8_t* proofs, const uint64_t* public_inputs,
                                            uint8_t* ok_out) {
  return verify_batch_groups(device, vks, counts, n_keys, proofs, public_inputs, ok_out);
}

extern "C" g16_status g16_verify_aggregate_keys(int device, const g16_vk_desc* const* vks, const uint32_t* counts,
                                                uint32_t n_keys, const uint8_t* proofs,
                                                const uint64_t* public_inputs, const uint64_t* rho, uint8_t* ok_out,
                                                uint8_t* structural_out) {
  return verify_aggregate_groups(device, vks, counts, n_keys, proofs, public_inputs, rho, ok_out, structural_out);
}
