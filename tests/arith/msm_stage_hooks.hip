// msm_stage_hooks.hip -- TEST INFRASTRUCTURE ONLY: host wrappers that drive the stages of the Pippenger pipeline
// behind the sort one at a time (csrc/msm.h, csrc/msm_curve.inc.h):
//
//   g16_test_stage_reduce_g1 / _g2   msm_reduce_head (k_combine_large + k_bucket_reduce), a snapshot of `contrib`,
//                                    then msm_reduce_tail (two k_set_sum levels + k_horner), over SYNTHETIC partial
//                                    sums that the caller codes slot by slot
//   g16_test_stage_acc_g1 / _g2      msm_accumulate / msm_accumulate_pair with their fix-up, every partial slot out
//
// so that pytest can compare every contribution, set sum, output and partial slot with the exact model of
// tests/msm_stage_model.py.  Buffers a stage may write are pre-filled with the byte POISON; an element that still holds
// it was not written.
//
// Only the public interface of msm.h is used: msm_make_config, msm_red_chunk, msm_seg_len, MsmSort, MsmPoints,
// MsmWork (partial, contrib, bsum, wsum, fix), msm_accumulate, msm_accumulate_pair, msm_reduce_head, msm_reduce_tail.
// The two kernels of this file are conversions: k_fill_partials builds an MsmAcc<F> from a coded affine point,
// k_to_affine brings one back, with ec29.h's own from-/to-affine arithmetic.
//
// Built twice from this one file (csrc/Makefile): with g++ against the SIMT emulator into
// tests/emu/libg16_emu.so and with hipcc and the product flags into tests/arith/libg16_msmstage_gpu.so (linked with
// the product's own msm_sort.o, msm_g1.o, msm_g2.o).  Never linked into, loaded by or reachable from libg16_amd.so.
//
// Every wrapper returns 0, a HIP error code, or -1 with the message of the std::runtime_error in msg.
#include "common.h"
#include "msm.h"

using namespace g16;

namespace {

constexpr int POISON = 0x5a;                  // byte; a limb of 0x5a5a5a5a is outside every class of ec29.h
constexpr uint32_t POISON_WORD = 0x5a5a5a5au;
constexpr int CODE_INF = -1, CODE_POISON = -2;  // codes >= 0: pool index + npool * lambda index
constexpr int HOOK_SUM_THREADS = 128;         // SUM_THREADS of msm_curve.inc.h, restated for the reported nblk
constexpr int BLOCK = 64;

void put_msg(char* msg, size_t msg_len, const char* what) {
  if (!msg || !msg_len) return;
  strncpy(msg, what, msg_len - 1);
  msg[msg_len - 1] = 0;
}

template <class Body>
int guarded(char* msg, size_t msg_len, Body body) {
  put_msg(msg, msg_len, "");
  try {
    body();
    return 0;
  } catch (const HipError& e) {
    put_msg(msg, msg_len, e.what());
    return e.code ? e.code : -1;
  } catch (const std::runtime_error& e) {
    put_msg(msg, msg_len, e.what());
    return -1;
  }
}

void need(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(what);
}

template <class T>
void upload(DevBuf<T>& d, const void* host, size_t count) {
  d.alloc(count ? count : 1);
  if (count) G16_HIP(hipMemcpy(d.p, host, count * sizeof(T), hipMemcpyHostToDevice));
}

template <class T>
void poison(DevBuf<T>& d) {
  if (d.n) G16_HIP(hipMemset(d.p, POISON, d.bytes()));
}

void fetch(uint32_t* host, const uint32_t* dev, size_t words) {
  if (words) G16_HIP(hipMemcpy(host, dev, words * 4, hipMemcpyDeviceToHost));
}

// partial[i] = the point codes[i] names: (l^2 x, l^3 y, l^2, l^3) for pool point (x, y) and lambda l, i.e. the same
// point in truly projective coordinates; CODE_INF: the point at infinity; CODE_POISON: the pool's last point under
// the last lambda (a valid point the model never sums)
template <class F>
__global__ void __launch_bounds__(BLOCK) k_fill_partials(const int32_t* codes, const Affine<F>* pool, uint32_t npool,
                                                         const F* lam, uint32_t nlam, MsmAcc<F>* partial, size_t n) {
  using LF = typename Lazy<F>::type;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t code = codes[i];
  if (code == CODE_POISON) code = (int32_t)((npool - 1) + npool * (nlam - 1));
  if (code < 0 || (uint32_t)code >= npool * nlam) {  // CODE_INF (the host refuses every other value)
    partial[i] = MsmAcc<F>::infinity();
    return;
  }
  const Aff29<LF> p = affine_from_mont256<F>(pool[(uint32_t)code % npool]);
  if (p.inf) {
    partial[i] = MsmAcc<F>::infinity();
    return;
  }
  const LF l = LF::from_mont256(lam[(uint32_t)code / npool]);
  const LF l2 = l.sqr(), l3 = l2 * l;
  partial[i] = MsmAcc<F>{p.x * l2, p.y * l3, l2, l3};
}

// out[i] = in[i] as an affine point in the storage form (all-zero: infinity); flag[i] = 1 when every word of in[i]
// still holds the poison (out[i] zeroed), 2 when only some do (not converted either)
template <class F>
__global__ void __launch_bounds__(BLOCK) k_to_affine(const MsmAcc<F>* in, Affine<F>* out, uint8_t* flag, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + i);
  uint32_t hit = 0;
  constexpr uint32_t words = sizeof(MsmAcc<F>) / 4;
  for (uint32_t k = 0; k < words; ++k) hit += w[k] == POISON_WORD ? 1u : 0u;
  flag[i] = hit == words ? 1 : hit ? 2 : 0;
  out[i] = Affine<F>::infinity();
  if (hit) return;
  const auto a = in[i].template to_affine<true>();  // the binary-GCD inversion: an element per thread, no wave to keep in step
  if (!a.inf) out[i] = Affine<F>{a.x.to_mont256(), a.y.to_mont256()};
}

template <class F>
void to_affine_host(const MsmAcc<F>* dev, size_t n, void* out_host, uint8_t* flag_host) {
  if (!n) return;
  DevBuf<Affine<F>> out;
  DevBuf<uint8_t> flag;
  out.alloc(n);
  flag.alloc(n);
  G16_LAUNCH((k_to_affine<F>), ceil_div(n, BLOCK), BLOCK, 0, 0, dev, out.p, flag.p, n);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());
  G16_HIP(hipMemcpy(out_host, out.p, n * sizeof(Affine<F>), hipMemcpyDeviceToHost));
  G16_HIP(hipMemcpy(flag_host, flag.p, n, hipMemcpyDeviceToHost));
}

struct SortArgs {
  const uint32_t* scalars;
  uint32_t n1;
  int mont, c, planes;
  uint32_t nproof;
  uint64_t stride;
  int rank, world;
  uint32_t lanes, lanes2;
};

// the real MsmSort::run, as g16_test_sort_run drives it
void run_sort(const SortArgs& a, MsmSort& s, DevBuf<U256>& dscal) {
  need(a.nproof >= 1, "stage hook: no proof");
  MsmConfig cfg = msm_make_config(a.n1, a.c, a.planes);
  if (a.lanes) cfg.lanes = a.lanes;
  if (a.lanes2) cfg.lanes2 = a.lanes2;
  need(cfg.lanes % MSM_ACC_THREADS == 0 && cfg.lanes2 % MSM_ACC_THREADS == 0 && cfg.lanes && cfg.lanes2,
       "stage hook: lanes are multiples of 128");
  const size_t nscal = a.nproof > 1 ? (size_t)(a.nproof - 1) * a.stride + a.n1 : a.n1;
  upload(dscal, a.scalars, nscal);
  s.init(a.n1, cfg, a.nproof);
  if (a.world > 1) s.set_shard(a.rank, a.world);
  s.run(dscal.p, a.n1, a.mont != 0, 0, a.nproof, (size_t)a.stride);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());
}

// geo: 12 words: red_chunk, cps, nchunks, nblk, sets, S, lanes, slots, ncontrib, work sets, M, hot count

template <class F>
void reduce_hook(const SortArgs& a, uint32_t nbatch, int hidden, uint64_t out_stride, const void* pool, uint32_t npool,
                 const void* lam, uint32_t nlam, const int32_t* codes, uint64_t ncodes, uint32_t contrib_pad,
                 uint32_t* geo, uint32_t* offset, uint32_t* hot, uint32_t hot_cap, uint32_t* range, void* contrib_out,
                 uint8_t* contrib_flag, void* wsum_out, uint8_t* wsum_flag, void* sums_out, uint8_t* sums_flag,
                 uint64_t* gap_dirty) {
  constexpr bool g2 = sizeof(F) != sizeof(Fq);
  need(nbatch >= 1 && npool >= 1 && nlam >= 1 && (uint64_t)npool * nlam < (1u << 30), "stage hook: bad pool");
  MsmSort s;
  DevBuf<U256> dscal;
  run_sort(a, s, dscal);
  const MsmConfig& cfg = s.cfg;
  const uint32_t nbt = s.nbt(), lanes = s.lanes_of(g2);
  fetch(offset, s.offset.p, (size_t)nbt + 1);
  const uint32_t M = offset[nbt];
  const uint32_t S = msm_seg_len(M, lanes);
  // slot = bucket + lane, lane < lanes
  const uint64_t slots64 = (uint64_t)nbt + lanes;
  need(slots64 < (1ull << 31), "stage hook: too many slots");
  const uint32_t slots = (uint32_t)slots64;
  need(ncodes == (uint64_t)nbatch * slots, "stage hook: one code per partial slot of every workspace slot");
  const uint32_t red_chunk = msm_red_chunk(cfg, nbatch * s.nproof, (uint32_t)s.world, hidden != 0);
  const uint32_t cps = ceil_div(cfg.B, red_chunk);
  const uint32_t sets = (uint32_t)cfg.D * s.nproof;
  const uint32_t nchunks = cps * sets;
  uint32_t nblk = ceil_div(cps / (uint32_t)s.world, HOOK_SUM_THREADS * 2);
  if (nblk > 256) nblk = 256;
  if (nblk < 1) nblk = 1;
  const uint32_t ncontrib = nchunks + contrib_pad;
  const int wsets = (int)sets + 1;  // one spare set per workspace slot: it must stay untouched

  uint32_t meta[4];
  fetch(meta, s.large_meta(g2), 4);
  need(meta[1] <= hot_cap, "stage hook: the hot-bucket list exceeds its buffer");
  fetch(hot, s.large_list(g2), meta[1]);
  if (s.world > 1) fetch(range, s.range.p, 6);

  for (uint64_t i = 0; i < ncodes; ++i)
    need(codes[i] == CODE_INF || codes[i] == CODE_POISON || (codes[i] >= 0 && (uint32_t)codes[i] < npool * nlam),
         "stage hook: a code names no pool point");
  DevBuf<Affine<F>> dpool;
  DevBuf<F> dlam;
  DevBuf<int32_t> dcodes;
  upload(dpool, pool, npool);
  upload(dlam, lam, nlam);
  upload(dcodes, codes, ncodes);

  MsmWork<F> work;
  work.init(slots, ncontrib, wsets, (int)nbatch);
  G16_LAUNCH((k_fill_partials<F>), ceil_div(ncodes, BLOCK), BLOCK, 0, 0, (const int32_t*)dcodes.p,
             (const Affine<F>*)dpool.p, npool, (const F*)dlam.p, nlam, work.partial.p, (size_t)ncodes);
  poison(work.contrib);
  poison(work.bsum);
  poison(work.wsum);
  const size_t rec = (size_t)nbatch * sizeof(MsmAcc<F>);
  if (s.nproof > 1) need(out_stride >= rec && out_stride % 4 == 0, "stage hook: out_stride is smaller than a record");
  const size_t out_bytes = s.nproof > 1 ? (size_t)s.nproof * out_stride : rec;
  DevBuf<uint8_t> dout;
  dout.alloc(out_bytes);
  poison(dout);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());

  geo[0] = red_chunk; geo[1] = cps; geo[2] = nchunks; geo[3] = nblk; geo[4] = sets; geo[5] = S;
  geo[6] = lanes; geo[7] = slots; geo[8] = ncontrib; geo[9] = (uint32_t)wsets; geo[10] = M; geo[11] = meta[1];

  msm_reduce_head<F>(s, work, 0, (int)nbatch, 0, nullptr, hidden != 0);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());
  to_affine_host<F>(work.contrib.p, (size_t)nbatch * ncontrib, contrib_out, contrib_flag);  // the snapshot
  msm_reduce_tail<F>(s, work, 0, (int)nbatch, reinterpret_cast<MsmAcc<F>*>(dout.p), 0, nullptr, hidden != 0,
                     s.nproof > 1 ? (size_t)out_stride : 0);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());
  to_affine_host<F>(work.wsum.p, (size_t)nbatch * wsets, wsum_out, wsum_flag);

  // the records, proof by proof, and the bytes between them
  std::vector<uint8_t> raw(out_bytes);
  G16_HIP(hipMemcpy(raw.data(), dout.p, out_bytes, hipMemcpyDeviceToHost));
  uint64_t dirty = 0;
  for (uint32_t z = 0; z < s.nproof; ++z) {
    const size_t base = (size_t)z * (s.nproof > 1 ? out_stride : 0);
    to_affine_host<F>(reinterpret_cast<const MsmAcc<F>*>(dout.p + base), nbatch,
                      (uint8_t*)sums_out + (size_t)z * nbatch * sizeof(Affine<F>), sums_flag + (size_t)z * nbatch);
    const size_t gap_end = z + 1 < s.nproof ? base + out_stride : out_bytes;
    for (size_t k = base + rec; k < gap_end; ++k) dirty += raw[k] != POISON;
  }
  *gap_dirty = dirty;
}

// info: 8 words: S, lanes, slots, M, overflow slot 0, overflow slot 1, MSM_FIX_CAP, workspace slots

// mode 0: init(pts_a), msm_accumulate.  1 / 2: init_pair(pts_a, pts_b), msm_accumulate of the first / second half.
// 3: init_pair, msm_accumulate_pair (G1 only: the product has no G2 pair launch; idx_min must be 0).  partial_out: `workspace slots` x slots points
template <class F>
void acc_hook(const SortArgs& a, const void* pts_a, const void* pts_b, uint32_t npts, uint32_t idx_min, int mode,
              uint32_t* info, uint32_t* offset, uint32_t* entries, uint64_t entries_cap, void* partial_out,
              uint8_t* partial_flag, uint64_t partial_cap) {
  constexpr bool g2 = sizeof(F) != sizeof(Fq);
  need(mode >= 0 && mode <= 3, "stage hook: bad mode");
  need(a.nproof == 1 && a.world <= 1, "stage hook: the accumulate hook takes one unsharded proof");
  need(pts_a && (mode == 0 || pts_b), "stage hook: missing points");
  // every entry names point idx - idx_min of the query, idx < n1
  need((uint64_t)npts + idx_min >= a.n1 && npts >= 1, "stage hook: fewer points than scalars above idx_min");
  need(mode != 3 || idx_min == 0, "stage hook: the pair launch has no idx_min");
  need(mode != 3 || !g2, "stage hook: there is no G2 pair launch");
  MsmSort s;
  DevBuf<U256> dscal;
  run_sort(a, s, dscal);
  const uint32_t nbt = s.nbt(), lanes = s.lanes_of(g2);
  fetch(offset, s.offset.p, (size_t)nbt + 1);
  const uint32_t M = offset[nbt];
  need(M <= entries_cap && M <= s.entries.n, "stage hook: offset[nb] exceeds the entry buffer");
  fetch(entries, s.entries.p, M);
  const uint64_t slots64 = (uint64_t)nbt + lanes;
  need(slots64 < (1ull << 31), "stage hook: too many slots");
  const uint32_t slots = (uint32_t)slots64;
  const int batch = mode == 3 ? 2 : 1;
  need((uint64_t)batch * slots <= partial_cap, "stage hook: the partial buffer is too small");

  MsmPoints<F> A, B;
  if (mode == 0) A.init(reinterpret_cast<const Affine<F>*>(pts_a), npts, s.cfg, 0);
  else MsmPoints<F>::init_pair(A, B, reinterpret_cast<const Affine<F>*>(pts_a),
                               reinterpret_cast<const Affine<F>*>(pts_b), npts, s.cfg, 0);
  MsmWork<F> work;
  work.init(slots, 1, 1, batch);
  poison(work.partial);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());
  if constexpr (!g2) {
    if (mode == 3) msm_accumulate_pair<F>(s, A, B, work, 0, 0);
  }
  if (mode != 3) msm_accumulate<F>(s, mode == 2 ? B : A, idx_min, work, 0, 0);
  G16_HIP(hipGetLastError());
  G16_HIP(hipDeviceSynchronize());

  std::vector<MsmFixList> fix((size_t)batch);
  G16_HIP(hipMemcpy(fix.data(), work.fix.p, fix.size() * sizeof(MsmFixList), hipMemcpyDeviceToHost));
  info[0] = msm_seg_len(M, lanes); info[1] = lanes; info[2] = slots; info[3] = M;
  info[4] = fix[0].overflow; info[5] = batch > 1 ? fix[1].overflow : 0u; info[6] = MSM_FIX_CAP; info[7] = (uint32_t)batch;
  to_affine_host<F>(work.partial.p, (size_t)batch * slots, partial_out, partial_flag);
}

}  // namespace

#define STAGE_REDUCE(NAME, F)                                                                                          \
  extern "C" int NAME(const uint32_t* scalars, uint32_t n1, int mont, int c, int planes, uint32_t nproof,             \
                      uint64_t stride, int rank, int world, uint32_t lanes, uint32_t lanes2, uint32_t nbatch,         \
                      int hidden, uint64_t out_stride, const void* pool, uint32_t npool, const void* lam,             \
                      uint32_t nlam, const int32_t* codes, uint64_t ncodes, uint32_t contrib_pad, uint32_t* geo,      \
                      uint32_t* offset, uint32_t* hot, uint32_t hot_cap, uint32_t* range, void* contrib_out,          \
                      uint8_t* contrib_flag, void* wsum_out, uint8_t* wsum_flag, void* sums_out, uint8_t* sums_flag,  \
                      uint64_t* gap_dirty, char* msg, size_t msg_len) {                                               \
    return guarded(msg, msg_len, [&] {                                                                                \
      const SortArgs a{scalars, n1, mont, c, planes, nproof, stride, rank, world, lanes, lanes2};                     \
      reduce_hook<F>(a, nbatch, hidden, out_stride, pool, npool, lam, nlam, codes, ncodes, contrib_pad, geo, offset,  \
                     hot, hot_cap, range, contrib_out, contrib_flag, wsum_out, wsum_flag, sums_out, sums_flag,        \
                     gap_dirty);                                                                                      \
    });                                                                                                               \
  }
STAGE_REDUCE(g16_test_stage_reduce_g1, Fq)
STAGE_REDUCE(g16_test_stage_reduce_g2, Fq2)

#define STAGE_ACC(NAME, F)                                                                                             \
  extern "C" int NAME(const uint32_t* scalars, uint32_t n1, int mont, int c, int planes, uint32_t lanes,              \
                      uint32_t lanes2, const void* pts_a, const void* pts_b, uint32_t npts, uint32_t idx_min,         \
                      int mode, uint32_t* info, uint32_t* offset, uint32_t* entries, uint64_t entries_cap,            \
                      void* partial_out, uint8_t* partial_flag, uint64_t partial_cap, char* msg, size_t msg_len) {    \
    return guarded(msg, msg_len, [&] {                                                                                \
      const SortArgs a{scalars, n1, mont, c, planes, 1u, 0, 0, 1, lanes, lanes2};                                     \
      acc_hook<F>(a, pts_a, pts_b, npts, idx_min, mode, info, offset, entries, entries_cap, partial_out,              \
                  partial_flag, partial_cap);                                                                         \
    });                                                                                                               \
  }
STAGE_ACC(g16_test_stage_acc_g1, Fq)
STAGE_ACC(g16_test_stage_acc_g2, Fq2)

// the lane counts, slot count and reduction chunk the two hooks above would use: launches nothing
extern "C" int g16_test_stage_plan(uint64_t len, int c, int planes, uint32_t nbatch, uint32_t nproof, int world,
                                   int hidden, uint32_t* out) {
  const MsmConfig cfg = msm_make_config((size_t)len, c, planes);
  out[0] = msm_red_chunk(cfg, nbatch * nproof, (uint32_t)world, hidden != 0);
  out[1] = cfg.lanes;
  out[2] = cfg.lanes2;
  out[3] = MSM_FIX_CAP;
  return 0;
}
