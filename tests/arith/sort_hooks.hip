// sort_hooks.hip -- TEST INFRASTRUCTURE ONLY: host wrappers that drive MsmSort (csrc/msm.h, csrc/msm_sort.hip) alone
// -- scalars in, the sorted (bucket -> entries) view, the level-1 partition offsets, the shard range and the
// hot-bucket lists out -- so that pytest can compare every array the accumulation and reduction kernels read from a
// sort with an exact integer model (tests/sort_model.py), at sizes no elliptic-curve reference could afford.
//
// Only the public interface of msm.h is used: msm_make_config, MsmSort::init / set_shard / run / init_view /
// run_view.  There is no kernel in this file.
//
// Built twice from this one file (csrc/Makefile): with g++ against the SIMT emulator into
// tests/emu/libg16_emu.so and with hipcc and the product flags into tests/arith/libg16_sort_gpu.so (linked with the
// product's own msm_sort.o).  Never linked into, loaded by or reachable from libg16_amd.so.
//
// Every wrapper returns 0, a HIP error code, or -1 with the message of the std::runtime_error in msg.
#include "common.h"
#include "msm.h"

using namespace g16;

namespace {

constexpr int CFG_WORDS = 11;  // c, W, Pn, D, B, idx_bits, lanes, lanes2, nb, part_shift, part_bits

void put_config(const MsmConfig& cfg, uint32_t* out) {
  out[0] = (uint32_t)cfg.c;
  out[1] = (uint32_t)cfg.W;
  out[2] = (uint32_t)cfg.Pn;
  out[3] = (uint32_t)cfg.D;
  out[4] = cfg.B;
  out[5] = cfg.idx_bits;
  out[6] = cfg.lanes;
  out[7] = cfg.lanes2;
  out[8] = cfg.nb();
  out[9] = (uint32_t)msm_part_shift(cfg.nb());
  out[10] = (uint32_t)msm_part_bits(cfg.nb());
}

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

void fetch(uint32_t* host, const uint32_t* dev, size_t words) {
  if (words) G16_HIP(hipMemcpy(host, dev, words * 4, hipMemcpyDeviceToHost));
}

}  // namespace

// msm_make_config alone: launches nothing.  out: CFG_WORDS words.
extern "C" int g16_test_sort_config(uint64_t len, int c, int planes, uint32_t* out) {
  put_config(msm_make_config((size_t)len, c, planes), out);
  return 0;
}

// MsmSort::init alone, for its refusals (they come before the first allocation).
extern "C" int g16_test_sort_init(uint64_t capacity, int c, int planes, uint32_t nproof_cap, char* msg,
                                  size_t msg_len) {
  return guarded(msg, msg_len, [&] {
    if (capacity >> 32) throw std::runtime_error("sort hook: capacity is a 32-bit count");
    MsmSort s;
    s.init((uint32_t)capacity, msm_make_config((size_t)capacity, c, planes), nproof_cap);
  });
}

// One sort.  scalars: proof z's n1 scalars (8 words each; Montgomery Fr when mont) at scalars + 8 z stride words.
// cap / nproof_cap: what init is given (0: n1 / nproof), the configuration is msm_make_config(cap, c, planes)
// with lanes / lanes2 (when not 0) in place of its lane counts.  world > 1: set_shard(rank, world).
// keep_bits (ceil(n1 / 32) words, or NULL): a view of the sort is run as well, and count / offset / entries /
// the hot-bucket lists are the VIEW's; part_off is always the source sort's.
// Outputs: cfg_out[CFG_WORDS]; count, offset: nproof nb + 1 words; entries: offset[nproof nb] words (refused when
// more than entries_cap); part_off: bins1 + 1 words (<= 4097); range: 6 words when sharded; multi_l / multi_l2:
// the listed buckets (refused when more than multi_cap); meta_out = {meta[1], meta2[1]}.
extern "C" int g16_test_sort_run(const uint32_t* scalars, uint32_t n1, int mont, int c, int planes, uint32_t nproof,
                                 uint64_t stride, int rank, int world, uint32_t lanes, uint32_t lanes2,
                                 const uint32_t* keep_bits, uint32_t cap, uint32_t nproof_cap, uint32_t* cfg_out,
                                 uint32_t* count, uint32_t* offset, uint32_t* entries, uint64_t entries_cap,
                                 uint32_t* part_off, uint32_t* range, uint32_t* multi_l, uint32_t* multi_l2,
                                 uint32_t multi_cap, uint32_t* meta_out, char* msg, size_t msg_len) {
  return guarded(msg, msg_len, [&] {
    if (!cap) cap = n1;
    if (!nproof_cap) nproof_cap = nproof;
    MsmConfig cfg = msm_make_config(cap, c, planes);
    if (lanes) cfg.lanes = lanes;
    if (lanes2) cfg.lanes2 = lanes2;
    put_config(cfg, cfg_out);

    const size_t nscal = nproof > 1 ? (size_t)(nproof - 1) * stride + n1 : n1;
    DevBuf<U256> dscal;
    dscal.alloc(nscal ? nscal : 1);
    if (nscal) G16_HIP(hipMemcpy(dscal.p, scalars, nscal * sizeof(U256), hipMemcpyHostToDevice));

    MsmSort src, view;
    src.init(cap, cfg, nproof_cap);
    if (world > 1) src.set_shard(rank, world);
    src.run(dscal.p, n1, mont != 0, 0, nproof, (size_t)stride);
    MsmSort* res = &src;
    DevBuf<uint32_t> dkeep;
    if (keep_bits) {
      const size_t kw = ((size_t)n1 + 31) / 32;
      dkeep.alloc(kw ? kw : 1);
      if (kw) G16_HIP(hipMemcpy(dkeep.p, keep_bits, kw * 4, hipMemcpyHostToDevice));
      view.init_view(cap, cfg, nproof_cap);
      view.run_view(src, dkeep.p, 0);
      res = &view;
    }
    G16_HIP(hipGetLastError());
    G16_HIP(hipDeviceSynchronize());

    const uint32_t nb = res->nbt();
    fetch(count, res->count.p, (size_t)nb + 1);
    fetch(offset, res->offset.p, (size_t)nb + 1);
    if (offset[nb] > entries_cap || offset[nb] > res->entries.n)
      throw std::runtime_error("sort hook: offset[nb] exceeds the entry buffer");
    fetch(entries, res->entries.p, offset[nb]);
    const int sh = msm_part_shift(nb);
    fetch(part_off, src.part_off.p, (size_t)((nb - 1) >> sh) + 2);
    if (world > 1) fetch(range, src.range.p, 6);
    uint32_t m[4];
    fetch(m, res->meta.p, 4);
    meta_out[0] = m[1];
    fetch(m, res->meta2.p, 4);
    meta_out[1] = m[1];
    if (meta_out[0] > multi_cap || meta_out[0] > res->multi_l.n || meta_out[1] > multi_cap ||
        meta_out[1] > res->multi_l2.n)
      throw std::runtime_error("sort hook: a hot-bucket list exceeds its buffer");
    fetch(multi_l, res->multi_l.p, meta_out[0]);
    fetch(multi_l2, res->multi_l2.p, meta_out[1]);
  });
}
