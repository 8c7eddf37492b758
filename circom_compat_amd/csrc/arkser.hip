// arkser.hip -- arkworks' canonical serialization (ark-serialize 0.4 / 0.5, BN254) to and from the packed
// Montgomery encoding of the rest of the ABI, on the GPU: g16_points_from_ark / g16_points_to_ark and the
// ProvingKey / VerifyingKey / Proof containers on top of them (include/g16_amd.h, "arkworks serialization").
//
// THE FORMAT IS WRITTEN FROM KNOWLEDGE OF arkworks: neither ark-serialize nor a Rust toolchain was at hand.  What
// pins it are known arkworks byte strings of single points (the compressed generators of G1 and G2, their
// negatives and the points at infinity; tests/test_ark_codec.py); no arkworks build was available to cross-check
// a whole ProvingKey blob.  ark-serialize 0.3 (another flag layout) is not supported.
//
//   Fq        32 bytes, the canonical (non-Montgomery) integer, little-endian; Fq2 = c0 | c1
//   flags     top two bits of the LAST byte of a record: 0x80 = "y is negative" (y > -y on canonical integers;
//             in Fq2 lexicographic with c1 first), 0x40 = the point at infinity; both = invalid
//   G1        compressed x (32 bytes), uncompressed x | y (64);  G2  x.c0 | x.c1 (64),  x.c0 | x.c1 | y.c0 | y.c1 (128)
//   infinity  all-zero coordinates + 0x40.  The writer sets the sign bit in uncompressed form too; the reader
//             IGNORES it there.
// Deviation from arkworks, on purpose: a record with the infinity flag and any other bit set is rejected
// (G16_KEY_BAD_ENCODING).  arkworks ignores those bits; a canonical writer never produces them, and accepting them
// would give one point many encodings.
//
// Kernels, one lane per point, KC_BLOCK lanes per block:
//   k_ak_decode<F>  flags -> canonical range -> curve; the reason byte is the FIRST test that fails, the record of
//                   a bad point is all-zero.  Compressed: y from the square root of x^3 + b (arkser.h: one 252-bit
//                   Fq exponentiation on G1, two on G2, no inversion, the verdict is the final y^2 == x^3 + b),
//                   then the root whose sign matches the flag.
//   k_ak_subgroup   G2 with G16_ARK_VALIDATE: [r] P = infinity (keycheck.h) for the points that decoded.
//   k_ak_encode<F>  Montgomery -> canonical, the sign flag, the infinity encoding; a stored word >= q is bad, the
//                   curve is not tested.
//   k_ak_count      one block: the chunk's bad points into the call's counter (a scan, no atomics).
// Arrays stream through two page-locked host slots and two device slots of min(2^18, n) points
// (G16_ARKSER_CHUNK=<points> overrides, tests): the host stages chunk k + 1 and its copy runs while the kernels of
// chunk k do, the results of chunk k come back on a third stream.  Standalone: no ctx is needed or touched.
#include <stdlib.h>

#include <memory>

#include "arkser.h"
#include "keycheck.h"

namespace g16 {
namespace {

constexpr uint32_t AK_DEFAULT_CHUNK = 1u << 18;

G16_HD void ak_load(Fq& f, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f.v[i] = w[i];
}
G16_HD void ak_load(Fq2& f, const uint32_t* w) {
  ak_load(f.c0, w);
  ak_load(f.c1, w + 8);
}
G16_HD void ak_store(uint32_t* w, const Fq& f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = f.v[i];
}
G16_HD void ak_store(uint32_t* w, const Fq2& f) {
  ak_store(w, f.c0);
  ak_store(w + 8, f.c1);
}
G16_HD uint32_t& ak_top(Fq& f) { return f.v[7]; }
G16_HD uint32_t& ak_top(Fq2& f) { return f.c1.v[7]; }
G16_HD bool ak_canonical(const Fq& f) { return fq_words_canonical(f); }
G16_HD bool ak_canonical(const Fq2& f) { return fq2_words_canonical(f); }
G16_HD Fq ak_to_mont(const Fq& raw) { return raw * Fq::r2(); }
G16_HD Fq2 ak_to_mont(const Fq2& raw) { return Fq2{ak_to_mont(raw.c0), ak_to_mont(raw.c1)}; }
G16_HD bool ak_sqrt(const Fq& a, Fq* r) { return fq_sqrt(a, r); }
G16_HD bool ak_sqrt(const Fq2& a, Fq2* r) { return fq2_sqrt(a, r); }

// in: n records of W (compressed) or 2 W words, W = words of F; b: the curve's constant, Montgomery
template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_ak_decode(const uint32_t* in, uint32_t n, uint32_t flags, F b,
                                                        Affine<F>* out, uint8_t* reason) {
  constexpr uint32_t W = sizeof(F) / 4;
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const bool comp = (flags & G16_ARK_COMPRESSED) != 0;
  const uint32_t* rec = in + (size_t)i * (comp ? W : 2 * W);
  F x, y = F::zero();
  ak_load(x, rec);
  if (!comp) ak_load(y, rec + W);
  uint32_t fl;  // bit 1: 0x80 negative, bit 0: 0x40 infinity
  if (comp) {
    fl = ak_top(x) >> 30;
    ak_top(x) &= 0x3fffffffu;
  } else {
    fl = ak_top(y) >> 30;
    ak_top(y) &= 0x3fffffffu;
  }
  uint8_t why = 0;
  Affine<F> p = Affine<F>::infinity();
  if (fl == 3) {
    why = G16_KEY_BAD_ENCODING;
  } else if (fl & 1) {
    if (!(x.is_zero() && y.is_zero())) why = G16_KEY_BAD_ENCODING;
  } else if (!(ak_canonical(x) && ak_canonical(y))) {
    why = G16_KEY_BAD_NONCANONICAL;
  } else {
    x = ak_to_mont(x);
    const F rhs = x.sqr() * x + b;
    if (comp) {
      if (!ak_sqrt(rhs, &y)) why = G16_KEY_BAD_OFF_CURVE;
      else if (ak_is_negative(y) != ((fl >> 1) != 0)) y = y.neg();
    } else {
      y = ak_to_mont(y);
      if (y.sqr() != rhs) why = G16_KEY_BAD_OFF_CURVE;
    }
    if (!why) p = Affine<F>{x, y};
  }
  out[i] = p;
  reason[i] = why;
}

// G2 with G16_ARK_VALIDATE, behind k_ak_decode<Fq2>: a point that decoded and is not in the r-torsion becomes
// G16_KEY_BAD_SUBGROUP and an all-zero record.  A kernel of its own: the 254-bit double-and-add needs the registers
// of k_chk_flags_g2, the square roots of the decode far fewer.
__global__ void __launch_bounds__(KC_BLOCK) k_ak_subgroup(G2Affine* pts, uint32_t n, uint8_t* reason) {
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n || reason[i]) return;
  const G2Affine p = pts[i];
  if (p.is_inf() || g2_r_torsion(p)) return;
  pts[i] = G2Affine::infinity();
  reason[i] = G16_KEY_BAD_SUBGROUP;
}

template <class F>
__global__ void __launch_bounds__(KC_BLOCK) k_ak_encode(const Affine<F>* in, uint32_t n, uint32_t flags, uint32_t* out,
                                                        uint8_t* reason) {
  constexpr uint32_t W = sizeof(F) / 4;
  const uint32_t i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const bool comp = (flags & G16_ARK_COMPRESSED) != 0;
  uint32_t* rec = out + (size_t)i * (comp ? W : 2 * W);
  const Affine<F> p = in[i];
  F x = F::zero(), y = F::zero();
  uint32_t fl = 0;
  uint8_t why = 0;
  if (!(ak_canonical(p.x) && ak_canonical(p.y))) {
    why = G16_KEY_BAD_NONCANONICAL;
  } else if (p.is_inf()) {
    fl = 1;
  } else {
    x = ak_from_mont(p.x);
    y = ak_from_mont(p.y);
    fl = ak_canon_negative(y) ? 2 : 0;
  }
  ak_top(comp ? x : y) |= fl << 30;
  ak_store(rec, x);
  if (!comp) ak_store(rec + W, y);
  reason[i] = why;
}

// one block: *total += the number of non-zero reason bytes of the chunk (segments, then lane 0 in lane order)
__global__ void __launch_bounds__(KC_SCAN) k_ak_count(const uint8_t* reason, uint32_t n, uint64_t* total) {
  __shared__ uint32_t sh[KC_SCAN];
  const uint32_t t = threadIdx.x;
  const uint32_t seg = (n + KC_SCAN - 1) / KC_SCAN;
  const uint32_t lo = t * seg < n ? t * seg : n, hi = lo + seg < n ? lo + seg : n;
  uint32_t bad = 0;
#pragma unroll 1
  for (uint32_t i = lo; i < hi; ++i) bad += reason[i] ? 1 : 0;
  sh[t] = bad;
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < KC_SCAN; ++k) run += sh[k];
    *total += run;
  }
}

size_t ark_bytes(int group, uint32_t flags) {
  return (group == G16_POINT_G2 ? 64 : 32) * ((flags & G16_ARK_COMPRESSED) ? 1 : 2);
}
size_t packed_bytes(int group) { return group == G16_POINT_G2 ? 128 : 64; }

void gather(uint8_t* dst, const uint8_t* src, size_t stride, size_t rec, uint32_t n) {
  if (stride == rec) {
    memcpy(dst, src, (size_t)n * rec);
    return;
  }
  for (uint32_t i = 0; i < n; ++i) memcpy(dst + (size_t)i * rec, src + (size_t)i * stride, rec);
}
void scatter(uint8_t* dst, size_t stride, const uint8_t* src, size_t rec, uint32_t n) {
  if (stride == rec) {
    memcpy(dst, src, (size_t)n * rec);
    return;
  }
  for (uint32_t i = 0; i < n; ++i) memcpy(dst + (size_t)i * stride, src + (size_t)i * rec, rec);
}

// both directions: decode = arkworks bytes in, packed points out
g16_status run_codec(bool decode, int device, int group, uint32_t flags, const uint8_t* in, size_t in_stride, uint64_t n,
                     uint8_t* out, size_t out_stride, uint8_t* reason_out, size_t reason_stride, uint64_t* n_bad) {
  if (n_bad) *n_bad = 0;
  if ((group != G16_POINT_G1 && group != G16_POINT_G2) || (flags & ~(uint32_t)(G16_ARK_COMPRESSED | G16_ARK_VALIDATE)))
    return G16_ERR_INVALID;
  const size_t in_rec = decode ? ark_bytes(group, flags) : packed_bytes(group);
  const size_t out_rec = decode ? packed_bytes(group) : ark_bytes(group, flags);
  if (!in_stride) in_stride = in_rec;
  if (!out_stride) out_stride = out_rec;
  if (!reason_stride) reason_stride = 1;
  if (in_stride < in_rec || out_stride < out_rec) return G16_ERR_INVALID;
  if (n == 0) return G16_OK;
  if (!in || !out) return G16_ERR_INVALID;
  if (const g16_status ds = device_ok(device)) return ds;
  return guarded_call([&]() -> g16_status {
    const uint32_t chunk = chunk_from_env("G16_ARKSER_CHUNK", AK_DEFAULT_CHUNK, n);
    const uint64_t n_chunks = (n + chunk - 1) / chunk;

    G16_HIP(hipSetDevice(device));
    // a slot: the chunk's input records | its output records | one reason byte per point
    const size_t off_out = (size_t)chunk * in_rec, off_why = off_out + (size_t)chunk * out_rec;
    const size_t slot_bytes = off_why + (((size_t)chunk + 15) & ~(size_t)15);
    PinnedBuf pin[2];
    DevBuf<uint8_t> dslot[2];
    DevBuf<uint64_t> dbad;
    StreamBox copy, comp, down;
    EventBox up[2], done[2], back[2];
    for (int s = 0; s < 2; ++s) {
      pin[s].alloc(slot_bytes);
      dslot[s].alloc(slot_bytes);
      up[s].create();
      done[s].create();
      back[s].create();
    }
    dbad.alloc(1);
    copy.create();
    comp.create();
    down.create();
    G16_HIP(hipMemsetAsync(dbad.p, 0, sizeof(uint64_t), comp.s));
    const Fq b1 = Fq::from_u32(3);
    const Fq2 b2 = host_consts().b_twist;

    for (uint64_t k = 0; k < n_chunks + 2; ++k) {
      const int s = (int)(k & 1);
      if (k >= 2) {  // the results of the chunk that used this slot two chunks ago
        const uint64_t at = (k - 2) * chunk;
        const uint32_t c = (uint32_t)(n - at < chunk ? n - at : chunk);
        G16_HIP(hipEventSynchronize(back[s].e));
        scatter(out + at * out_stride, out_stride, pin[s].p + off_out, out_rec, c);
        if (reason_out) scatter(reason_out + at * reason_stride, reason_stride, pin[s].p + off_why, 1, c);
      }
      if (k >= n_chunks) continue;
      const uint64_t at = k * chunk;
      const uint32_t c = (uint32_t)(n - at < chunk ? n - at : chunk);
      uint8_t* d = dslot[s].p;
      gather(pin[s].p, in + at * in_stride, in_stride, in_rec, c);
      G16_HIP(hipMemcpyAsync(d, pin[s].p, (size_t)c * in_rec, hipMemcpyHostToDevice, copy.s));
      G16_HIP(hipEventRecord(up[s].e, copy.s));
      G16_HIP(hipStreamWaitEvent(comp.s, up[s].e, 0));
      const uint32_t nb = ceil_div(c, KC_BLOCK);
      if (decode && group == G16_POINT_G1)
        G16_LAUNCH((k_ak_decode<Fq>), nb, KC_BLOCK, 0, comp.s, (const uint32_t*)d, c, flags, b1,
                   (G1Affine*)(d + off_out), d + off_why);
      else if (decode) {
        G16_LAUNCH((k_ak_decode<Fq2>), nb, KC_BLOCK, 0, comp.s, (const uint32_t*)d, c, flags, b2,
                   (G2Affine*)(d + off_out), d + off_why);
        if (flags & G16_ARK_VALIDATE)
          G16_LAUNCH(k_ak_subgroup, nb, KC_BLOCK, 0, comp.s, (G2Affine*)(d + off_out), c, d + off_why);
      }
      else if (group == G16_POINT_G1)
        G16_LAUNCH((k_ak_encode<Fq>), nb, KC_BLOCK, 0, comp.s, (const G1Affine*)d, c, flags, (uint32_t*)(d + off_out),
                   d + off_why);
      else
        G16_LAUNCH((k_ak_encode<Fq2>), nb, KC_BLOCK, 0, comp.s, (const G2Affine*)d, c, flags, (uint32_t*)(d + off_out),
                   d + off_why);
      G16_LAUNCH(k_ak_count, 1, KC_SCAN, 0, comp.s, (const uint8_t*)(d + off_why), c, dbad.p);
      G16_HIP(hipEventRecord(done[s].e, comp.s));
      G16_HIP(hipStreamWaitEvent(down.s, done[s].e, 0));
      G16_HIP(hipMemcpyAsync(pin[s].p + off_out, d + off_out, (size_t)c * out_rec, hipMemcpyDeviceToHost, down.s));
      G16_HIP(hipMemcpyAsync(pin[s].p + off_why, d + off_why, c, hipMemcpyDeviceToHost, down.s));
      G16_HIP(hipEventRecord(back[s].e, down.s));
    }
    G16_HIP(hipGetLastError());
    G16_HIP(hipStreamSynchronize(comp.s));
    uint64_t bad = 0;
    G16_HIP(hipMemcpy(&bad, dbad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (n_bad) *n_bad = bad;
    return G16_OK;
  });
}

const char* reason_text(uint8_t why) {
  switch (why) {
    case G16_KEY_BAD_NONCANONICAL: return "a coordinate is not below q";
    case G16_KEY_BAD_OFF_CURVE: return "not on the curve";
    case G16_KEY_BAD_SUBGROUP: return "not in the r-torsion subgroup";
    case G16_KEY_BAD_ENCODING: return "invalid flag bits";
    default: return "bad point";
  }
}

// ---- containers -----------------------------------------------------------------------------------------
bool field_is_g2(int f) {
  return f == G16_ARK_F_BETA_G2 || f == G16_ARK_F_GAMMA_G2 || f == G16_ARK_F_DELTA_G2 || f == G16_ARK_F_B2;
}

// one field of a container from the blob into dst (count x packed bytes); the first bad point is the error
g16_status decode_field(int device, uint32_t flags, const uint8_t* data, const g16_ark_layout& lay, int f, uint8_t* dst) {
  const uint64_t n = lay.count[f];
  if (!n) return G16_OK;
  std::vector<uint8_t> why(n);
  uint64_t bad = 0;
  const int group = field_is_g2(f) ? G16_POINT_G2 : G16_POINT_G1;
  const g16_status st =
      run_codec(true, device, group, flags, data + lay.offset[f], 0, n, dst, 0, why.data(), 1, &bad);
  if (st != G16_OK) return loader_fail(st, std::string("decoding ") + ark_field_name(f) + " failed");
  if (bad)
    for (uint64_t i = 0; i < n; ++i)
      if (why[i])
        return loader_fail(G16_ERR_IO, std::string(ark_field_name(f)) + "[" + std::to_string(i) + "]: " +
                                           reason_text(why[i]) + " (" + std::to_string(bad) + " bad in this array)");
  return G16_OK;
}

g16_status encode_field(int device, uint32_t flags, int f, const uint8_t* src, uint64_t n, uint8_t* dst) {
  if (!n) return G16_OK;
  if (!src) return loader_fail(G16_ERR_INVALID, std::string(ark_field_name(f)) + " is NULL");
  uint64_t bad = 0;
  const int group = field_is_g2(f) ? G16_POINT_G2 : G16_POINT_G1;
  const g16_status st = run_codec(false, device, group, flags, src, 0, n, dst, 0, nullptr, 1, &bad);
  if (st != G16_OK) return loader_fail(st, std::string("encoding ") + ark_field_name(f) + " failed");
  if (bad) return loader_fail(G16_ERR_INVALID, std::string(ark_field_name(f)) + ": " + std::to_string(bad) + " point(s) with a word >= q");
  return G16_OK;
}

// the single points of a container, all of one group, in ONE codec call (one set of staging slots for up to three
// points instead of one per point); the message still names the field
struct SingleIn {
  int f;
  uint8_t* dst;
};
g16_status decode_singles(int device, uint32_t flags, const uint8_t* data, const g16_ark_layout& lay, const SingleIn* s,
                          int n) {
  const int group = field_is_g2(s[0].f) ? G16_POINT_G2 : G16_POINT_G1;
  const size_t rec = ark_bytes(group, flags), pk = packed_bytes(group);
  uint8_t in[3 * 128], dec[3 * 128], why[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) memcpy(in + i * rec, data + lay.offset[s[i].f], rec);
  uint64_t bad = 0;
  const g16_status st = run_codec(true, device, group, flags, in, 0, (uint64_t)n, dec, 0, why, 1, &bad);
  if (st != G16_OK) return loader_fail(st, std::string("decoding ") + ark_field_name(s[0].f) + " failed");
  for (int i = 0; i < n; ++i) {
    if (why[i]) return loader_fail(G16_ERR_IO, std::string(ark_field_name(s[i].f)) + "[0]: " + reason_text(why[i]));
    memcpy(s[i].dst, dec + i * pk, pk);
  }
  return G16_OK;
}

struct SingleOut {
  int f;
  const uint8_t* src;
  size_t at;  // where its record goes in the blob
};
g16_status encode_singles(int device, uint32_t flags, const SingleOut* s, int n, uint8_t* out) {
  const int group = field_is_g2(s[0].f) ? G16_POINT_G2 : G16_POINT_G1;
  const size_t rec = ark_bytes(group, flags), pk = packed_bytes(group);
  uint8_t in[3 * 128], enc[3 * 128];
  for (int i = 0; i < n; ++i) memcpy(in + i * pk, s[i].src, pk);
  uint64_t bad = 0;
  const g16_status st = run_codec(false, device, group, flags, in, 0, (uint64_t)n, enc, 0, nullptr, 1, &bad);
  if (st != G16_OK) return loader_fail(st, std::string("encoding ") + ark_field_name(s[0].f) + " failed");
  if (bad) return loader_fail(G16_ERR_INVALID, "a single point of the key has a word >= q");
  for (int i = 0; i < n; ++i) memcpy(out + s[i].at, enc + i * rec, rec);
  return G16_OK;
}

void put_u64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }

}  // namespace
}  // namespace g16

using namespace g16;

struct g16_ark_pk {
  std::vector<uint8_t> ic, a, b1, b2, h, l;
  g16_key_desc key;
  g16_vk_desc vk;
};

extern "C" g16_status g16_points_from_ark(int device, int group, uint32_t flags, const uint8_t* in, size_t in_stride,
                                          uint64_t n, uint8_t* out, size_t out_stride, uint8_t* reason_out,
                                          uint64_t* n_bad) {
  return run_codec(true, device, group, flags, in, in_stride, n, out, out_stride, reason_out, 1, n_bad);
}

extern "C" g16_status g16_points_to_ark(int device, int group, uint32_t flags, const uint8_t* in, size_t in_stride,
                                        uint64_t n, uint8_t* out, size_t out_stride, uint64_t* n_bad) {
  uint64_t bad = 0;
  const g16_status st = run_codec(false, device, group, flags, in, in_stride, n, out, out_stride, nullptr, 1, &bad);
  if (n_bad) *n_bad = bad;
  return st == G16_OK && bad ? G16_ERR_INVALID : st;
}

extern "C" g16_status g16_ark_proofs_read(int device, uint32_t flags, const uint8_t* in, uint64_t n, uint8_t* proofs_out,
                                          uint8_t* reason_out, uint64_t* n_bad) {
  if (n_bad) *n_bad = 0;
  if (n && (!in || !proofs_out)) return loader_fail(G16_ERR_INVALID, "g16_ark_proofs_read: NULL argument");
  const size_t g1 = ark_bytes(G16_POINT_G1, flags), g2 = ark_bytes(G16_POINT_G2, flags), rec = 2 * g1 + g2;
  const size_t in_off[3] = {0, g1, g1 + g2}, out_off[3] = {0, 64, 192};
  std::vector<uint8_t> own;
  try {
    if (!reason_out) {
      own.assign((size_t)n * 3, 0);
      reason_out = own.data();
    }
  } catch (const std::exception&) {
    return loader_fail(G16_ERR_INTERNAL, "g16_ark_proofs_read: out of memory");
  }
  uint64_t total = 0;
  for (int k = 0; k < 3; ++k) {
    uint64_t bad = 0;
    const g16_status st = run_codec(true, device, k == 1 ? G16_POINT_G2 : G16_POINT_G1, flags, in + in_off[k], rec, n,
                                    proofs_out + out_off[k], G16_PROOF_BYTES, reason_out + k, 3, &bad);
    if (st != G16_OK) return loader_fail(st, "g16_ark_proofs_read: the codec did not run");
    total += bad;
  }
  if (n_bad) *n_bad = total;
  if (total)
    for (uint64_t i = 0; i < 3 * n; ++i)
      if (reason_out[i])
        return loader_fail(G16_ERR_IO, "proof " + std::to_string(i / 3) + ", point " + "abc"[i % 3] + ": " +
                                           reason_text(reason_out[i]) + " (" + std::to_string(total) + " bad point(s))");
  return G16_OK;
}

extern "C" g16_status g16_ark_proofs_write(int device, uint32_t flags, const uint8_t* proofs, uint64_t n, uint8_t* out,
                                           uint64_t* n_bad) {
  if (n_bad) *n_bad = 0;
  if (n && (!proofs || !out)) return G16_ERR_INVALID;
  const size_t g1 = ark_bytes(G16_POINT_G1, flags), g2 = ark_bytes(G16_POINT_G2, flags), rec = 2 * g1 + g2;
  const size_t out_off[3] = {0, g1, g1 + g2}, in_off[3] = {0, 64, 192};
  uint64_t total = 0;
  for (int k = 0; k < 3; ++k) {
    uint64_t bad = 0;
    const g16_status st = run_codec(false, device, k == 1 ? G16_POINT_G2 : G16_POINT_G1, flags, proofs + in_off[k],
                                    G16_PROOF_BYTES, n, out + out_off[k], rec, nullptr, 1, &bad);
    if (st != G16_OK) return st;
    total += bad;
  }
  if (n_bad) *n_bad = total;
  return total ? G16_ERR_INVALID : G16_OK;
}

extern "C" uint64_t g16_ark_vk_size(uint32_t flags, uint64_t n_public) {
  const uint64_t g1 = ark_bytes(G16_POINT_G1, flags), g2 = ark_bytes(G16_POINT_G2, flags);
  return g1 + 3 * g2 + 8 + (n_public + 1) * g1;
}

extern "C" uint64_t g16_ark_pk_size(uint32_t flags, uint64_t n_vars, uint64_t n_public, uint64_t h_len) {
  const uint64_t g1 = ark_bytes(G16_POINT_G1, flags), g2 = ark_bytes(G16_POINT_G2, flags);
  const uint64_t n_l = n_vars > n_public ? n_vars - n_public - 1 : 0;
  return g16_ark_vk_size(flags, n_public) + 2 * g1 + 5 * 8 + n_vars * (2 * g1 + g2) + (h_len + n_l) * g1;
}

extern "C" g16_status g16_ark_vk_read(int device, uint32_t flags, const uint8_t* data, size_t len, g16_vk_desc* vk,
                                      uint8_t* ic_out, uint32_t ic_cap) {
  if (!vk || !ic_out) return loader_fail(G16_ERR_INVALID, "g16_ark_vk_read: NULL argument");
  g16_ark_layout lay;
  g16_status st = g16_ark_vk_layout(data, len, flags, &lay);
  if (st != G16_OK) return st;
  if (lay.count[G16_ARK_F_IC] > ic_cap) return loader_fail(G16_ERR_INVALID, "g16_ark_vk_read: ic_out is too small");
  const SingleIn s1[1] = {{G16_ARK_F_ALPHA_G1, vk->alpha_g1}};
  const SingleIn s2[3] = {{G16_ARK_F_BETA_G2, vk->beta_g2}, {G16_ARK_F_GAMMA_G2, vk->gamma_g2}, {G16_ARK_F_DELTA_G2, vk->delta_g2}};
  if ((st = decode_singles(device, flags, data, lay, s1, 1)) != G16_OK) return st;
  if ((st = decode_singles(device, flags, data, lay, s2, 3)) != G16_OK) return st;
  if ((st = decode_field(device, flags, data, lay, G16_ARK_F_IC, ic_out)) != G16_OK) return st;
  vk->ic = ic_out;
  vk->ic_count = (uint32_t)lay.count[G16_ARK_F_IC];
  return G16_OK;
}

namespace {
// the VerifyingKey at out, and with key != NULL the two G1 points behind it (the G1 singles share one call);
// *at: the bytes written
g16_status write_fixed(int device, uint32_t flags, const g16_vk_desc* vk, const g16_key_desc* key, uint8_t* out, size_t* at) {
  const size_t g1 = ark_bytes(G16_POINT_G1, flags), g2 = ark_bytes(G16_POINT_G2, flags);
  const size_t ic_at = g1 + 3 * g2 + 8, vk_end = ic_at + (size_t)vk->ic_count * g1;
  const SingleOut s1[3] = {{G16_ARK_F_ALPHA_G1, vk->alpha_g1, 0},
                           {G16_ARK_F_BETA_G1, key ? key->beta_g1 : nullptr, vk_end},
                           {G16_ARK_F_DELTA_G1, key ? key->delta_g1 : nullptr, vk_end + g1}};
  const SingleOut s2[3] = {{G16_ARK_F_BETA_G2, vk->beta_g2, g1},
                           {G16_ARK_F_GAMMA_G2, vk->gamma_g2, g1 + g2},
                           {G16_ARK_F_DELTA_G2, vk->delta_g2, g1 + 2 * g2}};
  g16_status st;
  if ((st = encode_singles(device, flags, s1, key ? 3 : 1, out)) != G16_OK) return st;
  if ((st = encode_singles(device, flags, s2, 3, out)) != G16_OK) return st;
  put_u64(out + ic_at - 8, vk->ic_count);
  if ((st = encode_field(device, flags, G16_ARK_F_IC, vk->ic, vk->ic_count, out + ic_at)) != G16_OK) return st;
  *at = vk_end + (key ? 2 * g1 : 0);
  return G16_OK;
}
}  // namespace

extern "C" g16_status g16_ark_vk_write(int device, uint32_t flags, const g16_vk_desc* vk, uint8_t* out, size_t cap) {
  if (!vk || !out || !vk->ic || vk->ic_count < 1) return loader_fail(G16_ERR_INVALID, "g16_ark_vk_write: bad argument");
  if (cap < g16_ark_vk_size(flags, vk->ic_count - 1)) return loader_fail(G16_ERR_INVALID, "g16_ark_vk_write: out is too small");
  size_t at = 0;
  return write_fixed(device, flags, vk, nullptr, out, &at);
}

extern "C" g16_status g16_ark_pk_read(int device, uint32_t flags, const uint8_t* data, size_t len, g16_ark_pk** out) {
  if (!out) return loader_fail(G16_ERR_INVALID, "g16_ark_pk_read: NULL argument");
  *out = nullptr;
  g16_ark_layout lay;
  g16_status st = g16_ark_pk_layout(data, len, flags, &lay);
  if (st != G16_OK) return st;
  try {
    std::unique_ptr<g16_ark_pk> h(new g16_ark_pk());
    const uint64_t N = lay.count[G16_ARK_F_A], n_ic = lay.count[G16_ARK_F_IC], h_len = lay.count[G16_ARK_F_H];
    uint64_t dom = 1;
    while (dom < h_len) dom <<= 1;
    h->ic.assign(n_ic * 64, 0);
    h->a.assign(N * 64, 0);
    h->b1.assign(N * 64, 0);
    h->b2.assign(N * 128, 0);
    h->h.assign(dom * 64, 0);  // beyond h_len: infinity (a libsnark key has domain - 1 points)
    h->l.assign(lay.count[G16_ARK_F_L] * 64, 0);
    memset(&h->key, 0, sizeof h->key);
    memset(&h->vk, 0, sizeof h->vk);
    uint8_t* dst[G16_ARK_N_FIELDS] = {h->vk.alpha_g1, h->vk.beta_g2, h->vk.gamma_g2, h->vk.delta_g2,
                                      h->ic.data(),   h->key.beta_g1, h->key.delta_g1, h->a.data(),
                                      h->b1.data(),   h->b2.data(),   h->h.data(),     h->l.data()};
    const SingleIn s1[3] = {{G16_ARK_F_ALPHA_G1, dst[G16_ARK_F_ALPHA_G1]},
                            {G16_ARK_F_BETA_G1, dst[G16_ARK_F_BETA_G1]},
                            {G16_ARK_F_DELTA_G1, dst[G16_ARK_F_DELTA_G1]}};
    const SingleIn s2[3] = {{G16_ARK_F_BETA_G2, dst[G16_ARK_F_BETA_G2]},
                            {G16_ARK_F_GAMMA_G2, dst[G16_ARK_F_GAMMA_G2]},
                            {G16_ARK_F_DELTA_G2, dst[G16_ARK_F_DELTA_G2]}};
    if ((st = decode_singles(device, flags, data, lay, s1, 3)) != G16_OK) return st;
    if ((st = decode_singles(device, flags, data, lay, s2, 3)) != G16_OK) return st;
    for (int f : {G16_ARK_F_IC, G16_ARK_F_A, G16_ARK_F_B1, G16_ARK_F_B2, G16_ARK_F_H, G16_ARK_F_L})
      if ((st = decode_field(device, flags, data, lay, f, dst[f])) != G16_OK) return st;
    h->vk.ic = h->ic.data();
    h->vk.ic_count = (uint32_t)n_ic;
    h->key.n_vars = (uint32_t)N;
    h->key.n_public = (uint32_t)(n_ic - 1);
    h->key.domain_size = (uint32_t)dom;
    h->key.a_query = h->a.data();
    h->key.b_g1_query = h->b1.data();
    h->key.b_g2_query = h->b2.data();
    h->key.l_query = h->l.data();
    h->key.h_query = h->h.data();
    memcpy(h->key.alpha_g1, h->vk.alpha_g1, 64);
    memcpy(h->key.beta_g2, h->vk.beta_g2, 128);
    memcpy(h->key.delta_g2, h->vk.delta_g2, 128);
    *out = h.release();
    return G16_OK;
  } catch (const std::exception&) {
    return loader_fail(G16_ERR_INTERNAL, "g16_ark_pk_read: out of memory");
  }
}

extern "C" g16_status g16_ark_pk_key(const g16_ark_pk* h, g16_key_desc* key, g16_vk_desc* vk) {
  if (!h || !key) return G16_ERR_INVALID;
  *key = h->key;
  if (vk) *vk = h->vk;
  return G16_OK;
}

extern "C" void g16_ark_pk_close(g16_ark_pk* h) { delete h; }

extern "C" g16_status g16_ark_pk_write(int device, uint32_t flags, const g16_key_desc* key, const g16_vk_desc* vk,
                                       uint64_t h_len, uint8_t* out, size_t cap) {
  if (!key || !vk || !out || !vk->ic) return loader_fail(G16_ERR_INVALID, "g16_ark_pk_write: NULL argument");
  const uint64_t N = key->n_vars, p = key->n_public;
  if (N < 1 || p + 1 > N || vk->ic_count != p + 1 || h_len > key->domain_size)
    return loader_fail(G16_ERR_INVALID, "g16_ark_pk_write: inconsistent key sizes");
  if (cap < g16_ark_pk_size(flags, N, p, h_len)) return loader_fail(G16_ERR_INVALID, "g16_ark_pk_write: out is too small");
  const size_t g1 = ark_bytes(G16_POINT_G1, flags), g2 = ark_bytes(G16_POINT_G2, flags);
  size_t o = 0;
  g16_status st = write_fixed(device, flags, vk, key, out, &o);
  if (st != G16_OK) return st;
  const struct {
    int f;
    const void* src;
    uint64_t n;
  } vecs[5] = {{G16_ARK_F_A, key->a_query, N},
               {G16_ARK_F_B1, key->b_g1_query, N},
               {G16_ARK_F_B2, key->b_g2_query, N},
               {G16_ARK_F_H, key->h_query, h_len},
               {G16_ARK_F_L, key->l_query, N - p - 1}};
  for (const auto& v : vecs) {
    put_u64(out + o, v.n);
    o += 8;
    if ((st = encode_field(device, flags, v.f, (const uint8_t*)v.src, v.n, out + o)) != G16_OK) return st;
    o += (size_t)v.n * (field_is_g2(v.f) ? g2 : g1);
  }
  return G16_OK;
}
