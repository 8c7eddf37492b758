// msm_bases.hip -- the MSM engine over bases the caller supplies (include/g16_amd.h: g16_msm_bases_create, g16_msm,
// g16_msm_once).  ark-ec VariableBaseMSM::msm / msm_bigint for any bases: until now the engine of
// msm.h was reachable only through g16_msm_g1 / g16_msm_g2 over the queries of a resident key.
//
// Nothing of the engine is forked.  The points are ingested by MsmPoints::init / init_from_device (k_precompute_planes:
// packed Montgomery affine -> the packed Lazy<F> form, plus the planes), the scalars sorted by MsmSort::run -- with
// nproof vectors per chunk, the batched-proving path -- and summed by msm_run (k_bucket_accumulate, k_acc_fixup with
// the exact kernel behind it, k_combine_large, k_bucket_reduce, k_set_sum, k_horner).  What is new here is host
// orchestration: the memory plan of the planes, the chunking of many scalar vectors, the optional point predicates
// (keycheck.h, ahead of the ingestion) and the affine conversion of a chunk's sums (ec29.h).
#include "msm_bases.h"

#include <algorithm>
#include <memory>

#include "keycheck.h"

using namespace g16;

namespace g16 {

namespace {

constexpr size_t MB_MAX_POINTS = (size_t)1 << MSM_IDX_BITS_WIDE;

// one lane per sum of the chunk: XYZZ over the lazy limbs -> affine, storage form
template <class F>
__global__ void __launch_bounds__(64) k_mb_affine(const MsmAcc<F>* sums, uint32_t count, Affine<F>* out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  const auto p = sums[i].template to_affine<true>();
  out[i] = p.inf ? Affine<F>::infinity() : Affine<F>{p.x.to_mont256(), p.y.to_mont256()};
}

g16_status mb_fail(g16_status code, const std::string& msg) {
  set_create_error(msg);
  return code;
}

// vectors per chunk the sort can index for this configuration: entries and buckets of a chunk are 32-bit, and a
// level-1 sort partition should not span more than the 4096 buckets of the level-2 LDS histogram (msm.h)
uint32_t clamp_batch(uint32_t want, uint32_t n, const MsmConfig& cfg) {
  const uint64_t ent = std::max<uint64_t>((uint64_t)n * cfg.W, 1);
  const uint64_t part_cap = (uint64_t)4096 << MSM_PART_BITS_MAX;
  uint64_t b = std::min<uint64_t>({(uint64_t)want, (((uint64_t)1 << 32) - 1) / ent, part_cap / cfg.nb()});
  return (uint32_t)std::max<uint64_t>(b, 1);
}

template <class F>
size_t state_bytes(uint32_t n, const MsmConfig& cfg, uint32_t b) {
  const uint32_t slots = b * cfg.nb() + cfg.max_lanes();
  return (size_t)cfg.Pn * n * sizeof(Affine<F>) + MsmSort::bytes_for(n, cfg, b) +
         msm_work_bytes<F>(slots, msm_contrib_cap(cfg, b), (int)b * cfg.D, 1) + (size_t)b * n * sizeof(Fr);
}

// The memory plan (as plan_msm_configs does for a ctx): full planes when everything fits what is free on the device
// less a margin of 2 GiB + 2 % (never more than a quarter of it), else the largest plane count that does.
template <class F>
MsmConfig plan_config(uint32_t n, const g16_msm_options& o, uint32_t* batch) {
  const uint32_t want = o.max_batch > 0 ? (uint32_t)o.max_batch : 1u;
  MsmConfig cfg = msm_make_config(n ? n : 1, o.window_bits, o.planes);
  *batch = clamp_batch(want, n, cfg);
  if (o.planes > 0) return cfg;  // the caller's choice: an allocation failure is reported as such
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return cfg;
  const size_t budget = fr - std::min(((size_t)2 << 30) + fr / 50, fr / 4);
  for (int pn = cfg.Pn; pn >= 1; --pn) {
    const MsmConfig c = msm_make_config(n ? n : 1, o.window_bits, pn);
    const uint32_t b = clamp_batch(want, n, c);
    if (state_bytes<F>(n, c, b) <= budget) {
      *batch = b;
      return c;
    }
  }
  throw std::runtime_error("the bases do not fit this device's memory even with one plane per point (" +
                           std::to_string(fr >> 20) + " MiB free)");
}

const char* reason_name(uint8_t f) {
  if (f & G16_KEY_BAD_NONCANONICAL) return "a coordinate is not canonical (>= q)";
  if (f & G16_KEY_BAD_OFF_CURVE) return "the point is not on the curve";
  return "the point is outside the prime-order subgroup";
}

// the per-point predicates of g16_key_check over n points in device memory; returns the first bad index or -1
int64_t first_bad_point(int group, const void* dpts, uint32_t n, uint8_t* reason, hipStream_t s) {
  DevBuf<uint8_t> dflags;
  dflags.alloc(n);
  if (group == G16_GROUP_G1) {
    G16_LAUNCH(k_chk_flags_g1, ceil_div(n, KC_BLOCK), KC_BLOCK, 0, s, (const G1Affine*)dpts, n, dflags.p);
  } else {
    DevBuf<VkDev> dvk;
    dvk.alloc(1);
    std::unique_ptr<VkDev> hv(new VkDev());
    memset((void*)hv.get(), 0, sizeof(VkDev));
    vk_consts(hv.get());
    G16_HIP(hipMemcpyAsync(dvk.p, hv.get(), sizeof(VkDev), hipMemcpyHostToDevice, s));
    G16_LAUNCH(k_chk_flags_g2, ceil_div(n, KC_BLOCK), KC_BLOCK, 0, s, (const VkDev*)dvk.p, (const G2Affine*)dpts, n, 1u,
               dflags.p);
    G16_HIP(hipStreamSynchronize(s));  // dvk and hv live until the kernel has run
  }
  G16_HIP(hipGetLastError());
  std::vector<uint8_t> hf(n);
  G16_HIP(hipMemcpyAsync(hf.data(), dflags.p, n, hipMemcpyDeviceToHost, s));
  G16_HIP(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < n; ++i)
    if (hf[i] & ~KC_INF) {
      *reason = hf[i] & ~KC_INF;
      return i;
    }
  return -1;
}

template <class F>
void init_group(g16_msm_bases* h, MsmPoints<F>& pts, MsmWork<F>& work, DevBuf<MsmAcc<F>>& sums, const void* points,
                bool on_device, bool validate, const g16_msm_options& o) {
  const uint32_t n = h->n;
  h->cfg = plan_config<F>(n, o, &h->batch);
  hipStream_t s = h->stream;
  DevBuf<uint8_t> tmp;
  const void* dpts = points;
  if (n && !on_device && validate) {  // the predicates read the storage form: they run before the ingestion converts it
    tmp.alloc((size_t)n * sizeof(Affine<F>));
    G16_HIP(hipMemcpyAsync(tmp.p, points, tmp.bytes(), hipMemcpyHostToDevice, s));
    dpts = tmp.p;
  }
  if (n && validate) {
    uint8_t reason = 0;
    const int64_t bad = first_bad_point(h->group, dpts, n, &reason, s);
    if (bad >= 0) throw std::invalid_argument("point " + std::to_string(bad) + ": " + reason_name(reason));
    h->validated = true;
  }
  if (on_device || validate) pts.init_from_device((const Affine<F>*)dpts, n, h->cfg, s);
  else pts.init((const Affine<F>*)points, n, h->cfg, s);
  G16_HIP(hipGetLastError());
  if (n) {
    h->sort.init(n, h->cfg, h->batch);
    work.init(h->batch * h->cfg.nb() + h->cfg.max_lanes(), msm_contrib_cap(h->cfg, h->batch), (int)h->batch * h->cfg.D, 1);
    h->stage.alloc((size_t)h->batch * n);
  }
  sums.alloc(h->batch);
  h->out_dev.alloc((size_t)h->batch * h->psize());
  h->bad.alloc(1);
  G16_HIP(hipStreamSynchronize(s));  // tmp and the caller's points are no longer read
}

}  // namespace

void msm_bases_chunk(g16_msm_bases* h, const Fr* scal, uint32_t len, uint32_t b, size_t stride) {
  hipStream_t s = h->stream;
  if (b < 1 || b > h->batch || len > h->n) throw std::runtime_error("msm_bases_chunk: chunk out of range");
  if (!len) {
    G16_HIP(hipMemsetAsync(h->out_dev.p, 0, (size_t)b * h->psize(), s));
    return;
  }
  h->sort.run(scal, len, true, s, b, stride);
  if (h->group == G16_GROUP_G1) {
    msm_run<Fq>(h->sort, h->p1, 0, h->w1, h->s1.p, s, nullptr, sizeof(MsmAcc<Fq>));
    G16_LAUNCH((k_mb_affine<Fq>), ceil_div(b, 64), 64, 0, s, (const MsmAcc<Fq>*)h->s1.p, b, (G1Affine*)h->out_dev.p);
  } else {
    msm_run<Fq2>(h->sort, h->p2, 0, h->w2, h->s2.p, s, nullptr, sizeof(MsmAcc<Fq2>));
    G16_LAUNCH((k_mb_affine<Fq2>), ceil_div(b, 64), 64, 0, s, (const MsmAcc<Fq2>*)h->s2.p, b, (G2Affine*)h->out_dev.p);
  }
  G16_HIP(hipGetLastError());
}

}  // namespace g16

extern "C" g16_status g16_msm_bases_create(int device, int group, const void* points, size_t n, uint32_t flags,
                                           const g16_msm_options* opt, g16_msm_bases** out) {
  if (!out) return mb_fail(G16_ERR_INVALID, "g16_msm_bases_create: null argument");
  *out = nullptr;
  if (group != G16_GROUP_G1 && group != G16_GROUP_G2) return mb_fail(G16_ERR_INVALID, "g16_msm_bases_create: unknown group");
  if (n > MB_MAX_POINTS) return mb_fail(G16_ERR_INVALID, "g16_msm_bases_create: more than 2^27 points");
  if (n && !points) return mb_fail(G16_ERR_INVALID, "g16_msm_bases_create: null argument");
  if (const g16_status ds = device_ok(device)) return mb_fail(ds, "g16_msm_bases_create: no usable device (there is no CPU fallback)");
  g16_msm_options o{0, 0, 1, 0};
  if (opt) o = *opt;
  std::unique_ptr<g16_msm_bases> h;
  try {
    G16_HIP(hipSetDevice(device));
    h.reset(new g16_msm_bases);
    h->device = device;
    h->group = group;
    h->n = (uint32_t)n;
    G16_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const bool on_device = (flags & G16_MSM_POINTS_DEVICE) != 0;
    if (group == G16_GROUP_G1) init_group<Fq>(h.get(), h->p1, h->w1, h->s1, points, on_device, o.validate != 0, o);
    else init_group<Fq2>(h.get(), h->p2, h->w2, h->s2, points, on_device, o.validate != 0, o);
  } catch (const std::invalid_argument& e) {
    return mb_fail(G16_ERR_INVALID, std::string("g16_msm_bases_create: ") + e.what());
  } catch (const HipError& e) {
    return mb_fail(G16_ERR_HIP, e.what());
  } catch (const std::exception& e) {
    return mb_fail(G16_ERR_INTERNAL, e.what());
  }
  *out = h.release();
  return G16_OK;
}

extern "C" void g16_msm_bases_destroy(g16_msm_bases* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

extern "C" g16_status g16_msm_bases_info(const g16_msm_bases* h, uint32_t out[8]) {
  if (!h || !out) return G16_ERR_INVALID;
  out[0] = (uint32_t)h->group;
  out[1] = h->n;
  out[2] = (uint32_t)h->cfg.c;
  out[3] = (uint32_t)h->cfg.W;
  out[4] = (uint32_t)h->cfg.Pn;
  out[5] = (uint32_t)h->cfg.D;
  out[6] = h->batch;
  out[7] = h->validated ? 1u : 0u;
  return G16_OK;
}

extern "C" g16_status g16_msm(g16_msm_bases* h, const void* scalars, size_t len, size_t count, size_t stride,
                              uint32_t flags, uint8_t* out) {
  if (!h) return mb_fail(G16_ERR_INVALID, "g16_msm: null argument");
  if (count == 0) return G16_OK;
  if (!out || (len && !scalars)) return mb_fail(G16_ERR_INVALID, "g16_msm: null argument");
  if (len > h->n) return mb_fail(G16_ERR_INVALID, "g16_msm: more scalars than bases");
  if (count > 1 && stride < len) return mb_fail(G16_ERR_INVALID, "g16_msm: stride below len");
  if (count == 1) stride = len;
  const size_t ps = h->psize();
  if (len == 0) {
    memset(out, 0, count * ps);
    return G16_OK;
  }
  const bool canon = (flags & G16_MSM_SCALARS_CANONICAL) != 0, on_dev = (flags & G16_MSM_SCALARS_DEVICE) != 0;
  std::lock_guard<std::mutex> lock(h->mu);
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const Fr* in = (const Fr*)scalars;
    for (size_t k0 = 0; k0 < count; k0 += h->batch) {
      const uint32_t b = (uint32_t)std::min<size_t>(h->batch, count - k0);
      const Fr* src = in + k0 * stride;
      size_t st = stride;
      unsigned long long bad = INGEST_NONE;
      if (canon || !on_dev) {  // into the staging buffer, vectors back to back
        for (uint32_t k = 0; k < b; ++k)
          G16_HIP(hipMemcpyAsync(h->stage.p + (size_t)k * len, in + (k0 + k) * stride, len * sizeof(Fr),
                                 on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        if (canon) {
          G16_HIP(hipMemcpyAsync(h->bad.p, &bad, 8, hipMemcpyHostToDevice, s));
          fr_from_canonical_enqueue(h->stage.p, h->stage.p, (size_t)b * len, h->bad.p, s);
        }
        src = h->stage.p;
        st = len;
      }
      msm_bases_chunk(h, src, (uint32_t)len, b, st);
      if (canon) G16_HIP(hipMemcpyAsync(&bad, h->bad.p, 8, hipMemcpyDeviceToHost, s));
      G16_HIP(hipMemcpyAsync(out + k0 * ps, h->out_dev.p, (size_t)b * ps, hipMemcpyDeviceToHost, s));
      G16_HIP(hipStreamSynchronize(s));
      if (bad != INGEST_NONE) {
        const unsigned long long at = (unsigned long long)k0 * len + bad;
        return mb_fail(G16_ERR_INVALID, "g16_msm: scalar " + std::to_string(at) + " (vector " + std::to_string(at / len) +
                                            ", element " + std::to_string(at % len) + ") is >= the field modulus");
      }
    }
    return G16_OK;
  }, mb_fail);
}

extern "C" g16_status g16_msm_once(int device, int group, const void* points, const void* scalars, size_t n,
                                   uint32_t flags, uint8_t* out) {
  if (!out) return mb_fail(G16_ERR_INVALID, "g16_msm_once: null argument");
  if (n > MB_MAX_POINTS) return mb_fail(G16_ERR_INVALID, "g16_msm_once: more than 2^27 points");
  if (n && (!points || !scalars)) return mb_fail(G16_ERR_INVALID, "g16_msm_once: null argument");
  const g16_msm_options o{0, 1, 1, 0};  // one plane: D = W bucket sets folded by k_horner, no precomputation
  g16_msm_bases* h = nullptr;
  g16_status st = g16_msm_bases_create(device, group, points, n, flags & G16_MSM_POINTS_DEVICE, &o, &h);
  if (st != G16_OK) return st;
  st = g16_msm(h, scalars, n, 1, n, flags & (G16_MSM_SCALARS_CANONICAL | G16_MSM_SCALARS_DEVICE), out);
  g16_msm_bases_destroy(h);
  return st;
}
