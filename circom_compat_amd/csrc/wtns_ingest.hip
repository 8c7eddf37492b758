// wtns_ingest.hip -- canonical witness ingestion: the 32-byte little-endian integers of a snarkjs .wtns
// (rapidsnark, circom's C++ calculator) become the 4 x u64 Montgomery form of the ctx's witness buffer on the
// device, range test included.  32 bytes in, 32 bytes out, one Montgomery product per element: the host loop
// this replaces (loaders.cpp, wtns_parse) does the same product one element after the other.
#include "wtns_ingest.h"

#include "hostcall.h"

namespace g16 {
namespace {

constexpr int INGEST_BLOCK = 256;

// g16_fr_convert_times: device milliseconds of the calling thread's last g16_fr_convert
enum { T_UPLOAD = 0, T_CONVERT, T_DOWNLOAD, T_COUNT };
thread_local PhaseTimes<T_COUNT> t_phase;

struct Events {  // the four marks around the three phases, on the null stream
  EventBox e[T_COUNT + 1];
  Events() {
    for (auto& x : e) x.create(true);
  }
  void mark(int i) { G16_HIP(hipEventRecord(e[i].e, nullptr)); }
  void collect() {
    G16_HIP(hipEventSynchronize(e[T_COUNT].e));
    t_phase.take(Stored::REPLACE, e, {{0, 1, T_UPLOAD}, {1, 2, T_CONVERT}, {2, 3, T_DOWNLOAD}});
  }
};

// One lane per element, consecutive lanes read consecutive elements (U256 is 16-byte aligned: two 128-bit
// loads, two 128-bit stores).  No LDS.  in and out may be the same buffer.
__global__ void __launch_bounds__(INGEST_BLOCK) k_fr_from_canonical(const U256* in, Fr* out, uint64_t n,
                                                                   unsigned long long* first_bad) {
  const uint64_t i = (uint64_t)blockIdx.x * INGEST_BLOCK + threadIdx.x;
  if (i >= n) return;
  const U256 u = in[i];
  // v < r  <=>  v - r borrows
  uint64_t br = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) br = (((uint64_t)u.v[j] - FrParams::MOD[j] - br) >> 32) & 1;
  Fr m = Fr::from_canonical(u);
  if (!br) {  // nothing unreduced leaves this kernel; the smallest failing index wins whatever the schedule
    m = Fr::zero();
    atomicMin(first_bad, (unsigned long long)i);
  }
  out[i] = m;
}

}  // namespace

void fr_from_canonical_enqueue(const void* in_le, Fr* out, size_t n, unsigned long long* first_bad, hipStream_t s) {
  if (!n) return;
  G16_LAUNCH(k_fr_from_canonical, ceil_div(n, INGEST_BLOCK), INGEST_BLOCK, 0, s, (const U256*)in_le, out,
             (uint64_t)n, first_bad);
  G16_HIP(hipGetLastError());
}

}  // namespace g16

using namespace g16;

extern "C" g16_status g16_fr_convert(int device, const uint8_t* in_le, uint64_t* out_mont, size_t n,
                                     int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  if (n == 0) return G16_OK;
  if (!in_le || !out_mont) {
    set_create_error("g16_fr_convert: null argument");
    return G16_ERR_INVALID;
  }
  if (n >= ((size_t)1 << 31) * INGEST_BLOCK) {  // one launch: the grid holds fewer than 2^31 blocks
    set_create_error("g16_fr_convert: 2^39 elements or more");
    return G16_ERR_INVALID;
  }
  if (const g16_status ds = device_ok(device)) {
    if (ds == G16_ERR_INVALID) set_create_error("g16_fr_convert: device out of range");
    return ds;
  }
  return guarded_call([&]() -> g16_status {
    G16_HIP(hipSetDevice(device));
    DevBuf<Fr> buf;
    DevBuf<unsigned long long> bad;
    buf.alloc(n);
    bad.alloc(1);
    unsigned long long bad_host = INGEST_NONE;
    Events ev;
    t_phase.clear();
    ev.mark(T_UPLOAD);
    G16_HIP(hipMemcpy(buf.p, in_le, n * 32, hipMemcpyHostToDevice));
    G16_HIP(hipMemcpy(bad.p, &bad_host, 8, hipMemcpyHostToDevice));
    ev.mark(T_CONVERT);
    fr_from_canonical_enqueue(buf.p, buf.p, n, bad.p, nullptr);
    ev.mark(T_DOWNLOAD);
    G16_HIP(hipMemcpy(&bad_host, bad.p, 8, hipMemcpyDeviceToHost));
    if (bad_host == INGEST_NONE) G16_HIP(hipMemcpy(out_mont, buf.p, n * 32, hipMemcpyDeviceToHost));
    ev.mark(T_COUNT);
    ev.collect();
    if (bad_host != INGEST_NONE) {
      if (first_bad) *first_bad = (int64_t)bad_host;
      set_create_error("g16_fr_convert: element " + std::to_string(bad_host) + " is >= the field modulus");
      return G16_ERR_INVALID;
    }
    return G16_OK;
  });
}

extern "C" g16_status g16_fr_convert_times(float* ms, uint32_t cap) {
  return t_phase.read(ms, cap);
}
