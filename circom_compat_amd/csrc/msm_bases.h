// msm_bases.h -- private definition of g16_msm_bases (the opaque handle of include/g16_amd.h): the MSM engine of
// msm.h over bases a caller supplies.  Shared by msm_bases.hip (the handle and g16_msm) and kzg.hip (the commitment
// key is such a handle and feeds it quotients that never leave the device).
#pragma once
#include <mutex>

#include "../../include/g16_amd.h"

#include "msm.h"
#include "wtns_ingest.h"

struct g16_msm_bases {
  int device = 0, group = G16_GROUP_G1;
  uint32_t n = 0;      // points
  uint32_t batch = 1;  // scalar vectors per chunk: what the sort and the workspaces are sized for
  bool validated = false;
  g16::MsmConfig cfg;
  g16::MsmPoints<g16::Fq> p1;
  g16::MsmPoints<g16::Fq2> p2;
  g16::MsmSort sort;
  g16::MsmWork<g16::Fq> w1;
  g16::MsmWork<g16::Fq2> w2;
  g16::DevBuf<g16::Fr> stage;            // [batch][n]: scalars that arrive from the host or in canonical form
  g16::DevBuf<g16::MsmAcc<g16::Fq>> s1;  // [batch] sums of a chunk (lazy XYZZ)
  g16::DevBuf<g16::MsmAcc<g16::Fq2>> s2;
  g16::DevBuf<uint8_t> out_dev;          // [batch] affine results in the storage form
  g16::DevBuf<unsigned long long> bad;   // first canonical scalar >= r of a chunk (wtns_ingest.h)
  hipStream_t stream = nullptr;
  std::mutex mu;  // one call in flight per handle
  size_t psize() const { return group == G16_GROUP_G2 ? 128 : 64; }
  ~g16_msm_bases() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace g16 {

void set_create_error(const std::string& msg);  // api.hip: what g16_last_error(NULL) returns

// One chunk on h->stream (the caller holds h->mu and has set the device): b <= h->batch vectors of len <= h->n
// Montgomery scalars in device memory, vector k at scal + k * stride -> b affine points at h->out_dev.  One sort,
// one accumulation, one reduction.  len == 0: b points at infinity.  Enqueues only.
void msm_bases_chunk(g16_msm_bases* h, const Fr* scal, uint32_t len, uint32_t b, size_t stride);

}  // namespace g16
