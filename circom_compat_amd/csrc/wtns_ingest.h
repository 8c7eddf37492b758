// wtns_ingest.h -- canonical little-endian Fr values -> the Montgomery form of the witness buffers, on the
// device (wtns_ingest.hip).  The inverse direction of the digit sort's and h_canon's to_canonical.
#pragma once
#include "common.h"

namespace g16 {

// "no element was >= r": the value the caller presets *first_bad to (all ones)
static constexpr unsigned long long INGEST_NONE = ~0ull;

// Enqueues one launch over n elements: out[i] = Montgomery(in[i]) when in[i] < r; otherwise out[i] = 0 and
// *first_bad = min(*first_bad, i).  in == out is allowed (a lane reads its element before it writes it).
// first_bad: one 64-bit word in device memory, preset to INGEST_NONE; only failing lanes touch it.
void fr_from_canonical_enqueue(const void* in_le, Fr* out, size_t n, unsigned long long* first_bad, hipStream_t s);

}  // namespace g16
