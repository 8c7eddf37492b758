// hostcall.h -- what every entry point without a ctx starts and ends with, one copy:
//   device_ok, chunk_from_env          the refusals and the test knob in front of the work
//   PinnedBuf, StreamBox, EventBox     the RAII boxes of a call's page-locked memory, streams and events
//   k_phase_mark, PhaseTimes, PhaseClock   the phase times behind the ..._times exports
//   guarded_call                       no exception leaves an extern "C" function; its message is kept
#pragma once
#include <stdlib.h>

#include <chrono>
#include <initializer_list>
#include <type_traits>

#include "../../include/g16_amd.h"

#include "common.h"

namespace g16 {
void set_create_error(const std::string& msg);  // api.hip: what g16_last_error(NULL) returns

struct PinnedBuf {
  uint8_t* p = nullptr;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  void alloc(size_t bytes) { G16_HIP(hipHostMalloc((void**)&p, bytes, hipHostMallocPortable)); }
};
struct StreamBox {
  hipStream_t s = nullptr;
  bool made = false;
  ~StreamBox() {
    if (made) (void)hipStreamDestroy(s);
  }
  void create() {
    G16_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    made = true;
  }
};
struct EventBox {
  hipEvent_t e = nullptr;
  bool made = false;
  ~EventBox() {
    if (made) (void)hipEventDestroy(e);
  }
  // timed: the event closes or opens a span of PhaseTimes::take; otherwise it only orders streams
  void create(bool timed = false) {
    if (timed) G16_HIP(hipEventCreate(&e));
    else G16_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    made = true;
  }
};

// G16_OK, or what an entry point returns for this device number
inline g16_status device_ok(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G16_ERR_NO_DEVICE;
  return device < 0 || device >= ndev ? G16_ERR_INVALID : G16_OK;
}

// <name>=<points> (tests): points per staged chunk; never more than the longest array needs
inline uint32_t chunk_from_env(const char* name, uint32_t dflt, uint64_t longest) {
  uint32_t chunk = dflt;
  if (const char* e = getenv(name)) {
    const unsigned long long v = strtoull(e, nullptr, 0);
    if (v >= 1 && v <= (1ull << 24)) chunk = (uint32_t)v;
  }
  if (longest < 1) longest = 1;
  return chunk > longest ? (uint32_t)longest : chunk;
}

// ---- phase times -------------------------------------------------------------------------------------
namespace {  // a kernel: each including file gets its own instance, as in keycheck.h

// Launched in front of the event that opens a timed phase.  An event recorded behind an idle stretch of its stream
// can take the time of the command BEFORE the gap (the copy of the chunk before), and the phase would then count
// the gap; behind this kernel it takes the time at which the phase's own work is about to start.  (A template, so
// that only the files that launch it carry an instance: G16_LAUNCH(k_phase_mark<>, 1, 1, 0, stream).)
template <int = 0>
__global__ void k_phase_mark() {}

}  // namespace

// the device time from event `first` to event `last` of a call's events counts towards `phase`
struct PhaseSpan {
  int first, last, phase;
};
enum class Stored { REPLACE, ADD };

// The N phase times of one call family; a family's thread_local instance is what its ..._times export reads.
template <int N>
struct PhaseTimes {
  float ms[N];
  void clear() {
    for (float& t : ms) t = 0.f;
  }
  // Per phase named in `spans`: the milliseconds of its spans together (a span that cannot be measured counts 0),
  // in place of the stored value or on top of it.  Phases the table does not name keep what they hold.  After the
  // last event has completed.
  void take(Stored how, const EventBox* ev, std::initializer_list<PhaseSpan> spans) {
    float got[N] = {0.f};
    bool named[N] = {false};
    for (const PhaseSpan& sp : spans) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev[sp.first].e, ev[sp.last].e) == hipSuccess) got[sp.phase] += t;
      named[sp.phase] = true;
    }
    for (int i = 0; i < N; ++i)
      if (named[i]) ms[i] = (how == Stored::ADD ? ms[i] : 0.f) + got[i];
  }
  // the body of a ..._times(float* ms, uint32_t cap) export: zeros beyond the phases, nothing at or beyond cap
  g16_status read(float* out, uint32_t cap) const {
    if (!out) return G16_ERR_INVALID;
    for (uint32_t i = 0; i < cap; ++i) out[i] = i < (uint32_t)N ? ms[i] : 0.f;
    return G16_OK;
  }
};

// host clock around a stream synchronisation: lap(phase) adds the time since the last lap
struct PhaseClock {
  float* ms;
  hipStream_t s;
  std::chrono::steady_clock::time_point t0;
  PhaseClock(float* m, hipStream_t st) : ms(m), s(st), t0(std::chrono::steady_clock::now()) {}
  void lap(int phase) {
    G16_HIP(hipStreamSynchronize(s));
    const auto t1 = std::chrono::steady_clock::now();
    ms[phase] += std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// ---- exceptions to statuses ----------------------------------------------------------------------------
// the default sink of guarded_call: the message goes where g16_last_error(NULL) finds it
inline g16_status create_fail(g16_status code, const std::string& msg) {
  set_create_error(msg);
  return code;
}

// Runs the body of an extern "C" entry point (it returns a g16_status, or nothing for G16_OK).  A HipError leaves as
// G16_ERR_HIP, any other exception as G16_ERR_INTERNAL, both through sink(code, what()).  (api.hip's ctx-bound
// guarded(ctx, fn) is another function.)
template <class Body, class Sink = g16_status (*)(g16_status, const std::string&)>
g16_status guarded_call(Body&& body, Sink sink = create_fail) {
  try {
    if constexpr (std::is_void<decltype(body())>::value) {
      body();
      return G16_OK;
    } else {
      return body();
    }
  } catch (const HipError& e) {
    return sink(G16_ERR_HIP, e.what());
  } catch (const std::exception& e) {
    return sink(G16_ERR_INTERNAL, e.what());
  }
}

}  // namespace g16
