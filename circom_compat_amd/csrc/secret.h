// secret.h -- everything that touches a secret scalar on the host, in one place: a fix here reaches every call that
// draws or takes one (g16_key_contribute, g16_srs_contribute, g16_proofs_rerandomize) and the random coefficients of
// the checks.  Plain C++ on top of field.h, no HIP header: tests/host/secret_main.cpp builds it on its own.
//   wipe                 zeroing the compiler may not drop
//   fr_words_canonical   8 x u32 (or 4 x u64) words below r
//   os_random            the operating system's generator; never a fixed fallback
//   FrPool::draw_fr      a uniform element of Fr by rejection, candidates fetched SLOTS at a time
//   draw_rho             nonzero 128-bit coefficients of the small-exponent tests
#pragma once
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>

#include "field.h"

namespace g16 {

inline void wipe(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  while (n--) *v++ = 0;
}

// the stored words are below r
inline bool fr_words_canonical(const Fr& a) {
  for (int i = 7; i >= 0; --i) {
    if (a.v[i] < FrParams::MOD[i]) return true;
    if (a.v[i] > FrParams::MOD[i]) return false;
  }
  return false;  // == r
}
inline bool fr_words_canonical(const uint64_t s[4]) {  // 4 x u64, little-endian: the same 32 bytes
  Fr a;
  memcpy(&a, s, 32);
  return fr_words_canonical(a);
}

// a source of random bytes: false when it delivers none
typedef bool (*RandomSource)(void* buf, size_t len);

// operating-system CSPRNG; false when neither source delivers (never a fixed fallback)
inline bool os_random(void* buf, size_t len) {
  uint8_t* p = (uint8_t*)buf;
  while (len) {
    const ssize_t r = getrandom(p, len, 0);
    if (r < 0) {
      if (errno == EINTR) continue;
      break;
    }
    p += r;
    len -= (size_t)r;
  }
  if (!len) return true;
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f) return false;
  const size_t got = fread(p, 1, len, f);
  fclose(f);
  return got == len;
}

// The candidates draw_fr takes its scalars from: SLOTS per request to the source (one request per scalar would be
// 2 n system calls for the n proofs of a re-randomisation).  A slot is wiped as it is consumed, the pool when it goes.
struct FrPool {
  static constexpr size_t SLOTS = 1024;
  U256 slot[SLOTS];
  U256 cand;  // the candidate under test: wiped with the pool, not per draw (a draw costs what it always did)
  size_t left = 0;
  RandomSource source;
  explicit FrPool(RandomSource src = os_random) : source(src) {}
  FrPool(const FrPool&) = delete;
  FrPool& operator=(const FrPool&) = delete;
  ~FrPool() {
    wipe(slot, sizeof slot);
    wipe(&cand, sizeof cand);
  }

  // uniform in [nonzero ? 1 : 0, r): 254 random bits, rejected outside the range (r > 2^253: < 2 candidates on
  // average).  false: the source gave nothing and *out is untouched (never a fixed fallback).
  bool draw_fr(Fr* out, bool nonzero) {
    for (;;) {
      if (!left) {
        if (!source(slot, sizeof slot)) return false;
        left = SLOTS;
      }
      cand = slot[--left];
      wipe(&slot[left], sizeof(U256));
      cand.v[7] &= 0x3fffffffu;
      Fr w;
      memcpy(&w, &cand, 32);
      const bool in_range = fr_words_canonical(w) && !(nonzero && w.is_zero());
      wipe(&w, sizeof w);
      if (in_range) break;
    }
    *out = Fr::from_canonical(cand);
    return true;
  }
};

// n nonzero 128-bit coefficients, straight into hr; false: the source gave none (never a fixed fallback)
inline bool draw_rho(uint64_t* hr, size_t n, RandomSource source = os_random) {
  bool drawn = source(hr, n * 16);
  for (size_t i = 0; drawn && i < n; ++i)
    while (drawn && !(hr[2 * i] | hr[2 * i + 1])) drawn = source(&hr[2 * i], 16);  // probability 2^-128 per entry
  return drawn;
}

}  // namespace g16
