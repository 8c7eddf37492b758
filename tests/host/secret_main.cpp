// secret_main.cpp -- TEST INFRASTRUCTURE ONLY: csrc/secret.h on its own, with a scripted source of "random" bytes in
// place of the operating system's.  Built by tests/test_secret_host.py with g++ -fsanitize=address,undefined and run
// as a plain program: no GPU, nothing loaded into Python.
//
// FrPool hands out its slots from the last one down, so candidate i of a script lands in slot SLOTS - 1 - i; every
// slot the script does not name holds FILLER, a valid scalar.
#include <stdio.h>

#include <new>
#include <vector>

#include "../../circom_compat_amd/csrc/secret.h"

using namespace g16;

namespace {

int n_checks = 0, n_failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    ++n_checks;                                                        \
    if (!(cond)) {                                                     \
      ++n_failures;                                                    \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);        \
    }                                                                  \
  } while (0)

U256 u256(uint32_t w0 = 0) {
  U256 u{};
  u.v[0] = w0;
  return u;
}
U256 modulus() {
  U256 u{};
  for (int i = 0; i < 8; ++i) u.v[i] = FrParams::MOD[i];
  return u;
}
U256 plus(U256 a, int d) {  // a + d, d = +-1, no carry out in the cases below
  for (int i = 0; i < 8; ++i) {
    const uint32_t was = a.v[i];
    a.v[i] = was + (uint32_t)d;
    if (d > 0 ? a.v[i] != 0 : was != 0) break;
  }
  return a;
}
U256 all_ones(int bits) {
  U256 u{};
  for (int i = 0; i < bits; ++i) u.v[i >> 5] |= 1u << (i & 31);
  return u;
}
bool same(const U256& a, const U256& b) { return memcmp(a.v, b.v, 32) == 0; }
bool canonical(const U256& u) {  // both forms must agree
  Fr a;
  memcpy(&a, &u, 32);
  uint64_t s[4];
  memcpy(s, &u, 32);
  const bool w = fr_words_canonical(a), q = fr_words_canonical(s);
  CHECK(w == q);
  return w;
}

constexpr uint32_t FILLER = 5;

// ---- the scripted source ------------------------------------------------------------------------------
std::vector<U256> script;  // the candidates of the next pool request, in the order they are consumed
int calls = 0;             // requests so far
int fail_at = -1;          // from this request on (counted from 0) the source fails; -1: never
int rho_zero_calls = 0;    // draw_rho: this many requests are answered with zeros

bool scripted(void* buf, size_t len) {
  const int at = calls++;
  if (fail_at >= 0 && at >= fail_at) return false;
  U256* slot = (U256*)buf;
  const size_t n = len / 32;
  for (size_t i = 0; i < n; ++i) slot[i] = u256(FILLER);
  for (size_t i = 0; i < script.size() && i < n; ++i) slot[n - 1 - i] = script[i];
  script.clear();
  return true;
}
bool scripted_rho(void* buf, size_t len) {
  const int at = calls++;
  if (fail_at >= 0 && at >= fail_at) return false;
  memset(buf, calls <= rho_zero_calls ? 0 : 0x11, len);
  return true;
}
void reset(std::vector<U256> next = {}, int fail = -1) {
  script = next;
  calls = 0;
  fail_at = fail;
}

Fr sentinel() {
  Fr f;
  memset(&f, 0xEE, sizeof f);
  return f;
}
bool is_sentinel(const Fr& f) {
  const Fr s = sentinel();
  return memcmp(&f, &s, sizeof f) == 0;
}

}  // namespace

int main() {
  const U256 r = modulus();

  // the canonical predicate
  CHECK(canonical(u256(0)));
  CHECK(canonical(u256(1)));
  CHECK(canonical(plus(r, -1)));
  CHECK(!canonical(r));
  CHECK(!canonical(plus(r, +1)));
  CHECK(!canonical(all_ones(254)));
  CHECK(!canonical(all_ones(256)));

  {  // r, r + 1 and, for a nonzero draw, 0 are rejected; the next candidate is taken
    reset({r, plus(r, +1), u256(0), u256(7), u256(8)});
    FrPool pool(scripted);
    Fr out = sentinel();
    CHECK(pool.draw_fr(&out, true));
    CHECK(same(out.to_canonical(), u256(7)));
    CHECK(pool.left == FrPool::SLOTS - 4);
    CHECK(pool.draw_fr(&out, true) && same(out.to_canonical(), u256(8)));
    CHECK(calls == 1);
  }
  {  // 0 is a value of a draw that may be zero; r - 1 is the largest value
    reset({r, u256(0), plus(r, -1)});
    FrPool pool(scripted);
    Fr out = sentinel();
    CHECK(pool.draw_fr(&out, false));
    CHECK(out.is_zero() && pool.left == FrPool::SLOTS - 2);
    CHECK(pool.draw_fr(&out, false) && same(out.to_canonical(), plus(r, -1)));
  }
  {  // the top two bits are masked before the comparison: 9 with bits 254 and 255 set is 9
    U256 hi = u256(9);
    hi.v[7] |= 0xc0000000u;
    U256 hi255 = u256(10);
    hi255.v[7] |= 0x80000000u;
    reset({hi, hi255});
    FrPool pool(scripted);
    Fr out = sentinel();
    CHECK(pool.draw_fr(&out, true) && same(out.to_canonical(), u256(9)));
    CHECK(pool.draw_fr(&out, true) && same(out.to_canonical(), u256(10)));
    CHECK(pool.left == FrPool::SLOTS - 2);
  }
  {  // a source that fails on the first request: false, *out untouched
    reset({}, 0);
    FrPool pool(scripted);
    Fr out = sentinel();
    CHECK(!pool.draw_fr(&out, true));
    CHECK(is_sentinel(out));
    CHECK(!pool.draw_fr(&out, false) && is_sentinel(out));   // and again: still nothing, never a fixed value
  }
  {  // a source that fails on the refill: every slot of the first request is used, then false, *out untouched
    reset({}, 1);
    FrPool pool(scripted);
    Fr out;
    bool all = true;
    for (size_t i = 0; i < FrPool::SLOTS; ++i) all = all && pool.draw_fr(&out, true) && same(out.to_canonical(), u256(FILLER));
    CHECK(all && pool.left == 0 && calls == 1);
    out = sentinel();
    CHECK(!pool.draw_fr(&out, true));
    CHECK(is_sentinel(out) && calls == 2);
  }
  {  // a rejected tail and then a failing refill: nothing of the rejected candidates comes out
    std::vector<U256> bad(FrPool::SLOTS, r);
    reset(bad, 1);
    FrPool pool(scripted);
    Fr out = sentinel();
    CHECK(!pool.draw_fr(&out, true));
    CHECK(is_sentinel(out) && calls == 2);
  }
  {  // a consumed slot reads as zero, the pool reads as zero once it is gone: looked at through a pointer taken
     // before, into storage this test owns
    alignas(FrPool) static unsigned char store[sizeof(FrPool)];
    memset(store, 0x77, sizeof store);
    reset({u256(3)});
    FrPool* pool = new (store) FrPool(scripted);
    const unsigned char* slots = (const unsigned char*)pool->slot;
    const size_t bytes = sizeof pool->slot, last = (FrPool::SLOTS - 1) * 32;
    Fr out;
    CHECK(pool->draw_fr(&out, true) && same(out.to_canonical(), u256(3)));
    bool zero = true;
    for (size_t i = 0; i < 32; ++i) zero = zero && slots[last + i] == 0;
    CHECK(zero);
    CHECK(slots[last - 32] == FILLER);  // the next one is still there
    pool->~FrPool();
    zero = true;
    for (size_t i = 0; i < bytes; ++i) zero = zero && slots[i] == 0;
    CHECK(zero);
  }
  {  // draw_rho: a source that yields zeros first never leaves a zero coefficient
    uint64_t hr[2 * 6];
    reset();
    rho_zero_calls = 4;  // the request for all six, then three redraws of entry 0
    CHECK(draw_rho(hr, 6, scripted_rho));
    bool nonzero = true;
    for (int i = 0; i < 6; ++i) nonzero = nonzero && (hr[2 * i] | hr[2 * i + 1]);
    CHECK(nonzero);
    CHECK(calls == 4 + 6);   // every entry of the zero block was drawn again, the first one four times
    reset({}, 0);
    CHECK(!draw_rho(hr, 6, scripted_rho));
    reset({}, 2);            // fails on a redraw
    CHECK(!draw_rho(hr, 6, scripted_rho));
  }
  {  // wipe
    unsigned char buf[48];
    memset(buf, 0xFF, sizeof buf);
    wipe(buf + 8, 32);
    bool ok = true;
    for (int i = 0; i < 48; ++i) ok = ok && buf[i] == ((i >= 8 && i < 40) ? 0 : 0xFF);
    CHECK(ok);
  }
  {  // the real source delivers, and a drawn scalar is in range
    FrPool pool;
    Fr out = sentinel();
    CHECK(pool.draw_fr(&out, true));
    CHECK(fr_words_canonical(out) && !out.is_zero());
  }

  printf("%d checks, %d failures\n", n_checks, n_failures);
  return n_failures ? 1 : 0;
}
