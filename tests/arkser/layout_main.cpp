// layout_main.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_ark_layout_host.py): a stand-alone program around the
// layout walk of the arkworks containers (g16_ark_pk_layout / g16_ark_vk_layout, csrc/loaders.cpp), built with
// -fsanitize=address,undefined.  The walk is pure host code over untrusted bytes; every blob handed to it here lives
// in a heap block of EXACTLY its length, so one byte read past the end is a sanitizer report.  No GPU code runs.
//
// Exit status 0: the valid blobs walk to the expected offsets and every truncation and mutation is G16_ERR_IO.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/g16_loaders.h"

namespace {

int failures = 0, cases = 0;

void expect(bool ok, const char* what, long a = 0, long b = 0) {
  ++cases;
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAIL %s (%ld, %ld): %s\n", what, a, b, g16_loader_last_error());
  }
}

// the walk over a copy that ends exactly where the blob ends
g16_status walk(const std::vector<uint8_t>& blob, size_t len, uint32_t flags, bool pk, g16_ark_layout* lay) {
  uint8_t* exact = (uint8_t*)malloc(len ? len : 1);
  memcpy(exact, blob.data(), len);
  const g16_status st = pk ? g16_ark_pk_layout(len ? exact : nullptr, len, flags, lay)
                           : g16_ark_vk_layout(len ? exact : nullptr, len, flags, lay);
  free(exact);
  return st;
}

void put_u64(std::vector<uint8_t>& b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
void put_points(std::vector<uint8_t>& b, uint64_t n, size_t rec) {
  for (uint64_t i = 0; i < n * rec; ++i) b.push_back((uint8_t)(0x11 * (i % 13)));  // never looked at
}

struct Made {
  std::vector<uint8_t> blob;
  std::vector<size_t> boundaries;  // where every piece starts
  std::vector<size_t> prefixes;    // where the length prefixes are
  uint64_t want_off[G16_ARK_N_FIELDS], want_cnt[G16_ARK_N_FIELDS];
};

Made make(uint32_t flags, bool pk, uint64_t n_vars, uint64_t n_ic, uint64_t h_len) {
  Made m;
  const size_t g1 = (flags & G16_ARK_COMPRESSED) ? 32 : 64, g2 = 2 * g1;
  memset(m.want_off, 0, sizeof m.want_off);
  memset(m.want_cnt, 0, sizeof m.want_cnt);
  auto single = [&](int f, size_t rec) {
    m.boundaries.push_back(m.blob.size());
    m.want_off[f] = m.blob.size();
    m.want_cnt[f] = 1;
    put_points(m.blob, 1, rec);
  };
  auto vec = [&](int f, uint64_t n, size_t rec) {
    m.boundaries.push_back(m.blob.size());
    m.prefixes.push_back(m.blob.size());
    put_u64(m.blob, n);
    m.boundaries.push_back(m.blob.size());
    m.want_off[f] = m.blob.size();
    m.want_cnt[f] = n;
    put_points(m.blob, n, rec);
  };
  single(G16_ARK_F_ALPHA_G1, g1);
  single(G16_ARK_F_BETA_G2, g2);
  single(G16_ARK_F_GAMMA_G2, g2);
  single(G16_ARK_F_DELTA_G2, g2);
  vec(G16_ARK_F_IC, n_ic, g1);
  if (pk) {
    single(G16_ARK_F_BETA_G1, g1);
    single(G16_ARK_F_DELTA_G1, g1);
    vec(G16_ARK_F_A, n_vars, g1);
    vec(G16_ARK_F_B1, n_vars, g1);
    vec(G16_ARK_F_B2, n_vars, g2);
    vec(G16_ARK_F_H, h_len, g1);
    vec(G16_ARK_F_L, n_vars - n_ic, g1);
  }
  return m;
}

void run(uint32_t flags, bool pk) {
  const Made m = make(flags, pk, 9, 2, 7);
  g16_ark_layout lay;
  expect(walk(m.blob, m.blob.size(), flags, pk, &lay) == G16_OK, "valid blob", flags, pk);
  expect(lay.total == m.blob.size(), "total", flags, pk);
  for (int f = 0; f < G16_ARK_N_FIELDS; ++f)
    expect(lay.offset[f] == m.want_off[f] && lay.count[f] == m.want_cnt[f], "offset / count", flags, f);
  // the other record size: the same bytes cannot be a blob of the other mode
  expect(walk(m.blob, m.blob.size(), flags ^ G16_ARK_COMPRESSED, pk, &lay) == G16_ERR_IO, "other mode", flags, pk);
  // truncations: at every boundary, one byte before and after it, and in the middle of what follows
  for (size_t b : m.boundaries)
    for (long d : {-1L, 0L, 1L, 5L, 19L}) {
      const long len = (long)b + d;
      if (len < 0 || (size_t)len >= m.blob.size()) continue;
      expect(walk(m.blob, (size_t)len, flags, pk, &lay) == G16_ERR_IO, "truncation", (long)b, d);
      expect(lay.total == 0, "a failed walk leaves a zero layout", (long)b, d);
    }
  expect(walk(m.blob, 0, flags, pk, &lay) == G16_ERR_IO, "empty blob");
  // trailing bytes
  for (size_t extra : {1u, 8u, 64u}) {
    std::vector<uint8_t> t = m.blob;
    t.resize(t.size() + extra, 0);
    expect(walk(t, t.size(), flags, pk, &lay) == G16_ERR_IO, "trailing bytes", (long)extra);
  }
  // mutations of every length prefix: one off, huge, overflowing when multiplied by the record size
  const uint64_t lens[] = {0, 1, 3, 1ull << 31, 1ull << 32, (1ull << 58) + 1, 1ull << 59, 1ull << 63,
                           ~0ull, ~0ull / 32, ~0ull / 64 + 1, ~0ull - 7};
  for (size_t at : m.prefixes) {
    uint64_t was;
    memcpy(&was, m.blob.data() + at, 8);
    for (uint64_t v : lens)
      for (uint64_t vv : {v, was + 1, was - 1}) {
        if (vv == was) continue;
        std::vector<uint8_t> t = m.blob;
        memcpy(t.data() + at, &vv, 8);
        expect(walk(t, t.size(), flags, pk, &lay) == G16_ERR_IO, "mutated length", (long)at, (long)vv);
      }
  }
  if (pk) {  // array lengths that disagree with each other inside blobs that are otherwise well formed
    Made a = make(flags, true, 9, 2, 7);
    const size_t g1 = (flags & G16_ARK_COMPRESSED) ? 32 : 64;
    // one more point of l_query: the walk ends at the end of the blob, the counts do not match
    const uint64_t more = a.want_cnt[G16_ARK_F_L] + 1;
    memcpy(a.blob.data() + a.prefixes.back(), &more, 8);
    a.blob.resize(a.blob.size() + g1, 0x22);
    expect(walk(a.blob, a.blob.size(), flags, true, &lay) == G16_ERR_IO, "len(l_query)");
    // an empty gamma_abc_g1
    Made e = make(flags, true, 9, 0, 7);
    expect(walk(e.blob, e.blob.size(), flags, true, &lay) == G16_ERR_IO, "len(gamma_abc_g1) = 0");
    // h_query may have any length
    Made h = make(flags, true, 9, 2, 0);
    expect(walk(h.blob, h.blob.size(), flags, true, &lay) == G16_OK && lay.count[G16_ARK_F_H] == 0, "len(h_query) = 0");
  }
  expect(g16_ark_pk_layout(m.blob.data(), m.blob.size(), flags, nullptr) == G16_ERR_INVALID, "NULL out");
}

}  // namespace

int main() {
  for (uint32_t flags : {0u, (uint32_t)G16_ARK_COMPRESSED, (uint32_t)(G16_ARK_COMPRESSED | G16_ARK_VALIDATE)})
    for (bool pk : {true, false}) run(flags, pk);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
