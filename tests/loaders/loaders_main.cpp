// loaders_main.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_loaders_host.py): a stand-alone program around the four
// file parsers of csrc/loaders.cpp (.zkey, .r1cs, .wtns, .ptau) and the .zkey writer.  Pure host code over untrusted
// bytes; no GPU code runs and nothing is loaded into Python.  It is built twice:
//
//   * with -fsanitize=address,undefined: every blob handed to a *_mem entry point lives in a heap block of EXACTLY
//     its length and is freed right after the call, and after every successful open every byte that every handed-out
//     view promises is read -- a view or a parse that overruns is a sanitizer report;
//   * plain, with -DLOADERS_ALLOC_BOUND: the global operator new refuses (std::bad_alloc) a single request above
//     4 x (length of the file under test) + 64 KiB.  A count taken from a header and reserved for unchecked is then
//     an exception inside the loader -- which must come back as a status, never as an abort -- on a machine of any
//     size.  The factor 4 is a condition on the parsers, not a measurement: the largest legitimate request is the
//     vector of 32-byte values of an r1cs, under 2 x the file with doubling growth, and the copy of a zkey is 1 x.
//
// The files are written here from the format descriptions of SURVEY.md Appendix A; the loaders never look at point
// bytes, so those are arbitrary (and distinct per section, so that a view of the wrong section is seen).
//
// A truncation is always G16_ERR_IO.  Any other mutated file is either refused with G16_ERR_IO, or accepted with all
// its views reading clean and its invariants holding (examine_*).  Prints "N cases, F failures"; exit status 1 on any
// failure.  Before each group of cases its name is printed, and an abort prints the case it died in.
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/g16_loaders.h"

// ---- the allocation bound ---------------------------------------------------------------------------------------
static size_t g_alloc_limit = SIZE_MAX;
#ifdef LOADERS_ALLOC_BOUND
void* operator new(size_t n) {
  if (n > g_alloc_limit) throw std::bad_alloc();
  void* p = malloc(n ? n : 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void operator delete(void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
#endif

namespace {

typedef std::vector<uint8_t> Bytes;

int failures = 0, cases = 0;
char g_case[256] = "(start)";

void on_abort(int) {
  const char head[] = "\nABORTED in case: ";
  (void)!write(2, head, sizeof head - 1);
  (void)!write(2, g_case, strlen(g_case));
  (void)!write(2, "\n", 1);
  _exit(134);
}

void name_case(const char* group, const char* what, long long a = 0, long long b = 0) {
  snprintf(g_case, sizeof g_case, "%s: %s (%lld, %lld)", group, what, a, b);
}
void group(const char* g) {
  printf("# %s\n", g);
  fflush(stdout);
}

void expect(bool ok, const char* why = "") {
  ++cases;
  if (!ok) {
    ++failures;
    if (failures <= 200) fprintf(stderr, "FAIL %s %s: %s\n", g_case, why, g16_loader_last_error());
  }
}

// the file under test bounds what one request may ask for (plain build); no bound outside a case
struct Bound {
  explicit Bound(size_t file_len) { g_alloc_limit = 4 * file_len + (64u << 10); }
  ~Bound() { g_alloc_limit = SIZE_MAX; }
};

// f(data, len) over a heap block of exactly len bytes, freed right after the call
g16_status exact(const Bytes& b, size_t len, const std::function<g16_status(const uint8_t*, size_t)>& f) {
  uint8_t* e = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(e, b.data(), len);
  const g16_status st = f(e, len);
  free(e);
  return st;
}

// reads every byte of a view; the sum keeps the loop alive
volatile uint64_t g_sink;
void touch(const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  uint64_t s = 0;
  for (size_t i = 0; i < n; ++i) s += b[i];
  g_sink = g_sink + s;
}

// ---- bytes --------------------------------------------------------------------------------------------------------
void put32(Bytes& b, uint32_t v) {
  for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
void put64(Bytes& b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
void put(Bytes& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
void poke32(Bytes& b, size_t at, uint32_t v) { memcpy(b.data() + at, &v, 4); }
void poke64(Bytes& b, size_t at, uint64_t v) { memcpy(b.data() + at, &v, 8); }
uint32_t peek32(const Bytes& b, size_t at) {
  uint32_t v;
  memcpy(&v, b.data() + at, 4);
  return v;
}
uint64_t peek64(const Bytes& b, size_t at) {
  uint64_t v;
  memcpy(&v, b.data() + at, 8);
  return v;
}
// n arbitrary bytes that depend on the section they stand in
Bytes filler(uint32_t tag, size_t n) {
  Bytes b(n);
  for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)(tag * 37 + i * 11 + (i >> 8) * 5 + 1);
  return b;
}

struct V32 {
  uint8_t b[32];
  bool operator==(const V32& o) const { return memcmp(b, o.b, 32) == 0; }
};
// little-endian bytes of a 64-digit big-endian hex number
V32 from_hex(const char* hex) {
  V32 v;
  for (int i = 0; i < 32; ++i) {
    unsigned x = 0;
    sscanf(hex + 2 * (31 - i), "%2x", &x);
    v.b[i] = (uint8_t)x;
  }
  return v;
}
V32 small(uint64_t x) {
  V32 v;
  memset(v.b, 0, 32);
  memcpy(v.b, &x, 8);
  return v;
}
// SURVEY.md Appendix B
const V32 kR = from_hex("30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001");
const V32 kQ = from_hex("30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47");
const V32 kMontOne = from_hex("0e0a77c19a07df2f666ea36f7879462e36fc76959f60cd29ac96341c4ffffffb");  // 2^256 mod r
V32 r_plus(int d) {  // r - 1, r, r + 1: the low byte of r is 0x01
  V32 v = kR;
  v.b[0] = (uint8_t)(v.b[0] + d);
  return v;
}
V32 all_ones() {
  V32 v;
  memset(v.b, 0xff, 32);
  return v;
}
// Montgomery limbs of a canonical value, by the library's own helper (pinned to 2^256 mod r in main)
V32 mont(const V32& canonical) {
  V32 out;
  uint64_t limbs[4];
  if (g16_fr_from_canonical(canonical.b, limbs, 1) != G16_OK) memset(limbs, 0xee, sizeof limbs);
  memcpy(out.b, limbs, 32);
  return out;
}

// ---- the container: magic, version, nSections, then (id u32, size u64, payload)* ------------------------------
struct Sec {
  uint32_t id;
  Bytes body;
};
struct File {
  const char* magic;
  uint32_t version;
  std::vector<Sec> secs;
};
struct Made {
  Bytes blob;
  std::vector<size_t> entry;  // where the (id, size) of section i stands; its body starts 12 bytes on
};
Made assemble(const File& f) {
  Made m;
  put(m.blob, f.magic, 4);
  put32(m.blob, f.version);
  put32(m.blob, (uint32_t)f.secs.size());
  for (const Sec& s : f.secs) {
    m.entry.push_back(m.blob.size());
    put32(m.blob, s.id);
    put64(m.blob, s.body.size());
    put(m.blob, s.body.data(), s.body.size());
  }
  return m;
}
size_t body_of(const File& f, const Made& m, uint32_t id) {  // first occurrence
  for (size_t i = 0; i < f.secs.size(); ++i)
    if (f.secs[i].id == id) return m.entry[i] + 12;
  abort();
}
const Bytes& sec_of(const File& f, uint32_t id) {
  for (const Sec& s : f.secs)
    if (s.id == id) return s.body;
  abort();
}

struct Field {  // a count field of a header: where it stands in the section's body
  const char* name;
  uint32_t sec;
  size_t off;
  bool wide;  // u64
};

// ---- what a parse must give back --------------------------------------------------------------------------------
struct Csr {
  std::vector<uint32_t> rowptr, col;
  std::vector<V32> val;  // Montgomery limbs
};
bool csr_equal(const g16_csr& c, const Csr& w) {
  if (c.nnz != w.col.size()) return false;
  if (memcmp(c.row_ptr, w.rowptr.data(), w.rowptr.size() * 4) != 0) return false;
  if (c.nnz && memcmp(c.col, w.col.data(), c.nnz * 4) != 0) return false;
  for (size_t i = 0; i < w.val.size(); ++i)
    if (memcmp(c.coeff + 4 * i, w.val[i].b, 32) != 0) return false;
  return true;
}
// reads all three arrays of a CSR with `rows` rows; row_ptr spans [0, nnz] monotonically, col < col_bound
bool csr_sound(const g16_csr& c, uint64_t rows, uint64_t col_bound) {
  if (!c.row_ptr) return false;
  touch(c.row_ptr, (rows + 1) * 4);
  touch(c.col, c.nnz * 4);
  touch(c.coeff, c.nnz * 32);
  if (c.row_ptr[0] != 0 || c.row_ptr[rows] != c.nnz) return false;
  for (uint64_t i = 0; i < rows; ++i)
    if (c.row_ptr[i] > c.row_ptr[i + 1]) return false;
  for (uint64_t j = 0; j < c.nnz; ++j)
    if (c.col[j] >= col_bound) return false;
  return true;
}

// =================================================================================================== zkey ========
struct ZkeyWant {
  uint32_t n_vars = 5, n_public = 1, domain = 4, nc = 2;
  Csr a, b;
};
File zkey_file(ZkeyWant* want) {
  File f{"zkey", 1, {}};
  Bytes one;
  put32(one, 1);
  f.secs.push_back({1, one});
  Bytes h;
  put32(h, 32);
  put(h, kQ.b, 32);
  put32(h, 32);
  put(h, kR.b, 32);
  put32(h, 5);  // n_vars       at 72
  put32(h, 1);  // n_public     at 76
  put32(h, 4);  // domain_size  at 80
  const Bytes pts = filler(2, 64 + 64 + 128 + 128 + 64 + 128);
  put(h, pts.data(), pts.size());
  f.secs.push_back({2, h});
  f.secs.push_back({3, filler(3, 2 * 64)});
  // Coefs: two constraints plus the n_public + 1 rows snarkjs appends; B records between the A records, and the
  // rows of a matrix out of order, so that the counting sort of the loader has something to do
  struct Rec {
    uint32_t m, row, sig;
    uint64_t v;
  };
  const Rec recs[] = {{0, 1, 4, 9},  {1, 0, 3, 11}, {0, 0, 2, 5}, {1, 1, 1, 13},
                      {0, 2, 0, 1},  {0, 0, 3, 7},  {1, 1, 2, 17}, {0, 3, 1, 1}};
  Bytes c;
  put32(c, 8);
  for (const Rec& r : recs) {
    put32(c, r.m);
    put32(c, r.row);
    put32(c, r.sig);
    const V32 stored = mont(mont(small(r.v)));  // v R^2 mod r: the loader takes one R off
    put(c, stored.b, 32);
  }
  f.secs.push_back({4, c});
  f.secs.push_back({5, filler(5, 5 * 64)});
  f.secs.push_back({6, filler(6, 5 * 64)});
  f.secs.push_back({7, filler(7, 5 * 128)});
  f.secs.push_back({8, filler(8, 3 * 64)});
  f.secs.push_back({9, filler(9, 4 * 64)});
  f.secs.push_back({10, filler(10, 68)});
  if (want) {  // rows >= nc = max row - n_public = 2 are dropped; file order inside a row
    want->a.rowptr = {0, 2, 3};
    want->a.col = {2, 3, 4};
    want->a.val = {mont(small(5)), mont(small(7)), mont(small(9))};
    want->b.rowptr = {0, 1, 3};
    want->b.col = {3, 1, 2};
    want->b.val = {mont(small(11)), mont(small(13)), mont(small(17))};
  }
  return f;
}
std::vector<Field> zkey_fields() {
  std::vector<Field> v = {{"n8q", 2, 0, false},     {"n8r", 2, 36, false},         {"n_vars", 2, 72, false},
                          {"n_public", 2, 76, false}, {"domain_size", 2, 80, false}, {"coefs count", 4, 0, false}};
  for (size_t i = 0; i < 8; ++i) {
    v.push_back({"coef matrix", 4, 4 + 44 * i, false});
    v.push_back({"coef row", 4, 4 + 44 * i + 4, false});
    v.push_back({"coef signal", 4, 4 + 44 * i + 8, false});
  }
  return v;
}

// every view of an open zkey read to its promised end; the invariants; against `f` / `want` when given
bool examine_zkey(g16_zkey* z, const File* f, const ZkeyWant* want, const char** why) {
  g16_zkey_header h;
  g16_key_desc k;
  *why = "header / key";
  if (g16_zkey_header_get(z, &h) != G16_OK || g16_zkey_key(z, &k) != G16_OK) return false;
  *why = "header counts";
  if (k.n_vars != h.n_vars || k.n_public != h.n_public || k.domain_size != h.domain_size) return false;
  if ((uint64_t)h.n_public + 1 > h.n_vars || (uint64_t)h.n_public + 1 > h.domain_size) return false;
  const size_t N = k.n_vars, nl = (size_t)k.n_vars - k.n_public - 1;
  touch(k.a_query, N * 64);
  touch(k.b_g1_query, N * 64);
  touch(k.b_g2_query, N * 128);
  touch(k.l_query, nl * 64);
  touch(k.h_query, (size_t)k.domain_size * 64);
  uint32_t n_ic = 0;
  const uint8_t* ic = g16_zkey_ic(z, &n_ic);
  *why = "ic";
  if (!ic || n_ic != h.n_public + 1) return false;
  touch(ic, (size_t)n_ic * 64);
  if (f) {
    *why = "a view is not its section";
    if (memcmp(k.a_query, sec_of(*f, 5).data(), N * 64) || memcmp(k.b_g1_query, sec_of(*f, 6).data(), N * 64) ||
        memcmp(k.b_g2_query, sec_of(*f, 7).data(), N * 128) || memcmp(k.l_query, sec_of(*f, 8).data(), nl * 64) ||
        memcmp(k.h_query, sec_of(*f, 9).data(), (size_t)k.domain_size * 64) ||
        memcmp(ic, sec_of(*f, 3).data(), (size_t)n_ic * 64))
      return false;
    const uint8_t* p = sec_of(*f, 2).data() + 84;
    *why = "header points";
    if (memcmp(h.alpha_g1, p, 64) || memcmp(h.beta_g1, p + 64, 64) || memcmp(h.beta_g2, p + 128, 128) ||
        memcmp(h.gamma_g2, p + 256, 128) || memcmp(h.delta_g1, p + 384, 64) || memcmp(h.delta_g2, p + 448, 128) ||
        memcmp(k.alpha_g1, p, 64) || memcmp(k.delta_g2, p + 448, 128))
      return false;
  }
  g16_matrices m;
  const g16_status st = g16_zkey_matrices(z, &m);
  *why = "matrices status";
  if (st == G16_ERR_IO && !want) return true;  // a coefficient section that is refused is a refusal
  if (st != G16_OK) return false;
  *why = "matrices";
  if (m.num_constraints > h.domain_size || m.num_instance_variables != h.n_public + 1 ||
      m.num_witness_variables != h.n_vars - h.n_public || m.a_num_non_zero != m.a.nnz || m.b_num_non_zero != m.b.nnz)
    return false;
  if (!csr_sound(m.a, m.num_constraints, h.n_vars) || !csr_sound(m.b, m.num_constraints, h.n_vars)) return false;
  if (want) {
    *why = "values";
    if (h.n8q != 32 || h.n8r != 32 || memcmp(h.q, kQ.b, 32) || memcmp(h.r, kR.b, 32) || h.n_vars != want->n_vars ||
        h.n_public != want->n_public || h.domain_size != want->domain || h.power != 2 ||
        m.num_constraints != want->nc || !csr_equal(m.a, want->a) || !csr_equal(m.b, want->b))
      return false;
  }
  *why = "";
  return true;
}

// =================================================================================================== r1cs ========
struct R1csWant {
  uint32_t n_wires = 5, n_pub_out = 1, n_pub_in = 1, n_prv_in = 2, n_constraints = 3;
  uint64_t n_labels = 5;
  Csr m[3];
  std::vector<uint64_t> labels;
};
struct Term {
  uint32_t wire;
  V32 canonical;
};
typedef std::vector<Term> Lc;
Bytes r1cs_constraints(const std::vector<std::vector<Lc>>& cons, std::vector<Field>* fields) {
  Bytes b;
  for (const auto& con : cons)
    for (const Lc& lc : con) {
      if (fields) fields->push_back({"term count", 2, b.size(), false});
      put32(b, (uint32_t)lc.size());
      for (const Term& t : lc) {
        if (fields) fields->push_back({"wire index", 2, b.size(), false});
        put32(b, t.wire);
        put(b, t.canonical.b, 32);
      }
    }
  return b;
}
std::vector<std::vector<Lc>> r1cs_rows() {  // one-term, multi-term and empty rows in each matrix
  return {{{{1, small(3)}, {2, r_plus(-1)}}, {{3, small(1)}}, {{4, small(8)}}},
          {{}, {{0, small(0)}, {4, small(12)}}, {{1, small(21)}}},
          {{{2, small(6)}}, {{2, small(6)}}, {}}};
}
void r1cs_want_rows(const std::vector<std::vector<Lc>>& cons, R1csWant* w) {
  for (int q = 0; q < 3; ++q) {
    w->m[q] = Csr();
    w->m[q].rowptr.push_back(0);
    for (const auto& con : cons) {
      for (const Term& t : con[q]) {
        w->m[q].col.push_back(t.wire);
        w->m[q].val.push_back(mont(t.canonical));
      }
      w->m[q].rowptr.push_back((uint32_t)w->m[q].col.size());
    }
  }
}
File r1cs_file(R1csWant* want, std::vector<Field>* fields) {
  File f{"r1cs", 1, {}};
  const auto cons = r1cs_rows();
  if (fields)
    *fields = {{"field_size", 1, 0, false}, {"n_wires", 1, 36, false},  {"n_pub_out", 1, 40, false},
               {"n_pub_in", 1, 44, false},  {"n_prv_in", 1, 48, false}, {"n_labels", 1, 52, true},
               {"n_constraints", 1, 60, false}};
  f.secs.push_back({2, r1cs_constraints(cons, fields)});  // constraints first, as circom writes them
  Bytes h;
  put32(h, 32);
  put(h, kR.b, 32);
  put32(h, 5);
  put32(h, 1);
  put32(h, 1);
  put32(h, 2);
  put64(h, 5);
  put32(h, 3);
  f.secs.push_back({1, h});
  const std::vector<uint64_t> labels = {0, 3, 5, 7, 9};
  Bytes map;
  for (uint64_t l : labels) put64(map, l);
  f.secs.push_back({3, map});
  if (want) {
    r1cs_want_rows(cons, want);
    want->labels = labels;
  }
  return f;
}

bool examine_r1cs(g16_r1cs* r, const R1csWant* want, const char** why) {
  g16_r1cs_header h;
  *why = "header";
  if (g16_r1cs_header_get(r, &h) != G16_OK) return false;
  *why = "header counts";
  const uint64_t ni = (uint64_t)1 + h.n_pub_in + h.n_pub_out;
  if (h.num_inputs != ni || ni > h.n_wires || h.num_variables != h.n_wires || h.num_aux != h.n_wires - h.num_inputs ||
      h.field_size != 32 || h.version != 1)
    return false;
  g16_csr m[3];
  *why = "matrices";
  if (g16_r1cs_matrices(r, &m[0], &m[1], &m[2]) != G16_OK) return false;
  // a wire index is NOT compared with n_wires by this loader (nor by the reference's): g16_ctx_create and the setup
  // entry points refuse it.  Pinned, not endorsed: see main().
  for (int q = 0; q < 3; ++q)
    if (!csr_sound(m[q], h.n_constraints, (uint64_t)1 << 32)) return false;
  uint32_t nmap = 0;
  const uint64_t* map = g16_r1cs_wire_mapping(r, &nmap);
  *why = "wire mapping";
  if (nmap != h.n_wires || !map) return false;
  touch(map, (size_t)nmap * 8);
  if (map[0] != 0) return false;
  if (want) {
    *why = "values";
    if (h.n_wires != want->n_wires || h.n_pub_out != want->n_pub_out || h.n_pub_in != want->n_pub_in ||
        h.n_prv_in != want->n_prv_in || h.n_labels != want->n_labels || h.n_constraints != want->n_constraints ||
        memcmp(h.prime, kR.b, 32) || h.num_inputs != 3 || h.num_aux != 2)
      return false;
    for (int q = 0; q < 3; ++q)
      if (!csr_equal(m[q], want->m[q])) return false;
    if (memcmp(map, want->labels.data(), want->labels.size() * 8)) return false;
  }
  *why = "";
  return true;
}

// =================================================================================================== wtns ========
const uint64_t kWtnsValues[4] = {1, 33, 3, 11};
File wtns_file(const std::vector<V32>& values) {
  File f{"wtns", 2, {}};
  Bytes h;
  put32(h, 32);
  put(h, kR.b, 32);
  put32(h, (uint32_t)values.size());
  f.secs.push_back({1, h});
  Bytes v;
  for (const V32& x : values) put(v, x.b, 32);
  f.secs.push_back({2, v});
  return f;
}
std::vector<V32> wtns_values() {
  std::vector<V32> v;
  for (uint64_t x : kWtnsValues) v.push_back(small(x));
  return v;
}
// section 2 as the parser chose it: the LAST one, and its size
bool wtns_section2(const Bytes& blob, size_t* pos, uint64_t* size) {
  bool found = false;
  const uint32_t nsec = peek32(blob, 8);
  size_t o = 12;
  for (uint32_t i = 0; i < nsec && o + 12 <= blob.size(); ++i) {
    const uint32_t id = peek32(blob, o);
    const uint64_t sz = peek64(blob, o + 4);
    if (id == 2) {
      found = true;
      *pos = o + 12;
      *size = sz;
    }
    if (sz > blob.size() - o - 12) break;
    o += 12 + (size_t)sz;
  }
  return found;
}

// =================================================================================================== ptau ========
File ptau_file(bool prepared) {
  File f{"ptau", 1, {}};
  Bytes h;
  put32(h, 32);
  put(h, kQ.b, 32);
  put32(h, 2);  // power            at 36
  put32(h, 2);  // ceremony_power   at 40
  f.secs.push_back({1, h});
  f.secs.push_back({2, filler(2, 7 * 64)});
  f.secs.push_back({3, filler(3, 4 * 128)});
  f.secs.push_back({4, filler(4, 4 * 64)});
  f.secs.push_back({5, filler(5, 4 * 64)});
  f.secs.push_back({6, filler(6, 128)});
  Bytes c;
  put32(c, 0);
  f.secs.push_back({7, c});
  if (prepared) {
    f.secs.push_back({12, filler(12, 15 * 64)});
    f.secs.push_back({13, filler(13, 7 * 128)});
    f.secs.push_back({14, filler(14, 7 * 64)});
    f.secs.push_back({15, filler(15, 7 * 64)});
  }
  return f;
}
bool examine_ptau(g16_ptau* p, const File* f, bool must_be_prepared, const char** why) {
  g16_ptau_header h;
  g16_srs_desc s;
  *why = "header / srs";
  if (g16_ptau_header_get(p, &h) != G16_OK || g16_ptau_srs(p, &s) != G16_OK) return false;
  *why = "counts";
  if (h.n8q != 32 || memcmp(h.q, kQ.b, 32) || h.power > 28) return false;
  const uint64_t n = (uint64_t)1 << h.power;
  if (s.n_tau != n || s.n_tau_g1 != 2 * n - 1) return false;
  touch(s.tau_g1, (2 * n - 1) * 64);
  touch(s.tau_g2, n * 128);
  touch(s.alpha_tau_g1, n * 64);
  touch(s.beta_tau_g1, n * 64);
  if (f) {
    *why = "a view is not its section";
    if (h.power != 2 || h.ceremony_power != 2 || memcmp(s.tau_g1, sec_of(*f, 2).data(), 7 * 64) ||
        memcmp(s.tau_g2, sec_of(*f, 3).data(), 4 * 128) || memcmp(s.alpha_tau_g1, sec_of(*f, 4).data(), 4 * 64) ||
        memcmp(s.beta_tau_g1, sec_of(*f, 5).data(), 4 * 64) || memcmp(s.beta_g2, sec_of(*f, 6).data(), 128))
      return false;
  }
  g16_srs_lagrange_desc l;
  const g16_status st = g16_ptau_lagrange(p, &l);
  *why = "lagrange status";
  if (st == G16_ERR_IO) {
    if (l.tau_g1 || l.tau_g2 || l.alpha_tau_g1 || l.beta_tau_g1) return false;
    *why = "";
    return !must_be_prepared;
  }
  if (st != G16_OK || l.power != h.power) return false;
  touch(l.tau_g1, (4 * n - 1) * 64);
  touch(l.tau_g2, (2 * n - 1) * 128);
  touch(l.alpha_tau_g1, (2 * n - 1) * 64);
  touch(l.beta_tau_g1, (2 * n - 1) * 64);
  if (f && must_be_prepared) {
    *why = "a Lagrange view is not its section";
    if (memcmp(l.tau_g1, sec_of(*f, 12).data(), 15 * 64) || memcmp(l.tau_g2, sec_of(*f, 13).data(), 7 * 128) ||
        memcmp(l.alpha_tau_g1, sec_of(*f, 14).data(), 7 * 64) || memcmp(l.beta_tau_g1, sec_of(*f, 15).data(), 7 * 64))
      return false;
  }
  *why = "";
  return true;
}

// =============================================================================== one parse of one blob ===========
enum Kind { ZKEY, R1CS, WTNS, PTAU, PTAU_PREPARED, N_KINDS };
const char* const kKind[N_KINDS] = {"zkey", "r1cs", "wtns", "ptau", "prepared ptau"};

struct Outcome {
  g16_status st;
  bool sound;       // accepted: every view read clean, the invariants hold (and the values, where asked for)
  const char* why;
};

struct Wants {
  const File* file = nullptr;  // the sections the views must equal
  const ZkeyWant* zkey = nullptr;
  const R1csWant* r1cs = nullptr;
  const std::vector<V32>* wtns = nullptr;  // canonical values
  bool prepared = false;
};

// the wtns entry points: the view (no range test, g16_loaders.h) and the converting read
Outcome parse_wtns(const Bytes& blob, size_t len, const Wants& w) {
  Outcome o{G16_OK, false, ""};
  g16_wtns* h = nullptr;
  o.st = exact(blob, len, [&](const uint8_t* d, size_t n) { return g16_wtns_open_mem(d, n, &h); });
  uint64_t* vals = (uint64_t*)(uintptr_t)1;
  uint32_t cnt = 0;
  const g16_status st2 = exact(blob, len, [&](const uint8_t* d, size_t n) { return g16_wtns_read_mem(d, n, &vals, &cnt); });
  if (o.st != G16_OK) {
    o.why = "the view is refused but the read is not";
    o.sound = h == nullptr && st2 != G16_OK;
    if (st2 == G16_OK) g16_free(vals);
    return o;
  }
  const uint32_t n = g16_wtns_count(h);
  const uint8_t* v = g16_wtns_values(h);
  touch(v, (size_t)n * 32);
  size_t pos = 0;
  uint64_t size = 0;
  const Bytes whole(blob.begin(), blob.begin() + len);
  o.why = "count / section size";
  o.sound = v && wtns_section2(whole, &pos, &size) && (uint64_t)n * 32 <= size && memcmp(v, whole.data() + pos, (size_t)n * 32) == 0;
  bool canonical = true;
  for (uint32_t i = 0; i < n && o.sound; ++i) {
    V32 x;
    memcpy(x.b, v + (size_t)i * 32, 32);
    uint64_t limbs[4];
    canonical = canonical && g16_fr_from_canonical(x.b, limbs, 1) == G16_OK;
  }
  if (o.sound) {
    // the read accepts exactly the files whose values are all canonical, and converts each
    o.why = "the converting read disagrees with the view";
    if (st2 == G16_OK) {
      touch(vals, (size_t)cnt * 32);
      o.sound = canonical && cnt == n;
      for (uint32_t i = 0; i < n && o.sound; ++i) {
        V32 x, m;
        memcpy(x.b, v + (size_t)i * 32, 32);
        memcpy(m.b, vals + (size_t)i * 4, 32);
        o.sound = mont(x) == m;
      }
    } else {
      o.sound = !canonical && st2 == G16_ERR_IO;
    }
  }
  if (o.sound && w.wtns) {
    o.why = "values";
    o.sound = n == w.wtns->size() && memcmp(v, w.wtns->data(), (size_t)n * 32) == 0;
  }
  if (st2 == G16_OK) g16_free(vals);
  g16_wtns_close(h);
  if (o.sound) o.why = "";
  return o;
}

Outcome parse(Kind k, const Bytes& blob, size_t len, const Wants& w = Wants()) {
  const Bound bound(len);
  if (k == WTNS) return parse_wtns(blob, len, w);
  Outcome o{G16_OK, false, ""};
  if (k == ZKEY) {
    g16_zkey* z = (g16_zkey*)(uintptr_t)1;
    o.st = exact(blob, len, [&](const uint8_t* d, size_t n) { return g16_zkey_open_mem(d, n, &z); });
    if (o.st != G16_OK) {
      o.sound = z == nullptr;
      o.why = "*out is not NULL after a refusal";
      return o;
    }
    o.sound = examine_zkey(z, w.file, w.zkey, &o.why);
    g16_zkey_close(z);
  } else if (k == R1CS) {
    g16_r1cs* r = (g16_r1cs*)(uintptr_t)1;
    o.st = exact(blob, len, [&](const uint8_t* d, size_t n) { return g16_r1cs_open_mem(d, n, &r); });
    if (o.st != G16_OK) {
      o.sound = r == nullptr;
      o.why = "*out is not NULL after a refusal";
      return o;
    }
    o.sound = examine_r1cs(r, w.r1cs, &o.why);
    g16_r1cs_close(r);
  } else {
    g16_ptau* p = (g16_ptau*)(uintptr_t)1;
    o.st = exact(blob, len, [&](const uint8_t* d, size_t n) { return g16_ptau_open_mem(d, n, &p); });
    if (o.st != G16_OK) {
      o.sound = p == nullptr;
      o.why = "*out is not NULL after a refusal";
      return o;
    }
    o.sound = examine_ptau(p, w.file, w.prepared, &o.why);
    g16_ptau_close(p);
  }
  return o;
}

void expect_valid(Kind k, const Bytes& blob, const Wants& w) {
  const Outcome o = parse(k, blob, blob.size(), w);
  expect(o.st == G16_OK && o.sound, o.st == G16_OK ? o.why : "refused");
}
void expect_refused(Kind k, const Bytes& blob, size_t len) {
  const Outcome o = parse(k, blob, len);
  expect(o.st == G16_ERR_IO && o.sound, o.st == G16_ERR_IO ? o.why : "not G16_ERR_IO");
}
// refused with G16_ERR_IO, or accepted and sound; the status is handed back for cases that pin it
g16_status expect_refused_or_sound(Kind k, const Bytes& blob) {
  const Outcome o = parse(k, blob, blob.size());
  expect((o.st == G16_ERR_IO || o.st == G16_OK) && o.sound, o.st == G16_OK || o.st == G16_ERR_IO ? o.why : "status");
  return o.st;
}

// ---- the file-path entry points over temporary files ----------------------------------------------------------
std::string g_tmpdir;
std::string tmp_path(const char* name) { return g_tmpdir + "/" + name; }
bool write_file(const std::string& path, const Bytes& b, size_t len) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = len == 0 || fwrite(b.data(), 1, len, f) == len;
  return fclose(f) == 0 && ok;
}
// G16_OK and sound for the whole file, G16_ERR_IO for a truncation
void path_case(Kind k, const Bytes& blob, size_t len, const Wants& w) {
  const std::string path = tmp_path("file.bin");
  const bool whole = len == blob.size();
  if (!write_file(path, blob, len)) {
    expect(false, "cannot write the temporary file");
    return;
  }
  const Bound bound(len);
  const char* why = "";
  if (k == ZKEY) {
    g16_zkey* z = nullptr;
    const g16_status st = g16_zkey_open(path.c_str(), &z);
    expect(whole ? st == G16_OK && examine_zkey(z, w.file, w.zkey, &why) : st == G16_ERR_IO && !z, why);
    g16_zkey_close(z);
  } else if (k == R1CS) {
    g16_r1cs* r = nullptr;
    const g16_status st = g16_r1cs_open(path.c_str(), &r);
    expect(whole ? st == G16_OK && examine_r1cs(r, w.r1cs, &why) : st == G16_ERR_IO && !r, why);
    g16_r1cs_close(r);
  } else if (k == WTNS) {
    g16_wtns* h = nullptr;
    const g16_status st = g16_wtns_open(path.c_str(), &h);
    bool ok = whole ? st == G16_OK && g16_wtns_count(h) == w.wtns->size() : st == G16_ERR_IO && !h;
    if (ok && whole) ok = memcmp(g16_wtns_values(h), w.wtns->data(), w.wtns->size() * 32) == 0;
    expect(ok, "g16_wtns_open");
    g16_wtns_close(h);
    uint64_t* vals = nullptr;
    uint32_t cnt = 0;
    const g16_status st2 = g16_wtns_read(path.c_str(), &vals, &cnt);
    ok = whole ? st2 == G16_OK && cnt == w.wtns->size() : st2 == G16_ERR_IO;
    for (uint32_t i = 0; ok && whole && i < cnt; ++i) ok = memcmp(vals + 4 * i, mont((*w.wtns)[i]).b, 32) == 0;
    expect(ok, "g16_wtns_read");
    if (st2 == G16_OK) g16_free(vals);
  } else {
    g16_ptau* p = nullptr;
    const g16_status st = g16_ptau_open(path.c_str(), &p);
    expect(whole ? st == G16_OK && examine_ptau(p, w.file, w.prepared, &why) : st == G16_ERR_IO && !p, why);
    g16_ptau_close(p);
  }
  unlink(path.c_str());
}

// ---- the cases every format goes through ------------------------------------------------------------------------
const uint32_t kUnusedId = 0x7777;

void container_cases(Kind k, const File& f, const Wants& w, const std::vector<uint32_t>& required,
                     const std::vector<Field>& fields) {
  const Made m = assemble(f);
  const size_t len = m.blob.size();
  const uint32_t nsec = (uint32_t)f.secs.size();
  char g[96];

  snprintf(g, sizeof g, "%s: the valid file (%zu bytes)", kKind[k], len);
  group(g);
  name_case(g, "open_mem");
  expect_valid(k, m.blob, w);
  name_case(g, "path");
  path_case(k, m.blob, len, w);

  snprintf(g, sizeof g, "%s: every truncation", kKind[k]);
  group(g);
  for (size_t t = 0; t < len; ++t) {
    name_case(g, "length", (long long)t);
    expect_refused(k, m.blob, t);
  }
  snprintf(g, sizeof g, "%s: truncated files by path", kKind[k]);
  group(g);
  {
    std::vector<size_t> cuts = {0, 1, 11, 12, 13};
    for (size_t i = 0; i < m.entry.size(); ++i)
      for (size_t b : {m.entry[i], m.entry[i] + 12, m.entry[i] + 12 + f.secs[i].body.size()})
        for (long d : {-1L, 0L, 1L}) cuts.push_back((size_t)((long)b + d));
    for (size_t t : cuts) {
      if (t >= len) continue;
      name_case(g, "length", (long long)t);
      path_case(k, m.blob, t, w);
    }
  }

  snprintf(g, sizeof g, "%s: section permutations", kKind[k]);
  group(g);
  for (uint32_t rot = 0; rot <= nsec; ++rot) {  // every rotation, and the reversed file
    File p = f;
    p.secs.clear();
    for (uint32_t i = 0; i < nsec; ++i) p.secs.push_back(rot == nsec ? f.secs[nsec - 1 - i] : f.secs[(i + rot) % nsec]);
    name_case(g, "rotation", rot);
    expect_valid(k, assemble(p).blob, w);
  }

  snprintf(g, sizeof g, "%s: section count", kKind[k]);
  group(g);
  for (uint32_t v : {0u, nsec - 1, nsec + 1, 1u << 31, 0xFFFFFFFFu}) {
    Bytes b = m.blob;
    poke32(b, 8, v);
    name_case(g, "count", v);
    const g16_status st = expect_refused_or_sound(k, b);
    if (v == 0 || v > nsec) expect(st == G16_ERR_IO, "no section, or more than the file holds, must be refused");
  }

  snprintf(g, sizeof g, "%s: section ids", kKind[k]);
  group(g);
  for (uint32_t i = 0; i < nsec; ++i) {
    Bytes b = m.blob;
    poke32(b, m.entry[i], kUnusedId);
    name_case(g, "section", f.secs[i].id);
    const g16_status st = expect_refused_or_sound(k, b);
    bool req = false;
    for (uint32_t id : required) req = req || id == f.secs[i].id;
    // without its Lagrange sections a prepared file is still a ptau: examine_ptau sees the refusal of g16_ptau_lagrange
    expect(req ? st == G16_ERR_IO : st == G16_OK, req ? "a required section is missing" : "an ignored section is missing");
  }

  snprintf(g, sizeof g, "%s: section sizes", kKind[k]);
  group(g);
  for (uint32_t i = 0; i < nsec; ++i) {
    const uint64_t was = f.secs[i].body.size();
    for (uint64_t v : {(uint64_t)0, was - 1, was + 1, (uint64_t)1 << 32, (uint64_t)1 << 63, ~(uint64_t)0, ~(uint64_t)0 - 11}) {
      if (v == was) continue;
      Bytes b = m.blob;
      poke64(b, m.entry[i] + 4, v);
      name_case(g, "section / size", f.secs[i].id, (long long)v);
      const g16_status st = expect_refused_or_sound(k, b);
      if (v > len - (m.entry[i] + 12)) expect(st == G16_ERR_IO, "a section larger than what is left of the file");
    }
  }

  snprintf(g, sizeof g, "%s: header counts", kKind[k]);
  group(g);
  for (const Field& fd : fields) {
    const size_t at = body_of(f, m, fd.sec) + fd.off;
    if (fd.wide) {
      const uint64_t was = peek64(m.blob, at);
      for (uint64_t v : {(uint64_t)0, (uint64_t)1, was - 1, was + 1, (uint64_t)0x7FFFFFFF, (uint64_t)1 << 31, (uint64_t)0xFFFFFFFE,
                         (uint64_t)0xFFFFFFFF, (uint64_t)1 << 32, (uint64_t)1 << 63, ~(uint64_t)0}) {
        if (v == was) continue;
        Bytes b = m.blob;
        poke64(b, at, v);
        name_case(g, fd.name, (long long)fd.off, (long long)v);
        expect_refused_or_sound(k, b);
      }
      continue;
    }
    const uint32_t was = peek32(m.blob, at);
    for (uint32_t v : {0u, 1u, was - 1, was + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
      if (v == was) continue;
      Bytes b = m.blob;
      poke32(b, at, v);
      name_case(g, fd.name, (long long)fd.off, v);
      expect_refused_or_sound(k, b);
    }
  }
}

// ---- what only one format has -----------------------------------------------------------------------------------
void zkey_cases() {
  ZkeyWant want;
  const File f = zkey_file(&want);
  Wants w;
  w.file = &f;
  w.zkey = &want;
  container_cases(ZKEY, f, w, {2, 3, 4, 5, 6, 7, 8, 9}, zkey_fields());

  const char* g = "zkey: duplicate sections, the first wins";
  group(g);
  File d = f;
  d.secs.push_back({3, filler(33, 2 * 64)});
  d.secs.push_back({5, filler(35, 5 * 64)});
  Bytes h2 = sec_of(f, 2);
  poke32(h2, 72, 4);  // another n_vars
  d.secs.push_back({2, h2});
  Bytes c2 = sec_of(f, 4);
  poke32(c2, 4 + 8, 1);  // another signal in the first record
  d.secs.push_back({4, c2});
  name_case(g, "sections 3, 5, 2, 4 twice");
  expect_valid(ZKEY, assemble(d).blob, w);

  g = "zkey: counts named by the issue";
  group(g);
  const Made m = assemble(f);
  const size_t hdr = body_of(f, m, 2);
  struct {
    size_t off;
    uint32_t v;
  } refused[] = {{76, 0xFFFFFFFFu}, {76, 5}, {76, 4}, {72, 1}, {80, 1}, {72, 6}, {80, 5}};
  for (auto& c : refused) {  // n_public + 1 against n_vars and the domain in 64 bits; arrays longer than their sections
    Bytes b = m.blob;
    poke32(b, hdr + c.off, c.v);
    name_case(g, "header", (long long)c.off, c.v);
    expect_refused(ZKEY, b, b.size());
  }
}

void r1cs_cases() {
  R1csWant want;
  std::vector<Field> fields;
  const File f = r1cs_file(&want, &fields);
  Wants w;
  w.r1cs = &want;
  container_cases(R1CS, f, w, {1, 2, 3}, fields);
  const Made m = assemble(f);
  const size_t hdr = body_of(f, m, 1);

  const char* g = "r1cs: counts named by the issue";
  group(g);
  {
    Bytes b = m.blob;
    poke32(b, hdr + 60, 0xFFFFFFFFu);  // 3 x 16 GiB of row pointers if it is believed
    name_case(g, "n_constraints = 2^32 - 1");
    expect_refused(R1CS, b, b.size());
    b = m.blob;
    poke32(b, hdr + 60, (uint32_t)(sec_of(f, 2).size() / 12 + 1));
    name_case(g, "n_constraints = section / 12 + 1");
    expect_refused(R1CS, b, b.size());
    b = m.blob;
    poke32(b, hdr + 40, 0x7FFFFFFFu);  // num_aux = 5 - 0x80000001 wrapped to 2147483652 before
    name_case(g, "n_pub_out = 2^31 - 1");
    expect_refused(R1CS, b, b.size());
    b = m.blob;
    poke32(b, hdr + 44, 0xFFFFFFFFu);  // num_inputs wrapped to 1 + n_pub_out - 1 before
    name_case(g, "n_pub_in = 2^32 - 1");
    expect_refused(R1CS, b, b.size());
    b = m.blob;
    poke32(b, hdr + 36, 2);  // 1 + 1 + 1 > 2
    name_case(g, "n_wires = 2");
    expect_refused(R1CS, b, b.size());
    b = m.blob;
    poke32(b, hdr + 36, 3);  // num_aux = 0 is a circuit; the map section no longer matches
    name_case(g, "n_wires = 3");
    expect_refused(R1CS, b, b.size());
  }

  g = "r1cs: a wire index >= n_wires is accepted here (pinned): g16_ctx_create and the setup calls refuse it";
  group(g);
  for (const Field& fd : fields) {
    if (strcmp(fd.name, "wire index") != 0) continue;
    Bytes b = m.blob;
    poke32(b, body_of(f, m, 2) + fd.off, 5);
    name_case(g, "wire index = n_wires", (long long)fd.off);
    const Outcome o = parse(R1CS, b, b.size());
    expect(o.st == G16_OK && o.sound, o.why);
  }

  g = "r1cs: duplicate sections, the last wins";
  group(g);
  {
    auto rows = r1cs_rows();
    rows[0][0][0].canonical = small(1234567);  // distinguishable
    rows[2][1][0].wire = 4;
    R1csWant want2 = want;
    r1cs_want_rows(rows, &want2);
    want2.labels = {0, 2, 4, 6, 8};
    Bytes map2;
    for (uint64_t l : want2.labels) put64(map2, l);
    File d = f;
    d.secs.push_back({2, r1cs_constraints(rows, nullptr)});
    d.secs.push_back({3, map2});
    Wants w2;
    w2.r1cs = &want2;
    name_case(g, "sections 2 and 3 twice");
    expect_valid(R1CS, assemble(d).blob, w2);
    // the header too: a second one that asks for more constraints than the constraint section holds
    Bytes h2 = sec_of(f, 1);
    poke32(h2, 60, 4);
    File e = f;
    e.secs.push_back({1, h2});
    name_case(g, "section 1 twice");
    expect_refused(R1CS, assemble(e).blob, assemble(e).blob.size());
  }

  g = "r1cs: coefficients at the edge of the field";
  group(g);
  const V32 edge[] = {r_plus(0), r_plus(1), all_ones(), r_plus(-1), small(0)};
  for (int e = 0; e < 5; ++e)
    for (int where = 0; where < 2; ++where) {  // the first coefficient of the file and the last
      auto rows = r1cs_rows();
      Term& t = where ? rows[2][1][0] : rows[0][0][0];
      t.canonical = edge[e];
      File x = f;
      x.secs[0].body = r1cs_constraints(rows, nullptr);
      const Bytes b = assemble(x).blob;
      name_case(g, "value / position", e, where);
      if (e < 3) {
        expect_refused(R1CS, b, b.size());
        continue;
      }
      R1csWant wx = want;
      r1cs_want_rows(rows, &wx);
      Wants ww;
      ww.r1cs = &wx;
      expect_valid(R1CS, b, ww);
      // and back through g16_fr_to_canonical
      g16_r1cs* r = nullptr;
      expect(g16_r1cs_open_mem(b.data(), b.size(), &r) == G16_OK, "open");
      g16_csr A, B;
      expect(r && g16_r1cs_matrices(r, &A, &B, nullptr) == G16_OK, "matrices");
      if (r) {
        V32 back;
        const uint64_t* c = where ? B.coeff + 4 * (B.nnz - 1) : A.coeff;
        expect(g16_fr_to_canonical(c, back.b, 1) == G16_OK && back == edge[e], "round trip");
      }
      g16_r1cs_close(r);
    }
}

void wtns_cases() {
  const std::vector<V32> vals = wtns_values();
  const File f = wtns_file(vals);
  Wants w;
  w.wtns = &vals;
  container_cases(WTNS, f, w, {1, 2}, {{"n8", 1, 0, false}, {"value count", 1, 36, false}});

  const char* g = "wtns: duplicate sections, the last wins";
  group(g);
  {
    std::vector<V32> other = {small(1), small(34), small(2), small(17)};
    File d = f;
    d.secs.push_back({2, wtns_file(other).secs[1].body});
    Wants w2;
    w2.wtns = &other;
    name_case(g, "section 2 twice");
    expect_valid(WTNS, assemble(d).blob, w2);
  }

  g = "wtns: values at the edge of the field";
  group(g);
  const V32 edge[] = {r_plus(0), r_plus(1), all_ones(), r_plus(-1), small(0)};
  for (int e = 0; e < 5; ++e)
    for (size_t where : {(size_t)0, vals.size() - 1}) {
      std::vector<V32> v = vals;
      v[where] = edge[e];
      const Bytes b = assemble(wtns_file(v)).blob;
      name_case(g, "value / position", e, (long long)where);
      uint64_t* out = nullptr;
      uint32_t n = 0;
      const Bound bound(b.size());
      const g16_status st = exact(b, b.size(), [&](const uint8_t* d, size_t len) { return g16_wtns_read_mem(d, len, &out, &n); });
      if (e < 3) {
        expect(st == G16_ERR_IO, "a value >= r must be refused by the converting read");
      } else {
        V32 back;
        expect(st == G16_OK && n == v.size() && g16_fr_to_canonical(out + 4 * where, back.b, 1) == G16_OK && back == edge[e],
               "round trip");
      }
      if (st == G16_OK) g16_free(out);
      // the view hands the bytes out as they are (no range test: g16_loaders.h), parse_wtns checks both against each other
      Wants wv;
      wv.wtns = &v;
      expect_valid(WTNS, b, wv);
    }
}

void ptau_cases() {
  for (bool prepared : {false, true}) {
    const File f = ptau_file(prepared);
    Wants w;
    w.file = &f;
    w.prepared = prepared;
    const Kind k = prepared ? PTAU_PREPARED : PTAU;
    container_cases(k, f, w, {1, 2, 3, 4, 5, 6},
                    {{"n8", 1, 0, false}, {"power", 1, 36, false}, {"ceremony_power", 1, 40, false}});
    const Made m = assemble(f);

    const char* g = "ptau: duplicate sections, the first wins";
    group(g);
    File d = f;
    d.secs.push_back({6, filler(66, 128)});
    d.secs.push_back({2, filler(62, 7 * 64)});
    Bytes h2 = sec_of(f, 1);
    poke32(h2, 36, 3);
    d.secs.push_back({1, h2});
    if (prepared) d.secs.push_back({13, filler(63, 7 * 128)});
    name_case(g, "sections 6, 2, 1 (and 13) twice", prepared);
    expect_valid(k, assemble(d).blob, w);

    g = "ptau: powers, magic, version, prime";
    group(g);
    const size_t hdr = body_of(f, m, 1);
    for (uint32_t p : {0u, 1u, 3u, 27u, 28u, 29u, 31u, 32u, 33u, 63u, 64u}) {  // 1 << power must never be taken of these
      Bytes b = m.blob;
      poke32(b, hdr + 36, p);
      name_case(g, "power", p);
      expect_refused(k, b, b.size());
    }
    Bytes b = m.blob;
    b[0] = 'q';
    name_case(g, "magic");
    expect_refused(k, b, b.size());
    b = m.blob;
    poke32(b, 4, 2);
    name_case(g, "version");
    expect_refused(k, b, b.size());
    b = m.blob;
    memcpy(b.data() + hdr + 4, kR.b, 32);
    name_case(g, "the scalar field's prime");
    expect_refused(k, b, b.size());
    if (prepared) {  // a Lagrange section of another size: still a ptau, not a prepared one
      for (uint32_t id : {12u, 13u, 14u, 15u}) {
        File x = f;
        for (Sec& s : x.secs)
          if (s.id == id) s.body.resize(s.body.size() - 64);
        Wants wx = w;
        wx.prepared = false;
        wx.file = &x;
        name_case(g, "short Lagrange section", id);
        expect_valid(PTAU, assemble(x).blob, wx);
      }
    }
  }
}

void fr_cases() {
  const char* g = "g16_fr_from_canonical / g16_fr_to_canonical";
  group(g);
  uint64_t limbs[8];
  V32 back;
  name_case(g, "2^256 mod r");
  expect(g16_fr_from_canonical(small(1).b, limbs, 1) == G16_OK && memcmp(limbs, kMontOne.b, 32) == 0, "Montgomery one");
  const V32 bad[] = {r_plus(0), r_plus(1), all_ones()};
  for (int i = 0; i < 3; ++i) {
    name_case(g, "refused value", i);
    expect(g16_fr_from_canonical(bad[i].b, limbs, 1) == G16_ERR_INVALID, "a value >= r");
    uint8_t two[64];  // as the second of two
    memcpy(two, small(5).b, 32);
    memcpy(two + 32, bad[i].b, 32);
    expect(g16_fr_from_canonical(two, limbs, 2) == G16_ERR_INVALID, "a value >= r behind a good one");
  }
  const V32 good[] = {r_plus(-1), small(0), small(1), small(0xFFFFFFFFFFFFFFFFull)};
  for (int i = 0; i < 4; ++i) {
    name_case(g, "accepted value", i);
    expect(g16_fr_from_canonical(good[i].b, limbs, 1) == G16_OK && g16_fr_to_canonical(limbs, back.b, 1) == G16_OK &&
               back == good[i],
           "round trip");
  }
  expect(g16_fr_from_canonical(nullptr, limbs, 1) == G16_ERR_INVALID && g16_fr_to_canonical(limbs, nullptr, 1) == G16_ERR_INVALID,
         "NULL");
}

void null_cases() {
  const char* g = "NULL arguments";
  group(g);
  name_case(g, "opens");
  const Bytes b = assemble(wtns_file(wtns_values())).blob;
  g16_zkey* z = nullptr;
  g16_r1cs* r = nullptr;
  g16_wtns* w = nullptr;
  g16_ptau* p = nullptr;
  uint64_t* v = nullptr;
  uint32_t n = 0;
  expect(g16_zkey_open_mem(nullptr, 4, &z) == G16_ERR_INVALID && g16_zkey_open_mem(b.data(), b.size(), nullptr) == G16_ERR_INVALID);
  expect(g16_r1cs_open_mem(nullptr, 4, &r) == G16_ERR_INVALID && g16_r1cs_open_mem(b.data(), b.size(), nullptr) == G16_ERR_INVALID);
  expect(g16_wtns_open_mem(nullptr, 4, &w) == G16_ERR_INVALID && g16_wtns_open_mem(b.data(), b.size(), nullptr) == G16_ERR_INVALID);
  expect(g16_ptau_open_mem(nullptr, 4, &p) == G16_ERR_INVALID && g16_ptau_open_mem(b.data(), b.size(), nullptr) == G16_ERR_INVALID);
  expect(g16_wtns_read_mem(nullptr, 4, &v, &n) == G16_ERR_INVALID && g16_wtns_read_mem(b.data(), b.size(), nullptr, &n) == G16_ERR_INVALID);
  expect(g16_zkey_open(nullptr, &z) == G16_ERR_INVALID && g16_r1cs_open(nullptr, &r) == G16_ERR_INVALID &&
         g16_wtns_open(nullptr, &w) == G16_ERR_INVALID && g16_ptau_open(nullptr, &p) == G16_ERR_INVALID &&
         g16_wtns_read(nullptr, &v, &n) == G16_ERR_INVALID);
  name_case(g, "a file that is not there");
  const std::string gone = tmp_path("no-such-file");
  expect(g16_zkey_open(gone.c_str(), &z) == G16_ERR_IO && !z && g16_r1cs_open(gone.c_str(), &r) == G16_ERR_IO && !r &&
         g16_wtns_open(gone.c_str(), &w) == G16_ERR_IO && !w && g16_ptau_open(gone.c_str(), &p) == G16_ERR_IO && !p &&
         g16_wtns_read(gone.c_str(), &v, &n) == G16_ERR_IO);
}

// ---- the .zkey writer: its descriptor is checked before the file is created ------------------------------------
void writer_cases() {
  const char* g = "g16_zkey_write";
  group(g);
  ZkeyWant want;
  const File f = zkey_file(&want);
  g16_key_desc key;
  memset(&key, 0, sizeof key);
  key.n_vars = 5;
  key.n_public = 1;
  key.domain_size = 4;
  key.a_query = sec_of(f, 5).data();
  key.b_g1_query = sec_of(f, 6).data();
  key.b_g2_query = sec_of(f, 7).data();
  key.l_query = sec_of(f, 8).data();
  key.h_query = sec_of(f, 9).data();
  const uint8_t* pts = sec_of(f, 2).data() + 84;
  memcpy(key.alpha_g1, pts, 64);
  memcpy(key.beta_g1, pts + 64, 64);
  memcpy(key.beta_g2, pts + 128, 128);
  memcpy(key.delta_g1, pts + 384, 64);
  memcpy(key.delta_g2, pts + 448, 128);
  const uint8_t* gamma = pts + 256;
  const uint8_t* ic = sec_of(f, 3).data();
  auto csr_of = [](const Csr& c) {
    g16_csr v;
    v.row_ptr = c.rowptr.data();
    v.col = c.col.data();
    v.coeff = (const uint64_t*)c.val.data();
    v.nnz = c.col.size();
    return v;
  };
  const g16_csr a = csr_of(want.a), b = csr_of(want.b);
  const std::string path = tmp_path("written.zkey");

  name_case(g, "the valid call reads back");
  expect(g16_zkey_write(path.c_str(), &key, ic, gamma, &a, &b, want.nc) == G16_OK, "write");
  {
    g16_zkey* z = nullptr;
    const char* why = "";
    expect(g16_zkey_open(path.c_str(), &z) == G16_OK && examine_zkey(z, &f, &want, &why), why);
    g16_zkey_close(z);
  }
  unlink(path.c_str());

  auto refused = [&](const char* what, const g16_key_desc& k, const g16_csr& A, const g16_csr& B, uint32_t nc) {
    name_case(g, what);
    expect(g16_zkey_write(path.c_str(), &k, ic, gamma, &A, &B, nc) == G16_ERR_INVALID, "not G16_ERR_INVALID");
    expect(access(path.c_str(), F_OK) != 0, "the file was created");
    unlink(path.c_str());
  };
  g16_key_desc k = key;
  k.n_vars = 1;  // (N - p - 1) * 64 wrapped to hundreds of gigabytes of l_query before
  refused("n_vars < n_public + 1", k, a, b, want.nc);
  k = key;
  k.n_public = 0xFFFFFFFFu;
  refused("n_public + 1 wraps", k, a, b, want.nc);
  const uint8_t* g16_key_desc::*queries[] = {&g16_key_desc::a_query, &g16_key_desc::b_g1_query, &g16_key_desc::b_g2_query,
                                             &g16_key_desc::l_query, &g16_key_desc::h_query};
  for (auto q : queries) {
    k = key;
    k.*q = nullptr;
    refused("a NULL query with a count that is not zero", k, a, b, want.nc);
  }
  for (int which = 0; which < 2; ++which) {
    g16_csr x = which ? b : a;
    x.nnz += 1;
    refused("row_ptr[num_constraints] != nnz", key, which ? a : x, which ? x : b, want.nc);
    x = which ? b : a;
    refused("row_ptr[num_constraints] != nnz: fewer constraints", key, which ? a : x, which ? x : b, want.nc - 1);
    x.row_ptr = nullptr;
    refused("row_ptr NULL", key, which ? a : x, which ? x : b, want.nc);
    x = which ? b : a;
    x.col = nullptr;
    refused("col NULL", key, which ? a : x, which ? x : b, want.nc);
    const uint32_t down[3] = {0, 5, (uint32_t)x.nnz};  // spans [0, nnz], steps back in between
    x = which ? b : a;
    x.row_ptr = down;
    refused("row_ptr not monotone", key, which ? a : x, which ? x : b, want.nc);
  }
  {
    // 2^32 - 1 coefficients in a alone: with b's and the appended rows the count no longer fits the u32 of the file.
    // The arrays are never read: the refusal comes first.
    const uint32_t huge[2] = {0, 0xFFFFFFFFu};
    g16_csr x = a;
    x.row_ptr = huge;
    x.nnz = 0xFFFFFFFFu;
    const uint32_t small_rp[2] = {0, (uint32_t)b.nnz};
    g16_csr y = b;
    y.row_ptr = small_rp;
    refused("a coefficient count that does not fit in 32 bits", key, x, y, 1);
  }
  name_case(g, "NULL arguments");
  expect(g16_zkey_write(nullptr, &key, ic, gamma, &a, &b, want.nc) == G16_ERR_INVALID &&
         g16_zkey_write(path.c_str(), nullptr, ic, gamma, &a, &b, want.nc) == G16_ERR_INVALID &&
         g16_zkey_write(path.c_str(), &key, nullptr, gamma, &a, &b, want.nc) == G16_ERR_INVALID &&
         g16_zkey_write(path.c_str(), &key, ic, gamma, nullptr, &b, want.nc) == G16_ERR_INVALID);
}

}  // namespace

int main() {
  signal(SIGABRT, on_abort);
  const char* base = getenv("TMPDIR");
  std::string tmpl = std::string(base && *base ? base : "/tmp") + "/g16_loaders_XXXXXX";
  if (!mkdtemp(&tmpl[0])) {
    perror("mkdtemp");
    return 2;
  }
  g_tmpdir = tmpl;
#ifdef LOADERS_ALLOC_BOUND
  printf("# allocation bound: 4 x file + 64 KiB per request\n");
#endif
  fr_cases();
  zkey_cases();
  r1cs_cases();
  wtns_cases();
  ptau_cases();
  null_cases();
  writer_cases();
  rmdir(g_tmpdir.c_str());
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
