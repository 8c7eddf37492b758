// loaders.cpp -- host-side loaders behind include/g16_loaders.h.
//
//   zkey : reference src/zkey.rs  (BinFile::new :73-101, proving_key :103-133, matrices :151-196,
//          HeaderGroth::read :288-317, deserialize_field_fr :322-325, deserialize_g1/g2 :340-360)
//   r1cs : reference src/circom/r1cs_reader.rs (R1CSFile::new :54-146, Header::new :161-200,
//          read_constraint_vec :203-213, read_constraints :215-229, read_map :231-249, R1CS::from :26-39)
//   ptau : snarkjs powers-of-tau files, the same container (not parsed by the reference; g16_loaders.h)
// The point sections are handed out as zero-copy views: the on-disk encoding (x|y Montgomery LE,
// all-zero = infinity) is already the device encoding.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <exception>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/g16_loaders.h"
#include "field.h"

using g16::Fr;
using g16::U256;

namespace {

thread_local std::string t_err;

g16_status fail(g16_status code, const std::string& m) {
  t_err = m;
  return code;
}

// No exception leaves an extern "C" function of g16_loaders.h: every entry point that allocates runs its body in
// here.  A handle that is still half built sits in a unique_ptr inside the body, so it is freed on the way out and
// *out stays NULL.
template <class Body>
g16_status guarded(Body&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(G16_ERR_INTERNAL, "out of memory");
  } catch (const std::length_error&) {
    return fail(G16_ERR_INTERNAL, "out of memory");
  } catch (const std::exception& e) {
    return fail(G16_ERR_INTERNAL, e.what());
  } catch (...) {
    return fail(G16_ERR_INTERNAL, "unknown exception");
  }
}

bool read_file(const char* path, std::vector<uint8_t>& out, std::string& err) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    err = std::string("cannot open ") + path;
    return false;
  }
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (sz < 0) {
    fclose(f);
    err = "cannot stat file";
    return false;
  }
  out.resize((size_t)sz);
  size_t got = sz ? fread(out.data(), 1, (size_t)sz, f) : 0;
  fclose(f);
  if (got != (size_t)sz) {
    err = "short read";
    return false;
  }
  return true;
}

struct Cursor {
  const uint8_t* p;
  size_t n, o = 0;
  bool ok = true;
  Cursor(const uint8_t* p_, size_t n_, size_t o_ = 0) : p(p_), n(n_), o(o_) {}
  bool need(size_t k) {
    if (!ok || o + k > n || o + k < o) {
      ok = false;
      return false;
    }
    return true;
  }
  uint32_t u32() {
    if (!need(4)) return 0;
    uint32_t v;
    memcpy(&v, p + o, 4);
    o += 4;
    return v;
  }
  uint64_t u64() {
    if (!need(8)) return 0;
    uint64_t v;
    memcpy(&v, p + o, 8);
    o += 8;
    return v;
  }
  const uint8_t* bytes(size_t k) {
    if (!need(k)) return nullptr;
    const uint8_t* r = p + o;
    o += k;
    return r;
  }
  void skip(uint64_t k) {
    if (!ok || k > n - o) {
      ok = false;
      return;
    }
    o += (size_t)k;
  }
};

struct Section {
  size_t pos;
  uint64_t size;
};

const uint8_t kR1csPrime[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9,
                                0x79, 0x48, 0xe8, 0x33, 0x28, 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45,
                                0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

bool fr_lt_modulus(const uint8_t* le32) {
  for (int i = 31; i >= 0; --i) {
    if (le32[i] < kR1csPrime[i]) return true;
    if (le32[i] > kR1csPrime[i]) return false;
  }
  return false;  // equal
}

Fr fr_load(const uint8_t* le32) {
  Fr a;
  memcpy(a.v, le32, 32);
  return a;
}

struct CsrOwned {
  std::vector<uint32_t> rowptr, col;
  std::vector<Fr> val;
  g16_csr view() const {
    g16_csr c;
    c.row_ptr = rowptr.data();
    c.col = col.data();
    c.coeff = (const uint64_t*)val.data();
    c.nnz = col.size();
    return c;
  }
};

}  // namespace

// Read-only view of a whole file.  g16_zkey_open maps the file (the 64 / 128-byte point sections are
// handed to g16_ctx_create straight out of the page cache: no 6 GiB host copy at 2^24, and the
// reference's one-Read-call-per-field-element loop, src/zkey.rs:328-368, becomes page faults);
// g16_zkey_open_mem owns a copy of the caller's buffer.
struct FileView {
  const uint8_t* p = nullptr;
  size_t n = 0;
  void* map = nullptr;  // non-null: munmap on release
  std::vector<uint8_t> own;
  FileView() = default;
  FileView(const FileView&) = delete;
  FileView& operator=(const FileView&) = delete;
  ~FileView() {
    if (map) munmap(map, n);
  }
  void copy_of(const uint8_t* d, size_t len) {
    own.assign(d, d + len);
    p = own.data();
    n = own.size();
  }
  bool map_file(const char* path, std::string& err) {
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
      err = std::string("cannot open ") + path;
      return false;
    }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 0) {
      close(fd);
      err = "cannot stat file";
      return false;
    }
    n = (size_t)st.st_size;
    if (n == 0) {  // mmap of length 0 is an error; an empty file is a truncated header downstream
      close(fd);
      p = own.data();
      return true;
    }
    void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) {
      err = "mmap failed";
      n = 0;
      return false;
    }
    // No MADV_SEQUENTIAL: the sharded provers read the H section strided (global_index(t)) and a
    // multi-device ctx uploads every section once per device.  G16_ZKEY_COPY=1 reads the file into
    // owned memory instead of mapping it: a zkey that is truncated or rewritten while the handle is
    // open then cannot raise SIGBUS inside a later upload (the mapping requires the file to stay
    // unchanged until g16_zkey_close; include/g16_loaders.h says so).
    if (const char* e = getenv("G16_ZKEY_COPY")) {
      if (e[0] == '1') {
        own.assign((const uint8_t*)m, (const uint8_t*)m + n);
        munmap(m, n);
        p = own.data();
        return true;
      }
    }
    // sequential access hint only: MADV_WILLNEED on a multi-10-GB zkey would start a whole-file
    // readahead up front, while the sections are uploaded one after another
    (void)madvise(m, n, MADV_SEQUENTIAL);
    map = m;
    p = (const uint8_t*)m;
    return true;
  }
  const uint8_t* data() const { return p; }
  size_t size() const { return n; }
};

struct g16_zkey {
  FileView data;
  std::map<uint32_t, Section> sec;  // first occurrence wins (get_section, zkey.rs:135-137)
  g16_zkey_header hdr;
  bool have_matrices = false;
  g16_matrices mat;
  CsrOwned A, B;
};

struct g16_ptau {
  FileView data;
  std::map<uint32_t, Section> sec;  // first occurrence wins, as for a zkey
  g16_ptau_header hdr;
};

struct g16_r1cs {
  g16_r1cs_header hdr;
  CsrOwned A, B, C;
  std::vector<uint64_t> wire_mapping;
};

namespace {

g16_status zkey_parse(g16_zkey* z) {
  const uint8_t* d = z->data.data();
  const size_t n = z->data.size();
  Cursor c(d, n);
  c.bytes(4);  // magic: the reference does not check it (zkey.rs:74-75)
  (void)c.u32();
  const uint32_t nsec = c.u32();
  if (!c.ok) return fail(G16_ERR_IO, "zkey: truncated file header");
  for (uint32_t i = 0; i < nsec; ++i) {
    const uint32_t id = c.u32();
    const uint64_t len = c.u64();
    if (!c.ok) return fail(G16_ERR_IO, "zkey: truncated section table");
    if (!z->sec.count(id)) z->sec[id] = Section{c.o, len};
    c.skip(len);
    if (!c.ok) return fail(G16_ERR_IO, "zkey: section runs past the end of the file");
  }
  for (uint32_t id : {2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u})
    if (!z->sec.count(id)) return fail(G16_ERR_IO, "zkey: missing section " + std::to_string(id));
  // HeaderGroth::read (zkey.rs:288-317)
  Cursor h(d, n, z->sec[2].pos);
  g16_zkey_header& H = z->hdr;
  memset(&H, 0, sizeof H);
  H.n8q = h.u32();
  if (H.n8q != 32) return fail(G16_ERR_IO, "zkey: n8q != 32");
  const uint8_t* q = h.bytes(32);
  H.n8r = h.u32();
  if (!h.ok || H.n8r != 32) return fail(G16_ERR_IO, "zkey: n8r != 32");
  const uint8_t* r = h.bytes(32);
  H.n_vars = h.u32();
  H.n_public = h.u32();
  H.domain_size = h.u32();
  const uint8_t* pts = h.bytes(64 + 64 + 128 + 128 + 64 + 128);
  if (!h.ok) return fail(G16_ERR_IO, "zkey: truncated groth16 header");
  memcpy(H.q, q, 32);
  memcpy(H.r, r, 32);
  uint32_t pw = 0;
  while (((uint64_t)1 << pw) < H.domain_size) ++pw;  // ark_std::log2 = ceil(log2)
  H.power = pw;
  // ZVerifyingKey::new order (zkey.rs:241-257): alpha1, beta1, beta2, gamma2, delta1, delta2
  memcpy(H.alpha_g1, pts, 64);
  memcpy(H.beta_g1, pts + 64, 64);
  memcpy(H.beta_g2, pts + 128, 128);
  memcpy(H.gamma_g2, pts + 256, 128);
  memcpy(H.delta_g1, pts + 384, 64);
  memcpy(H.delta_g2, pts + 448, 128);
  // 64-bit comparisons: n_public = 0xFFFFFFFF must not wrap n_public + 1 to 0
  if ((uint64_t)H.n_public + 1 > (uint64_t)H.n_vars)
    return fail(G16_ERR_IO, "zkey: n_vars < n_public + 1");
  if ((uint64_t)H.n_public + 1 > (uint64_t)H.domain_size)
    return fail(G16_ERR_IO, "zkey: domain_size < n_public + 1");
  // section sizes the proving_key() reads rely on (zkey.rs:107-111)
  struct Need {
    uint32_t id;
    uint64_t bytes;
  } needs[] = {{3, ((uint64_t)H.n_public + 1) * 64},
               {5, (uint64_t)H.n_vars * 64},
               {6, (uint64_t)H.n_vars * 64},
               {7, (uint64_t)H.n_vars * 128},
               {8, ((uint64_t)H.n_vars - H.n_public - 1) * 64},
               {9, (uint64_t)H.domain_size * 64}};
  for (auto& nd : needs)
    if (z->sec[nd.id].size < nd.bytes)
      return fail(G16_ERR_IO, "zkey: section " + std::to_string(nd.id) + " is too short");
  return G16_OK;
}

// snarkjs .ptau (include/g16_loaders.h).  Written from knowledge of snarkjs: there
// was no .ptau file to pin the reader to.
constexpr uint32_t kPtauMaxPower = 28;

uint64_t ptau_section_bytes(uint32_t id, uint32_t power) {
  const uint64_t n = (uint64_t)1 << power;
  switch (id) {
    case 2: return (2 * n - 1) * 64;
    case 3: return n * 128;
    case 4: case 5: return n * 64;
    case 12: return (4 * n - 1) * 64;  // levels 0 .. power + 1
    case 13: return (2 * n - 1) * 128; // levels 0 .. power
    case 14: case 15: return (2 * n - 1) * 64;
    default: return 128;  // 6
  }
}

g16_status ptau_parse(g16_ptau* z) {
  const uint8_t* d = z->data.data();
  const size_t n = z->data.size();
  Cursor c(d, n);
  const uint8_t* magic = c.bytes(4);
  if (!magic) return fail(G16_ERR_IO, "ptau: truncated file header");
  if (memcmp(magic, "ptau", 4) != 0) return fail(G16_ERR_IO, "ptau: bad magic");
  const uint32_t version = c.u32();
  const uint32_t nsec = c.u32();
  if (!c.ok) return fail(G16_ERR_IO, "ptau: truncated file header");
  if (version != 1) return fail(G16_ERR_IO, "ptau: unsupported version " + std::to_string(version));
  for (uint32_t i = 0; i < nsec; ++i) {
    const uint32_t id = c.u32();
    const uint64_t len = c.u64();
    if (!c.ok) return fail(G16_ERR_IO, "ptau: truncated section table");
    if (!z->sec.count(id)) z->sec[id] = Section{c.o, len};
    c.skip(len);
    if (!c.ok) return fail(G16_ERR_IO, "ptau: section " + std::to_string(id) + " runs past the end of the file");
  }
  for (uint32_t id : {1u, 2u, 3u, 4u, 5u, 6u})
    if (!z->sec.count(id)) return fail(G16_ERR_IO, "ptau: missing section " + std::to_string(id));
  const Section s1 = z->sec[1];
  Cursor h(d, s1.pos + (size_t)s1.size, s1.pos);  // the section lies inside the file: checked above
  g16_ptau_header& H = z->hdr;
  memset(&H, 0, sizeof H);
  H.n8q = h.u32();
  if (!h.ok) return fail(G16_ERR_IO, "ptau: truncated header section");
  if (H.n8q != 32) return fail(G16_ERR_IO, "ptau: n8 != 32");
  const uint8_t* q = h.bytes(32);
  H.power = h.u32();
  H.ceremony_power = h.u32();
  if (!h.ok) return fail(G16_ERR_IO, "ptau: truncated header section");
  if (memcmp(q, g16::FqParams::MOD, 32) != 0) return fail(G16_ERR_IO, "ptau: the prime is not the BN254 base field's");
  memcpy(H.q, q, 32);
  if (H.power > kPtauMaxPower)
    return fail(G16_ERR_IO, "ptau: power " + std::to_string(H.power) + " > " + std::to_string(kPtauMaxPower));
  for (uint32_t id : {2u, 3u, 4u, 5u, 6u})
    if (z->sec[id].size != ptau_section_bytes(id, H.power))
      return fail(G16_ERR_IO, "ptau: section " + std::to_string(id) + " has " + std::to_string(z->sec[id].size) +
                                  " bytes, power " + std::to_string(H.power) + " needs " +
                                  std::to_string(ptau_section_bytes(id, H.power)));
  return G16_OK;
}

g16_status r1cs_parse(const uint8_t* d, size_t n, g16_r1cs* R) {
  Cursor c(d, n);
  const uint8_t* magic = c.bytes(4);
  if (!magic || memcmp(magic, "r1cs", 4) != 0) return fail(G16_ERR_IO, "Invalid magic number");
  const uint32_t version = c.u32();
  if (!c.ok) return fail(G16_ERR_IO, "unexpected end of file");
  if (version != 1) return fail(G16_ERR_IO, "Unsupported version");
  const uint32_t nsec = c.u32();
  std::map<uint32_t, Section> sec;  // later duplicates overwrite (HashMap::insert, :85-86)
  for (uint32_t i = 0; i < nsec; ++i) {
    const uint32_t ty = c.u32();
    const uint64_t sz = c.u64();
    if (!c.ok) return fail(G16_ERR_IO, "unexpected end of file");
    sec[ty] = Section{c.o, sz};
    c.skip(sz);
    if (!c.ok) return fail(G16_ERR_IO, "unexpected end of file");
  }
  if (!sec.count(1)) return fail(G16_ERR_IO, "No section offset for header type found");
  g16_r1cs_header& H = R->hdr;
  memset(&H, 0, sizeof H);
  H.version = version;
  {
    Cursor h(d, n, sec[1].pos);
    H.field_size = h.u32();
    if (!h.ok) return fail(G16_ERR_IO, "unexpected end of file");
    if (H.field_size != 32) return fail(G16_ERR_IO, "This parser only supports 32-byte fields");
    if (sec[1].size != 32 + (uint64_t)H.field_size)
      return fail(G16_ERR_IO, "Invalid header section size");
    const uint8_t* prime = h.bytes(32);
    if (!prime) return fail(G16_ERR_IO, "unexpected end of file");
    if (memcmp(prime, kR1csPrime, 32) != 0) return fail(G16_ERR_IO, "This parser only supports bn256");
    memcpy(H.prime, prime, 32);
    H.n_wires = h.u32();
    H.n_pub_out = h.u32();
    H.n_pub_in = h.u32();
    H.n_prv_in = h.u32();
    H.n_labels = h.u64();
    H.n_constraints = h.u32();
    if (!h.ok) return fail(G16_ERR_IO, "unexpected end of file");
    // 64-bit: n_pub_in = 0xFFFFFFFF must not wrap num_inputs to 0, nor num_aux past n_wires (R1CS::from, :28-30)
    if ((uint64_t)1 + H.n_pub_in + H.n_pub_out > (uint64_t)H.n_wires)
      return fail(G16_ERR_IO, "1 + n_pub_in + n_pub_out exceeds n_wires");
  }
  if (!sec.count(2)) return fail(G16_ERR_IO, "No section offset for constraint type found");
  // a constraint is at least its three term counts: a count the section cannot hold is refused before anything
  // is reserved for it (n_constraints = 0xFFFFFFFF would ask for 3 x 16 GiB of row pointers)
  if ((uint64_t)H.n_constraints > sec[2].size / 12)
    return fail(G16_ERR_IO, "n_constraints exceeds what the constraint section can hold");
  {
    Cursor k(d, n, sec[2].pos);
    CsrOwned* M[3] = {&R->A, &R->B, &R->C};
    for (auto* m : M) {
      m->rowptr.assign(1, 0);
      m->rowptr.reserve((size_t)H.n_constraints + 1);
    }
    for (uint32_t i = 0; i < H.n_constraints; ++i) {
      for (auto* m : M) {
        const uint32_t cnt = k.u32();
        if (!k.ok) return fail(G16_ERR_IO, "unexpected end of file");
        for (uint32_t j = 0; j < cnt; ++j) {
          const uint32_t wire = k.u32();
          const uint8_t* v = k.bytes(32);
          if (!v) return fail(G16_ERR_IO, "unexpected end of file");
          // F::deserialize_uncompressed rejects non-canonical values
          if (!fr_lt_modulus(v)) return fail(G16_ERR_IO, "invalid field element (>= modulus)");
          U256 u;
          memcpy(u.v, v, 32);
          m->col.push_back(wire);
          m->val.push_back(Fr::from_canonical(u));
        }
        m->rowptr.push_back((uint32_t)m->col.size());
      }
    }
  }
  if (!sec.count(3)) return fail(G16_ERR_IO, "No section offset for wire2label type found");
  {
    if (sec[3].size != (uint64_t)H.n_wires * 8) return fail(G16_ERR_IO, "Invalid map section size");
    Cursor w(d, n, sec[3].pos);
    R->wire_mapping.resize(H.n_wires);
    for (uint32_t i = 0; i < H.n_wires; ++i) R->wire_mapping[i] = w.u64();
    if (!w.ok) return fail(G16_ERR_IO, "unexpected end of file");
    if (H.n_wires == 0 || R->wire_mapping[0] != 0)
      return fail(G16_ERR_IO, "Wire 0 should always be mapped to 0");
  }
  H.num_inputs = 1 + H.n_pub_in + H.n_pub_out;
  H.num_variables = H.n_wires;
  H.num_aux = H.num_variables - H.num_inputs;
  return G16_OK;
}

// the container walk and header rules of a .wtns: where the nw canonical values of section 2 start
g16_status wtns_locate(const uint8_t* d, size_t n, size_t* values_pos, uint32_t* cnt) {
  Cursor c(d, n);
  const uint8_t* magic = c.bytes(4);
  if (!magic || memcmp(magic, "wtns", 4) != 0) return fail(G16_ERR_IO, "wtns: bad magic");
  (void)c.u32();
  const uint32_t nsec = c.u32();
  std::map<uint32_t, Section> sec;
  for (uint32_t i = 0; i < nsec; ++i) {
    const uint32_t ty = c.u32();
    const uint64_t sz = c.u64();
    if (!c.ok) return fail(G16_ERR_IO, "wtns: truncated");
    sec[ty] = Section{c.o, sz};
    c.skip(sz);
    if (!c.ok) return fail(G16_ERR_IO, "wtns: truncated");
  }
  if (!sec.count(1) || !sec.count(2)) return fail(G16_ERR_IO, "wtns: missing section");
  Cursor h(d, n, sec[1].pos);
  const uint32_t n8 = h.u32();
  if (!h.ok || n8 != 32) return fail(G16_ERR_IO, "wtns: only 32-byte fields are supported");
  const uint8_t* prime = h.bytes(32);
  if (!prime || memcmp(prime, kR1csPrime, 32) != 0) return fail(G16_ERR_IO, "wtns: not bn128");
  const uint32_t nw = h.u32();
  if (!h.ok || sec[2].size < (uint64_t)nw * 32) return fail(G16_ERR_IO, "wtns: truncated values");
  *values_pos = sec[2].pos;
  *cnt = nw;
  return G16_OK;
}

g16_status wtns_parse(const uint8_t* d, size_t n, uint64_t** out, uint32_t* cnt) {
  size_t pos = 0;
  uint32_t nw = 0;
  const g16_status st = wtns_locate(d, n, &pos, &nw);
  if (st != G16_OK) return st;
  Cursor v(d, n, pos);
  uint64_t* buf = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 32);
  if (!buf) return fail(G16_ERR_INTERNAL, "out of memory");
  for (uint32_t i = 0; i < nw; ++i) {
    const uint8_t* b = v.bytes(32);
    if (!b || !fr_lt_modulus(b)) {
      free(buf);
      return fail(G16_ERR_IO, "wtns: invalid field element");
    }
    U256 u;
    memcpy(u.v, b, 32);
    Fr m = Fr::from_canonical(u);
    memcpy(buf + (size_t)i * 4, m.v, 32);
  }
  *out = buf;
  *cnt = nw;
  return G16_OK;
}

}  // namespace

extern "C" {

const char* g16_loader_last_error(void) { return t_err.c_str(); }

g16_status g16_zkey_open_mem(const uint8_t* data, size_t len, g16_zkey** out) {
  if (!data || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_zkey> z(new g16_zkey());
    z->data.copy_of(data, len);
    const g16_status st = zkey_parse(z.get());
    if (st != G16_OK) return st;
    *out = z.release();
    return G16_OK;
  });
}

g16_status g16_zkey_open(const char* path, g16_zkey** out) {
  if (!path || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_zkey> z(new g16_zkey());
    std::string err;
    if (!z->data.map_file(path, err)) return fail(G16_ERR_IO, err);
    const g16_status st = zkey_parse(z.get());
    if (st != G16_OK) return st;
    *out = z.release();
    return G16_OK;
  });
}

void g16_zkey_close(g16_zkey* z) { delete z; }

g16_status g16_zkey_header_get(const g16_zkey* z, g16_zkey_header* out) {
  if (!z || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = z->hdr;
  return G16_OK;
}

g16_status g16_zkey_key(const g16_zkey* z, g16_key_desc* out) {
  if (!z || !out) return fail(G16_ERR_INVALID, "null argument");
  const uint8_t* d = z->data.data();
  memset(out, 0, sizeof *out);
  out->n_vars = z->hdr.n_vars;
  out->n_public = z->hdr.n_public;
  out->domain_size = z->hdr.domain_size;
  out->a_query = d + z->sec.at(5).pos;
  out->b_g1_query = d + z->sec.at(6).pos;
  out->b_g2_query = d + z->sec.at(7).pos;
  out->l_query = d + z->sec.at(8).pos;
  out->h_query = d + z->sec.at(9).pos;
  memcpy(out->alpha_g1, z->hdr.alpha_g1, 64);
  memcpy(out->beta_g1, z->hdr.beta_g1, 64);
  memcpy(out->delta_g1, z->hdr.delta_g1, 64);
  memcpy(out->beta_g2, z->hdr.beta_g2, 128);
  memcpy(out->delta_g2, z->hdr.delta_g2, 128);
  return G16_OK;
}

const uint8_t* g16_zkey_ic(const g16_zkey* z, uint32_t* count) {
  if (!z) return nullptr;
  if (count) *count = z->hdr.n_public + 1;
  return z->data.data() + z->sec.at(3).pos;
}

static g16_status zkey_matrices_body(g16_zkey* z, g16_matrices* out);

g16_status g16_zkey_matrices(g16_zkey* z, g16_matrices* out) {
  if (!z || !out) return fail(G16_ERR_INVALID, "null argument");
  return guarded([&] { return zkey_matrices_body(z, out); });
}

static g16_status zkey_matrices_body(g16_zkey* z, g16_matrices* out) {
  if (!z->have_matrices) {
    // BinFile::matrices (zkey.rs:151-196)
    const uint8_t* d = z->data.data();
    const Section s4 = z->sec.at(4);
    Cursor c(d, s4.pos + (size_t)s4.size <= z->data.size() ? s4.pos + (size_t)s4.size : z->data.size(),
             s4.pos);
    const uint32_t ncoef = c.u32();
    if (!c.ok) return fail(G16_ERR_IO, "zkey: truncated coefficient section");
    const uint8_t* recs = c.bytes((size_t)ncoef * 44);
    if (!recs) return fail(G16_ERR_IO, "zkey: truncated coefficient section");
    const uint32_t dom = z->hdr.domain_size;
    uint32_t max_c = 0;
    std::vector<uint32_t> cnt[2];
    cnt[0].assign((size_t)dom + 1, 0);
    cnt[1].assign((size_t)dom + 1, 0);
    for (uint32_t i = 0; i < ncoef; ++i) {
      uint32_t m, row;
      memcpy(&m, recs + (size_t)i * 44, 4);
      memcpy(&row, recs + (size_t)i * 44 + 4, 4);
      if (m > 1) return fail(G16_ERR_IO, "zkey: coefficient with matrix index > 1");
      if (row >= dom) return fail(G16_ERR_IO, "zkey: coefficient row outside the domain");
      if (row > max_c) max_c = row;
      cnt[m][row + 1]++;
    }
    if (max_c < z->hdr.n_public) return fail(G16_ERR_IO, "zkey: fewer rows than public inputs");
    const uint32_t nc = max_c - z->hdr.n_public;  // :171
    CsrOwned* M[2] = {&z->A, &z->B};
    std::vector<uint32_t> cur[2];
    for (int k = 0; k < 2; ++k) {
      // rows >= nc are dropped (truncate, :173-175): arkworks re-adds the public-input rows
      M[k]->rowptr.assign((size_t)nc + 1, 0);
      for (uint32_t r = 0; r < nc; ++r) M[k]->rowptr[r + 1] = M[k]->rowptr[r] + cnt[k][r + 1];
      M[k]->col.resize(M[k]->rowptr[nc]);
      M[k]->val.resize(M[k]->rowptr[nc]);
      cur[k].assign(M[k]->rowptr.begin(), M[k]->rowptr.end());
    }
    for (uint32_t i = 0; i < ncoef; ++i) {  // stable: file order inside a row, like the push()
      const uint8_t* rec = recs + (size_t)i * 44;
      uint32_t m, row, sig;
      memcpy(&m, rec, 4);
      memcpy(&row, rec + 4, 4);
      memcpy(&sig, rec + 8, 4);
      if (row >= nc) continue;
      // the reference indexes full_assignment[signal] (evaluate_constraint) and panics out of
      // bounds; the kernels would read past the witness, so a bad wire index is a load error here
      if (sig >= z->hdr.n_vars) return fail(G16_ERR_IO, "zkey: coefficient signal index >= n_vars");
      const uint32_t at = cur[m][row]++;
      M[m]->col[at] = sig;
      // deserialize_field_fr (:322-325): the stored value is v*R^2; one Montgomery reduction
      // leaves v*R, the in-memory Montgomery form of v
      U256 u = fr_load(rec + 12).to_canonical();
      Fr v;
      memcpy(v.v, u.v, 32);
      M[m]->val[at] = v;
    }
    g16_matrices& mt = z->mat;
    mt.num_instance_variables = z->hdr.n_public + 1;              // :182
    mt.num_witness_variables = z->hdr.n_vars - z->hdr.n_public;   // :183
    mt.num_constraints = nc;
    mt.a_num_non_zero = z->A.col.size();
    mt.b_num_non_zero = z->B.col.size();
    mt.a = z->A.view();
    mt.b = z->B.view();
    z->have_matrices = true;
  }
  *out = z->mat;
  return G16_OK;
}

g16_status g16_ptau_open_mem(const uint8_t* data, size_t len, g16_ptau** out) {
  if (!data || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_ptau> z(new g16_ptau());
    z->data.copy_of(data, len);
    const g16_status st = ptau_parse(z.get());
    if (st != G16_OK) return st;
    *out = z.release();
    return G16_OK;
  });
}

g16_status g16_ptau_open(const char* path, g16_ptau** out) {
  if (!path || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_ptau> z(new g16_ptau());
    std::string err;
    if (!z->data.map_file(path, err)) return fail(G16_ERR_IO, err);
    const g16_status st = ptau_parse(z.get());
    if (st != G16_OK) return st;
    *out = z.release();
    return G16_OK;
  });
}

void g16_ptau_close(g16_ptau* p) { delete p; }

g16_status g16_ptau_header_get(const g16_ptau* p, g16_ptau_header* out) {
  if (!p || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = p->hdr;
  return G16_OK;
}

g16_status g16_ptau_srs(const g16_ptau* p, g16_srs_desc* out) {
  if (!p || !out) return fail(G16_ERR_INVALID, "null argument");
  const uint8_t* d = p->data.data();
  const uint32_t n = 1u << p->hdr.power;
  memset(out, 0, sizeof *out);
  out->n_tau_g1 = 2 * n - 1;
  out->n_tau = n;
  out->tau_g1 = d + p->sec.at(2).pos;
  out->tau_g2 = d + p->sec.at(3).pos;
  out->alpha_tau_g1 = d + p->sec.at(4).pos;
  out->beta_tau_g1 = d + p->sec.at(5).pos;
  memcpy(out->beta_g2, d + p->sec.at(6).pos, 128);
  return G16_OK;
}

static g16_status ptau_lagrange_body(const g16_ptau* p, g16_srs_lagrange_desc* out);

g16_status g16_ptau_lagrange(const g16_ptau* p, g16_srs_lagrange_desc* out) {
  if (!p || !out) return fail(G16_ERR_INVALID, "null argument");
  return guarded([&] { return ptau_lagrange_body(p, out); });
}

static g16_status ptau_lagrange_body(const g16_ptau* p, g16_srs_lagrange_desc* out) {
  memset(out, 0, sizeof *out);
  const uint32_t power = p->hdr.power;
  if (power > 27) return fail(G16_ERR_IO, "ptau: Lagrange sections of power " + std::to_string(power) + " > 27");
  for (uint32_t id : {12u, 13u, 14u, 15u}) {
    const auto it = p->sec.find(id);
    if (it == p->sec.end())
      return fail(G16_ERR_IO, "ptau: missing section " + std::to_string(id) + ": the file is not prepared");
    if (it->second.size != ptau_section_bytes(id, power))
      return fail(G16_ERR_IO, "ptau: section " + std::to_string(id) + " has " + std::to_string(it->second.size) +
                                  " bytes, power " + std::to_string(power) + " needs " +
                                  std::to_string(ptau_section_bytes(id, power)));
  }
  const uint8_t* d = p->data.data();
  out->power = power;
  out->tau_g1 = d + p->sec.at(12).pos;
  out->tau_g2 = d + p->sec.at(13).pos;
  out->alpha_tau_g1 = d + p->sec.at(14).pos;
  out->beta_tau_g1 = d + p->sec.at(15).pos;
  return G16_OK;
}

static g16_status ptau_write_impl(const char* path, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                  uint32_t power);

g16_status g16_ptau_write(const char* path, const g16_srs_desc* srs, uint32_t power) {
  return guarded([&] { return ptau_write_impl(path, srs, nullptr, power); });
}

g16_status g16_ptau_write_prepared(const char* path, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                   uint32_t power) {
  if (!lag || !lag->tau_g1 || !lag->tau_g2 || !lag->alpha_tau_g1 || !lag->beta_tau_g1)
    return fail(G16_ERR_INVALID, "null argument");
  if (power > 27) return fail(G16_ERR_INVALID, "ptau: Lagrange sections need power <= 27");
  if (lag->power != power) return fail(G16_ERR_INVALID, "ptau: the Lagrange set is not of this power");
  return guarded([&] { return ptau_write_impl(path, srs, lag, power); });
}

static g16_status ptau_write_impl(const char* path, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                  uint32_t power) {
  if (!path || !srs || !srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1)
    return fail(G16_ERR_INVALID, "null argument");
  if (power > kPtauMaxPower) return fail(G16_ERR_INVALID, "ptau: power > 28");
  const uint64_t n = (uint64_t)1 << power;
  if (srs->n_tau_g1 < 2 * n - 1 || srs->n_tau < n) return fail(G16_ERR_INVALID, "ptau: the SRS is shorter than 2^power");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(G16_ERR_IO, std::string("cannot create ") + path);
  bool ok = true;
  auto put = [&](const void* p, size_t k) { ok = ok && (k == 0 || fwrite(p, 1, k, f) == k); };
  auto u32 = [&](uint32_t v) { put(&v, 4); };
  auto sec = [&](uint32_t id, const void* p) {
    const uint64_t len = ptau_section_bytes(id, power);
    u32(id);
    put(&len, 8);
    put(p, (size_t)len);
  };
  put("ptau", 4);
  u32(1);
  u32(lag ? 11 : 7);
  const uint64_t len1 = 4 + 32 + 4 + 4, len7 = 4;
  u32(1);
  put(&len1, 8);
  u32(32);
  put(g16::FqParams::MOD, 32);
  u32(power);
  u32(power);
  sec(2, srs->tau_g1);
  sec(3, srs->tau_g2);
  sec(4, srs->alpha_tau_g1);
  sec(5, srs->beta_tau_g1);
  sec(6, srs->beta_g2);
  u32(7);
  put(&len7, 8);
  u32(0);  // no contributions recorded
  if (lag) {
    sec(12, lag->tau_g1);
    sec(13, lag->tau_g2);
    sec(14, lag->alpha_tau_g1);
    sec(15, lag->beta_tau_g1);
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? G16_OK : fail(G16_ERR_IO, "short write");
}

g16_status g16_r1cs_open_mem(const uint8_t* data, size_t len, g16_r1cs** out) {
  if (!data || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_r1cs> r(new g16_r1cs());
    const g16_status st = r1cs_parse(data, len, r.get());
    if (st != G16_OK) return st;
    *out = r.release();
    return G16_OK;
  });
}

g16_status g16_r1cs_open(const char* path, g16_r1cs** out) {
  if (!path || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::vector<uint8_t> buf;
    std::string err;
    if (!read_file(path, buf, err)) return fail(G16_ERR_IO, err);
    if (buf.empty()) return fail(G16_ERR_IO, "Invalid magic number");  // no data() of an empty vector downstream
    return g16_r1cs_open_mem(buf.data(), buf.size(), out);
  });
}

void g16_r1cs_close(g16_r1cs* r) { delete r; }

g16_status g16_r1cs_header_get(const g16_r1cs* r, g16_r1cs_header* out) {
  if (!r || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = r->hdr;
  return G16_OK;
}

g16_status g16_r1cs_matrices(const g16_r1cs* r, g16_csr* a, g16_csr* b, g16_csr* c) {
  if (!r) return fail(G16_ERR_INVALID, "null argument");
  if (a) *a = r->A.view();
  if (b) *b = r->B.view();
  if (c) *c = r->C.view();
  return G16_OK;
}

const uint64_t* g16_r1cs_wire_mapping(const g16_r1cs* r, uint32_t* count) {
  if (!r) return nullptr;
  if (count) *count = (uint32_t)r->wire_mapping.size();
  return r->wire_mapping.data();
}

g16_status g16_wtns_read_mem(const uint8_t* data, size_t len, uint64_t** out, uint32_t* n) {
  if (!data || !out || !n) return fail(G16_ERR_INVALID, "null argument");
  return guarded([&] { return wtns_parse(data, len, out, n); });
}

g16_status g16_wtns_read(const char* path, uint64_t** out, uint32_t* n) {
  if (!path || !out || !n) return fail(G16_ERR_INVALID, "null argument");
  return guarded([&]() -> g16_status {
    std::vector<uint8_t> buf;
    std::string err;
    if (!read_file(path, buf, err)) return fail(G16_ERR_IO, err);
    return wtns_parse(buf.data(), buf.size(), out, n);
  });
}

// .wtns as it lies in the file: the header is checked, the values are handed out where they are (the device
// converts and range-tests them: g16_prove_canonical)
struct g16_wtns {
  FileView data;
  size_t pos = 0;
  uint32_t n = 0;
};

static g16_status wtns_open_view(std::unique_ptr<g16_wtns>& w, g16_wtns** out) {
  const g16_status st = wtns_locate(w->data.data(), w->data.size(), &w->pos, &w->n);
  if (st != G16_OK) return st;
  *out = w.release();
  return G16_OK;
}

g16_status g16_wtns_open(const char* path, g16_wtns** out) {
  if (!path || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_wtns> w(new g16_wtns());
    std::string err;
    if (!w->data.map_file(path, err)) return fail(G16_ERR_IO, err);
    return wtns_open_view(w, out);
  });
}

g16_status g16_wtns_open_mem(const uint8_t* data, size_t len, g16_wtns** out) {
  if (!data || !out) return fail(G16_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() -> g16_status {
    std::unique_ptr<g16_wtns> w(new g16_wtns());
    w->data.copy_of(data, len);
    return wtns_open_view(w, out);
  });
}

uint32_t g16_wtns_count(const g16_wtns* w) { return w ? w->n : 0; }

const uint8_t* g16_wtns_values(const g16_wtns* w) { return w ? w->data.data() + w->pos : nullptr; }

void g16_wtns_close(g16_wtns* w) { delete w; }

void g16_free(void* p) { free(p); }

/* snarkjs .zkey writer (format: SURVEY.md Appendix A.2 = what read_zkey parses, reference
 * src/zkey.rs:1-27,73-133,151-196,288-368).  Coefs(4) values are stored as v * R^2 (the reader
 * divides by R^2, zkey.rs:320-325), points in the Montgomery encoding the key arrays already have;
 * the n_public + 1 rows snarkjs appends (row m+i: A coefficient 1 on signal i) are written too.    */
g16_status g16_zkey_write(const char* path, const g16_key_desc* key, const uint8_t* ic,
                          const uint8_t gamma_g2[128], const g16_csr* a, const g16_csr* b,
                          uint32_t num_constraints) {
  if (!path || !key || !ic || !gamma_g2 || !a || !b) return fail(G16_ERR_INVALID, "null argument");
  // the descriptor is checked before the file is created: every length below is derived from it
  if ((uint64_t)key->n_vars < (uint64_t)key->n_public + 1) return fail(G16_ERR_INVALID, "zkey: n_vars < n_public + 1");
  const uint64_t n_l = (uint64_t)key->n_vars - key->n_public - 1;
  if ((key->n_vars && (!key->a_query || !key->b_g1_query || !key->b_g2_query)) || (n_l && !key->l_query) ||
      (key->domain_size && !key->h_query))
    return fail(G16_ERR_INVALID, "zkey: a query array is NULL but its count is not zero");
  for (const g16_csr* m : {a, b}) {
    if (!m->row_ptr || (m->nnz && (!m->col || !m->coeff))) return fail(G16_ERR_INVALID, "zkey: matrix with null arrays");
    if (m->row_ptr[0] != 0 || m->row_ptr[num_constraints] != m->nnz)
      return fail(G16_ERR_INVALID, "zkey: matrix row_ptr does not span [0, nnz]");
    for (uint32_t i = 0; i < num_constraints; ++i)
      if (m->row_ptr[i] > m->row_ptr[i + 1]) return fail(G16_ERR_INVALID, "zkey: matrix row_ptr is not monotone");
  }
  if (a->nnz > UINT32_MAX || b->nnz > UINT32_MAX || a->nnz + b->nnz + key->n_public + 1 > UINT32_MAX)
    return fail(G16_ERR_INVALID, "zkey: the coefficient count does not fit in 32 bits");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(G16_ERR_IO, std::string("cannot create ") + path);
  bool ok = true;
  auto put = [&](const void* p, size_t n) { ok = ok && (n == 0 || fwrite(p, 1, n, f) == n); };
  auto u32 = [&](uint32_t v) { put(&v, 4); };
  auto u64 = [&](uint64_t v) { put(&v, 8); };
  auto sec = [&](uint32_t id, uint64_t len) {
    u32(id);
    u64(len);
  };
  const uint32_t N = key->n_vars, p = key->n_public;
  const uint64_t ncoef = a->nnz + b->nnz + p + 1;
  put("zkey", 4);
  u32(1);
  u32(10);
  sec(1, 4);
  u32(1);  // groth16
  sec(2, 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128);
  u32(32);
  put(g16::FqParams::MOD, 32);
  u32(32);
  put(g16::FrParams::MOD, 32);
  u32(N);
  u32(p);
  u32(key->domain_size);
  put(key->alpha_g1, 64);
  put(key->beta_g1, 64);
  put(key->beta_g2, 128);
  put(gamma_g2, 128);
  put(key->delta_g1, 64);
  put(key->delta_g2, 128);
  sec(3, (uint64_t)(p + 1) * 64);
  put(ic, (size_t)(p + 1) * 64);
  sec(4, 4 + ncoef * (12 + 32));
  u32((uint32_t)ncoef);
  const Fr r2 = Fr::r2();
  auto coefs = [&](uint32_t which, const g16_csr* m) {
    for (uint32_t row = 0; row < num_constraints; ++row)
      for (uint32_t j = m->row_ptr[row]; j < m->row_ptr[row + 1]; ++j) {
        u32(which);
        u32(row);
        u32(m->col[j]);
        Fr v;
        memcpy(v.v, m->coeff + (size_t)j * 4, 32);
        // v holds the limbs of coeff * R; the Montgomery product with R^2 is (coeff R)(R^2)/R =
        // coeff * R^2 mod r: exactly the integer snarkjs stores
        const Fr vr = v * r2;
        put(vr.v, 32);
      }
  };
  coefs(0, a);
  coefs(1, b);
  for (uint32_t i = 0; i <= p; ++i) {
    u32(0);
    u32(num_constraints + i);
    u32(i);
    const Fr one_r2 = Fr::one() * r2;  // 1 * R^2
    put(one_r2.v, 32);
  }
  sec(5, (uint64_t)N * 64);
  put(key->a_query, (size_t)N * 64);
  sec(6, (uint64_t)N * 64);
  put(key->b_g1_query, (size_t)N * 64);
  sec(7, (uint64_t)N * 128);
  put(key->b_g2_query, (size_t)N * 128);
  sec(8, (uint64_t)(N - p - 1) * 64);
  put(key->l_query, (size_t)(N - p - 1) * 64);
  sec(9, (uint64_t)key->domain_size * 64);
  put(key->h_query, (size_t)key->domain_size * 64);
  sec(10, 4 + 64);
  u32(0);
  uint8_t zeros[64] = {0};
  put(zeros, 64);
  ok = (fclose(f) == 0) && ok;
  return ok ? G16_OK : fail(G16_ERR_IO, "short write");
}

g16_status g16_fr_from_canonical(const uint8_t* in, uint64_t* out, size_t n) {
  if (!in || !out) return fail(G16_ERR_INVALID, "null argument");
  for (size_t i = 0; i < n; ++i) {
    if (!fr_lt_modulus(in + i * 32)) return fail(G16_ERR_INVALID, "value >= field modulus");
    U256 u;
    memcpy(u.v, in + i * 32, 32);
    Fr m = Fr::from_canonical(u);
    memcpy(out + i * 4, m.v, 32);
  }
  return G16_OK;
}

g16_status g16_fr_to_canonical(const uint64_t* in, uint8_t* out, size_t n) {
  if (!in || !out) return fail(G16_ERR_INVALID, "null argument");
  for (size_t i = 0; i < n; ++i) {
    Fr m;
    memcpy(m.v, in + i * 4, 32);
    U256 u = m.to_canonical();
    memcpy(out + i * 32, u.v, 32);
  }
  return G16_OK;
}

// ---- arkworks containers: the layout walk (g16_loaders.h) ---------------------------------------
// Untrusted bytes: every step is checked against what is left of the blob BEFORE it is taken, in u64
// arithmetic that cannot wrap (count <= left / record size).
namespace {

const char* const kArkField[G16_ARK_N_FIELDS] = {"vk.alpha_g1", "vk.beta_g2", "vk.gamma_g2", "vk.delta_g2",
                                                 "vk.gamma_abc_g1", "beta_g1", "delta_g1", "a_query",
                                                 "b_g1_query", "b_g2_query", "h_query", "l_query"};

struct ArkWalk {
  const uint8_t* data;
  uint64_t len, at = 0;
  uint64_t g1, g2;
  g16_ark_layout* lay;
  std::string err;

  bool single(int f, bool is_g2) {
    const uint64_t rec = is_g2 ? g2 : g1;
    if (len - at < rec) {
      err = std::string("truncated in ") + kArkField[f];
      return false;
    }
    lay->offset[f] = at;
    lay->count[f] = 1;
    at += rec;
    return true;
  }
  bool vec(int f, bool is_g2) {
    const uint64_t rec = is_g2 ? g2 : g1;
    if (len - at < 8) {
      err = std::string("truncated in the length of ") + kArkField[f];
      return false;
    }
    uint64_t n;
    memcpy(&n, data + at, 8);
    at += 8;
    if (n > (len - at) / rec) {
      err = std::string("the length of ") + kArkField[f] + " (" + std::to_string(n) + ") overruns the blob";
      return false;
    }
    lay->offset[f] = at;
    lay->count[f] = n;
    at += n * rec;
    return true;
  }
  bool vk() {
    return single(G16_ARK_F_ALPHA_G1, false) && single(G16_ARK_F_BETA_G2, true) && single(G16_ARK_F_GAMMA_G2, true) &&
           single(G16_ARK_F_DELTA_G2, true) && vec(G16_ARK_F_IC, false);
  }
  bool check_vk() {
    if (lay->count[G16_ARK_F_IC] < 1 || lay->count[G16_ARK_F_IC] > (1ull << 31)) {
      err = "vk.gamma_abc_g1 must hold between 1 and 2^31 points";
      return false;
    }
    return true;
  }
  bool end() {
    if (at != len) {
      err = std::to_string(len - at) + " trailing byte(s)";
      return false;
    }
    lay->total = at;
    return true;
  }
};

g16_status ark_layout(const uint8_t* data, size_t len, uint32_t flags, g16_ark_layout* out, bool pk) {
  if (!out || (len && !data)) return fail(G16_ERR_INVALID, "null argument");
  memset(out, 0, sizeof *out);
  const bool comp = (flags & G16_ARK_COMPRESSED) != 0;
  ArkWalk w{data, (uint64_t)len, 0, comp ? 32u : 64u, comp ? 64u : 128u, out, {}};
  bool ok = w.vk() && w.check_vk();
  if (ok && pk) {
    ok = w.single(G16_ARK_F_BETA_G1, false) && w.single(G16_ARK_F_DELTA_G1, false) && w.vec(G16_ARK_F_A, false) &&
         w.vec(G16_ARK_F_B1, false) && w.vec(G16_ARK_F_B2, true) && w.vec(G16_ARK_F_H, false) && w.vec(G16_ARK_F_L, false);
    if (ok) {
      const uint64_t N = out->count[G16_ARK_F_A], n_ic = out->count[G16_ARK_F_IC];
      if (out->count[G16_ARK_F_B1] != N || out->count[G16_ARK_F_B2] != N) {
        w.err = "len(b_g1_query) and len(b_g2_query) must equal len(a_query)";
        ok = false;
      } else if (N < n_ic || out->count[G16_ARK_F_L] != N - n_ic) {
        w.err = "len(l_query) must equal len(a_query) - len(vk.gamma_abc_g1)";
        ok = false;
      } else if (N > (1ull << 31) || out->count[G16_ARK_F_H] > (1ull << 31)) {
        w.err = "more than 2^31 points in a query";
        ok = false;
      }
    }
  }
  ok = ok && w.end();
  if (!ok) {
    memset(out, 0, sizeof *out);
    return fail(G16_ERR_IO, std::string(pk ? "ark ProvingKey: " : "ark VerifyingKey: ") + w.err);
  }
  return G16_OK;
}

}  // namespace

g16_status g16_ark_pk_layout(const uint8_t* data, size_t len, uint32_t flags, g16_ark_layout* out) {
  return guarded([&] { return ark_layout(data, len, flags, out, true); });
}
g16_status g16_ark_vk_layout(const uint8_t* data, size_t len, uint32_t flags, g16_ark_layout* out) {
  return guarded([&] { return ark_layout(data, len, flags, out, false); });
}

}  // extern "C"

namespace g16 {
// arkser.hip: its container calls report through g16_loader_last_error, with the one table of field names
g16_status loader_fail(g16_status code, const std::string& message) { return fail(code, message); }
const char* ark_field_name(int field) { return field >= 0 && field < G16_ARK_N_FIELDS ? kArkField[field] : "?"; }
}  // namespace g16
