/* g16_loaders.h -- host-side (C++) loaders for the circom/snarkjs binary formats, exported over
 * the same C ABI.  They mirror the reference's loaders value-for-value and error-for-error:
 *   g16_zkey_*  <- read_zkey / BinFile (reference src/zkey.rs:53-60,73-133,151-196,288-368)
 *   g16_r1cs_*  <- R1CSFile::new + R1CS::from (reference src/circom/r1cs_reader.rs:26-39,54-249)
 *   g16_wtns_*  <- snarkjs .wtns (not parsed by the reference)
 *   g16_ptau_*  <- snarkjs .ptau (not parsed by the reference)
 * but hand back GPU-ready packed arrays (the on-disk point encoding IS the device encoding) from
 * one bulk read instead of one Read call per 32-byte field (src/zkey.rs:328-368).
 * All returned pointers are owned by the handle and stay valid until *_close.
 * The files are untrusted: every count a header states is checked against the section that has to hold it before
 * anything is reserved for it, and no C++ exception leaves these functions -- an allocation that fails comes back
 * as G16_ERR_INTERNAL ("out of memory"), the half-built handle is freed and *out stays NULL
 * (tests/loaders/loaders_main.cpp walks the truncations and mutations).                              */
#ifndef G16_LOADERS_H
#define G16_LOADERS_H

#include "g16_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* g16_loader_last_error(void); /* thread-local message of the last failed loader call */

/* ---------------------------------------------------------------- .zkey ---------------------- */
typedef struct g16_zkey g16_zkey;

typedef struct {                 /* HeaderGroth (src/zkey.rs:270-317) */
  uint32_t n8q, n8r;
  uint8_t q[32], r[32];          /* little-endian */
  uint32_t n_vars, n_public, domain_size, power;
  uint8_t alpha_g1[64], beta_g1[64], beta_g2[128], gamma_g2[128], delta_g1[64], delta_g2[128];
} g16_zkey_header;

typedef struct {                 /* ConstraintMatrices as built by BinFile::matrices (src/zkey.rs:151-196) */
  uint32_t num_instance_variables; /* n_public + 1              (:182) */
  uint32_t num_witness_variables;  /* n_vars - n_public         (:183) */
  uint32_t num_constraints;        /* max constraint - n_public (:171) */
  uint64_t a_num_non_zero, b_num_non_zero;
  g16_csr a, b;                    /* coefficients Montgomery (file value / R, :322-325) */
} g16_matrices;

/* g16_zkey_open maps the file (the key arrays handed to g16_ctx_create are views of the page cache):
 * the file must stay unchanged until g16_zkey_close -- a zkey truncated or rewritten underneath an
 * open handle faults (SIGBUS) instead of returning G16_ERR_IO.  G16_ZKEY_COPY=1 in the environment
 * reads it into owned memory instead (the behaviour of g16_zkey_open_mem).                        */
g16_status g16_zkey_open(const char* path, g16_zkey** out);
g16_status g16_zkey_open_mem(const uint8_t* data, size_t len, g16_zkey** out); /* data is copied */
void g16_zkey_close(g16_zkey* z);
g16_status g16_zkey_header_get(const g16_zkey* z, g16_zkey_header* out);
/* ProvingKey arrays (zero-copy views of sections 5..9) + header points */
g16_status g16_zkey_key(const g16_zkey* z, g16_key_desc* out);
/* vk.gamma_abc_g1 = IC, (n_public + 1) x 64 bytes (section 3) */
const uint8_t* g16_zkey_ic(const g16_zkey* z, uint32_t* count);
g16_status g16_zkey_matrices(g16_zkey* z, g16_matrices* out);

/* snarkjs-format .zkey WRITER: the inverse of g16_zkey_open for a key held in packed arrays (e.g.
 * one minted by g16_setup_create) -- lets synthetic circuits go through the same file format and
 * loader path as circom/snarkjs artefacts (reference format notes: src/zkey.rs:1-27).  ic:
 * (n_public + 1) x 64 bytes; a, b: ConstraintMatrices rows WITHOUT the n_public + 1 rows snarkjs
 * appends (they are generated).  G16_ERR_INVALID, before the file is created: n_vars < n_public + 1; a NULL
 * query array whose count is not zero; a or b with a NULL row_ptr, a row_ptr that does not run from 0 to nnz
 * monotonically over num_constraints rows, or NULL col / coeff with nnz > 0; more than 2^32 - 1 coefficients
 * (a's, b's and the appended rows together: the count field of section 4 is a u32).                        */
g16_status g16_zkey_write(const char* path, const g16_key_desc* key, const uint8_t* ic,
                          const uint8_t gamma_g2[128], const g16_csr* a, const g16_csr* b,
                          uint32_t num_constraints);

/* ---------------------------------------------------------------- .ptau ---------------------- */
/* snarkjs powers-of-tau files: the SRS g16_setup_from_srs / g16_srs_check take.  The binfile container of
 * .zkey: magic "ptau", version u32 = 1, nSections u32, then (id u32, size u64,
 * payload) in any order (the first occurrence of an id wins).
 *   1  n8 u32 (= 32), q[n8] little-endian (must be BN254 q), power u32, ceremony_power u32
 *   2  tauG1, 2 * 2^power - 1 G1 points      3  tauG2, 2^power G2 points
 *   4  alphaTauG1, 2^power G1 points          5  betaTauG1, 2^power G1 points        6  betaG2, one G2 point
 *   7  contributions: ignored on read, written as a zero count
 *   12..15  the Lagrange-form copies of a "prepared" file (`powersoftau prepare phase2`): tauG1 in levels
 *           0 .. power + 1 (4 * 2^power - 1 G1 points), tauG2, alphaTauG1, betaTauG1 in levels 0 .. power
 *           (2 * 2^power - 1 points each); the layout of a level is g16_amd.h's ("prepared powers of tau").
 *           g16_ptau_open and g16_ptau_srs ignore them whatever their size; g16_ptau_lagrange hands them out.
 * Points in the encoding of the rest of the ABI: 32-byte little-endian Montgomery coordinates, all-zero =
 * infinity.  THIS DESCRIPTION IS WRITTEN FROM KNOWLEDGE OF snarkjs: no .ptau file and no snarkjs were at hand to
 * pin it to, the reader is tested against this writer and against an independent encoding of the same
 * description only.
 * G16_ERR_IO with a message in g16_loader_last_error: wrong magic, version or prime; a section among 1..6
 * missing; a section size that does not match power; a truncated file; power > 28.
 * The points are handed out as they come: run g16_srs_check on them.  The section-7 transcript is NOT
 * verified.  g16_ptau_open maps the file under the rules of g16_zkey_open (the file must stay unchanged
 * until g16_ptau_close; G16_ZKEY_COPY=1 reads it into owned memory).                                      */
typedef struct g16_ptau g16_ptau;
typedef struct { uint32_t n8q; uint8_t q[32]; uint32_t power, ceremony_power; } g16_ptau_header;
g16_status g16_ptau_open(const char* path, g16_ptau** out);
g16_status g16_ptau_open_mem(const uint8_t* data, size_t len, g16_ptau** out); /* data is copied */
void g16_ptau_close(g16_ptau* p);
g16_status g16_ptau_header_get(const g16_ptau* p, g16_ptau_header* out);
/* zero-copy views of sections 2..6, owned by the handle */
g16_status g16_ptau_srs(const g16_ptau* p, g16_srs_desc* out);
/* writes sections 1..7 from an SRS with n_tau_g1 >= 2 * 2^power - 1 and n_tau >= 2^power (entries beyond are
 * dropped); ceremony_power = power                                                                       */
g16_status g16_ptau_write(const char* path, const g16_srs_desc* srs, uint32_t power);
/* zero-copy views of sections 12..15, owned by the handle.  G16_ERR_IO with a message: one of them is absent (the
 * file is not prepared), its size does not match the power, or power > 27.  The points are handed out as they
 * come: run g16_srs_lagrange_check on them.                                                              */
g16_status g16_ptau_lagrange(const g16_ptau* p, g16_srs_lagrange_desc* out);
/* g16_ptau_write plus sections 12..15 from a Lagrange set of exactly this power (power <= 27)           */
g16_status g16_ptau_write_prepared(const char* path, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                   uint32_t power);

/* ------------------------------------------------ arkworks containers: the layout walk -------- */
/* Where the fields of an ark-serialize'd ProvingKey<Bn254> / VerifyingKey<Bn254> lie (the format: g16_amd.h,
 * "arkworks serialization"; flags: G16_ARK_COMPRESSED decides the record sizes).  Pure host code over untrusted
 * bytes: nothing beyond data[len) is dereferenced, no point is looked at.  offset[f] is where the first point of
 * field f starts (behind the length prefix of a Vec), count[f] its points (1 for the single ones), total the
 * length the blob must have.  G16_ERR_IO with a message in g16_loader_last_error: a truncated blob; a length
 * prefix that overruns the blob or overflows; len(b_g1_query) or len(b_g2_query) != len(a_query),
 * len(gamma_abc_g1) < 1, len(l_query) != len(a_query) - len(gamma_abc_g1), len(h_query) > 2^31; trailing bytes.
 * g16_ark_vk_layout fills the first five fields and leaves the others zero.                                */
enum { G16_ARK_F_ALPHA_G1 = 0, G16_ARK_F_BETA_G2, G16_ARK_F_GAMMA_G2, G16_ARK_F_DELTA_G2, G16_ARK_F_IC,
       G16_ARK_F_BETA_G1, G16_ARK_F_DELTA_G1, G16_ARK_F_A, G16_ARK_F_B1, G16_ARK_F_B2, G16_ARK_F_H, G16_ARK_F_L,
       G16_ARK_N_FIELDS };
typedef struct {
  uint64_t offset[G16_ARK_N_FIELDS];
  uint64_t count[G16_ARK_N_FIELDS];
  uint64_t total;
} g16_ark_layout;
g16_status g16_ark_pk_layout(const uint8_t* data, size_t len, uint32_t flags, g16_ark_layout* out);
g16_status g16_ark_vk_layout(const uint8_t* data, size_t len, uint32_t flags, g16_ark_layout* out);

/* ---------------------------------------------------------------- .r1cs ---------------------- */
typedef struct g16_r1cs g16_r1cs;

typedef struct {
  uint32_t version;
  uint32_t field_size;
  uint8_t prime[32];
  uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in;
  uint64_t n_labels;
  uint32_t n_constraints;
  /* R1CS::from (r1cs_reader.rs:26-39) */
  uint32_t num_inputs, num_aux, num_variables;
} g16_r1cs_header;

/* G16_ERR_IO beyond the reference's own errors: n_constraints > size of section 2 / 12 (a constraint is at least
 * its three term counts); 1 + n_pub_in + n_pub_out > n_wires, compared in 64 bits (num_inputs and num_aux
 * would wrap).  A wire index is NOT compared with n_wires here, as in the reference: g16_ctx_create and the
 * setup entry points refuse a matrix that names a wire or a constraint out of range.                     */
g16_status g16_r1cs_open(const char* path, g16_r1cs** out);
g16_status g16_r1cs_open_mem(const uint8_t* data, size_t len, g16_r1cs** out);
void g16_r1cs_close(g16_r1cs* r);
g16_status g16_r1cs_header_get(const g16_r1cs* r, g16_r1cs_header* out);
/* the three linear-combination lists per constraint as CSR (column = wire index, coefficient
 * Montgomery, as F::deserialize_uncompressed leaves it in memory, r1cs_reader.rs:203-213) */
g16_status g16_r1cs_matrices(const g16_r1cs* r, g16_csr* a, g16_csr* b, g16_csr* c);
const uint64_t* g16_r1cs_wire_mapping(const g16_r1cs* r, uint32_t* count);

/* ---------------------------------------------------------------- .wtns ---------------------- */
/* Reads n witness values; *out (malloc'd, free with g16_free) holds n x 4 u64 Montgomery Fr.      */
g16_status g16_wtns_read(const char* path, uint64_t** out, uint32_t* n);
g16_status g16_wtns_read_mem(const uint8_t* data, size_t len, uint64_t** out, uint32_t* n);
void g16_free(void* p);

/* The same file left as it is: the header is checked by the rules and with the messages of g16_wtns_read (magic,
 * 32-byte fields, the bn128 prime, a section 2 of at least n x 32 bytes), and the n canonical little-endian values
 * are handed out where they lie -- no conversion, no copy and NO RANGE TEST here: g16_prove_canonical /
 * g16_witness_upload_canonical / g16_fr_convert (g16_amd.h) convert them on the device and reject a value >= r
 * there.  g16_wtns_open maps the file read-only under the rules of g16_zkey_open (it must stay unchanged until
 * g16_wtns_close; G16_ZKEY_COPY=1 reads it into owned memory); g16_wtns_open_mem copies the caller's buffer.
 * g16_wtns_values: n x 32 bytes owned by the handle; the pointer is only 4-byte aligned in the file.             */
typedef struct g16_wtns g16_wtns;
g16_status g16_wtns_open(const char* path, g16_wtns** out);
g16_status g16_wtns_open_mem(const uint8_t* data, size_t len, g16_wtns** out);
uint32_t g16_wtns_count(const g16_wtns* w);
const uint8_t* g16_wtns_values(const g16_wtns* w);
void g16_wtns_close(g16_wtns* w);

/* canonical little-endian 32-byte integers <-> Montgomery Fr (host helpers for callers that hold
 * decimal / canonical witnesses, e.g. snarkjs JSON)                                               */
g16_status g16_fr_from_canonical(const uint8_t* in, uint64_t* out, size_t n);
g16_status g16_fr_to_canonical(const uint64_t* in, uint8_t* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* G16_LOADERS_H */
