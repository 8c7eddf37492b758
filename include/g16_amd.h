/* g16_amd.h -- C ABI of the MI355X-native Groth16 (BN254) proving path for Circom circuits.
 *
 * Drop-in boundary for the proving path of arkworks-rs/circom-compat (ark-circom 0.5.0).  The
 * reference has no FFI of its own; the seam is the call
 *   Groth16::<Bn254, CircomReduction>::create_proof_with_reduction_and_matrices(
 *       &pk, r, s, &matrices, num_inputs, num_constraints, &full_assignment)
 * (reference benches/groth16.rs:52-60, src/zkey.rs:903-911) plus the loaders that feed it
 * (read_zkey, src/zkey.rs:53-60; R1CSFile::new, src/circom/r1cs_reader.rs:54-146).  Each entry
 * point below names the reference interface it replaces.  INTEGRATION.md shows the Rust
 * `extern "C"` binding a maintainer would add on the ark-circom side.
 *
 * Conventions
 *  - Field elements are 4 x u64 little-endian limbs in MONTGOMERY form (R = 2^256): exactly the
 *    in-memory form of ark_bn254::{Fr,Fq} (`x.0.0`) and the on-disk form of zkey points
 *    (src/zkey.rs:327-332).  "Fr" arguments (witness, r, s, CSR coefficients, h) are Montgomery.
 *  - G1 affine = x|y (64 bytes), G2 affine = x.c0|x.c1|y.c0|y.c1 (128 bytes), all-zero = point
 *    at infinity: the packed form deserialize_g1/g2 decode (src/zkey.rs:340-360).
 *  - Every function returns a g16_status; no exceptions cross the boundary; the caller owns all
 *    buffers; a ctx is not re-entrant (one call in flight per ctx, several ctxs allowed).
 *  - There is NO CPU fallback: without a usable HIP device g16_ctx_create fails with
 *    G16_ERR_NO_DEVICE.
 */
#ifndef G16_AMD_H
#define G16_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int g16_status;
enum {
  G16_OK = 0,
  G16_ERR_INVALID = 1,          /* bad argument / size mismatch                                  */
  G16_ERR_DOMAIN_TOO_LARGE = 2, /* SynthesisError::PolynomialDegreeTooLarge (qap.rs:31,66)       */
  G16_ERR_HIP = 3,              /* HIP runtime error, see g16_last_error                         */
  G16_ERR_NO_DEVICE = 4,        /* no gfx950 device visible: the product path refuses to run     */
  G16_ERR_IO = 5,               /* SerializationError / io error in a loader                     */
  G16_ERR_INTERNAL = 6
};

typedef struct g16_ctx g16_ctx;

/* Row-major sparse matrix = ConstraintMatrices::{a,b} (Vec<Vec<(Fr, usize)>>, src/zkey.rs:165-194)
 * flattened to CSR.  coeff: nnz x 4 u64, Montgomery.                                              */
typedef struct {
  const uint32_t* row_ptr; /* [num_constraints + 1] */
  const uint32_t* col;     /* [nnz] wire index      */
  const uint64_t* coeff;   /* [nnz][4]              */
  uint64_t nnz;
} g16_csr;

/* ProvingKey<Bn254> as read_zkey builds it (src/zkey.rs:103-133), packed arrays on the host.     */
typedef struct {
  uint32_t n_vars;      /* N: wires incl. the constant 1 (HeaderGroth.n_vars)                    */
  uint32_t n_public;    /* p (HeaderGroth.n_public); num_inputs = p + 1                          */
  uint32_t domain_size; /* n = len(h_query)                                                      */
  const uint8_t* a_query;    /* N x 64           (zkey section 5) */
  const uint8_t* b_g1_query; /* N x 64           (section 6)      */
  const uint8_t* b_g2_query; /* N x 128          (section 7)      */
  const uint8_t* l_query;    /* (N-p-1) x 64     (section 8)      */
  const uint8_t* h_query;    /* domain_size x 64 (section 9)      */
  uint8_t alpha_g1[64], beta_g1[64], delta_g1[64];
  uint8_t beta_g2[128], delta_g2[128];
} g16_key_desc;

typedef struct {
  int device;      /* HIP device ordinal                                                        */
  int rank, world; /* point-range shard of the MSMs owned by this ctx (world = 1: everything)   */
  int window_bits; /* MSM window c; <= 0: automatic                                              */
  int planes;      /* stored multiples 2^(c*D*j)P per point; <= 0: as many as fit (full = W)     */
  int dist_wm;     /* > 0: distribute the witness map too; the ctx then proves ONLY through the
                      g16_prove_dist_phase* calls (g16_prove answers G16_ERR_INVALID).  world = 1 with
                      dist_wm = 1 is the degenerate one-rank case of that API (every exchange copies onto
                      itself: what a one-process run of the host framework's collectives drives)      */
  int reduction;   /* G16_REDUCTION_CIRCOM (0, default) or G16_REDUCTION_LIBSNARK                  */
  int shard;       /* world > 1: G16_SHARD_AUTO (0), G16_SHARD_POINTS, G16_SHARD_BUCKETS (below)    */
  int fixed_tables; /* small keys: every MSM of g16_prove as table lookups + a tree sum (per point and
                      8-bit window the multiples 1..128: 256 KiB per G1 point, 512 KiB per G2 point) and
                      the finalisation's variable-base products as two more table MSMs -- ~20 launches
                      with ~21 dependent EC additions each instead of ~75 with bucket reductions.
                      0: automatic (single-device proving ctx, <= 2^14 points per query, tables within a
                      third of the free device memory); > 0: require it (creation fails where it cannot
                      apply); < 0: never.  Results are the same group elements either way.            */
} g16_options;

/* How the MSMs of one proof are cut over `world` ranks:
 *   POINTS   every query array by contiguous point range; a rank sorts and accumulates its n/world
 *            points with the window that suits n/world (more windows, a bucket set per rank);
 *   BUCKETS  the four witness-scalar queries (A, B1, B2, L -- the witness is resident on every rank
 *            anyway): every rank keeps ALL their points (sized for 288 GB: 18 GiB at 2^22, 72 GiB at
 *            2^24) and the single-GPU window; the sorted (bucket, point) list is cut into `world`
 *            equal runs of whole sort partitions, chosen on the device from the digit histogram, and
 *            rank g accumulates and reduces run g only.  Same additions per point as on one GPU,
 *            1/world of the bucket reduction per rank, and no bucket sums on the links: the only MSM
 *            traffic is the 1 KiB record per rank.  The H query stays cut by point range -- its
 *            scalars are born sharded (the distributed witness map leaves rank g its n / world
 *            evaluations), moving them would put the whole vector on every link.
 *   AUTO     POINTS.  One rank of 8 measured alone on an MI355X takes the same time either way
 *            (7.6 / 7.8 ms at 2^22, 21.0 / 21.4 ms at 2^24, profiles/r03_proj_*.json): the window a
 *            bucket-sharded rank saves is paid back by walking all n scalars to keep an eighth of the
 *            digits; POINTS holds 1/world of the key per device.  BUCKETS stays selectable (it is the
 *            better cut where the per-device key does not matter and the windows differ more).      */
enum { G16_SHARD_AUTO = 0, G16_SHARD_POINTS = 1, G16_SHARD_BUCKETS = 2 };

/* The R1CS -> QAP reduction (the `QAP` type parameter of ark_groth16::Groth16<E, QAP>):
 *   CIRCOM   = ark_circom::CircomReduction (reference src/circom/qap.rs:12-106): snarkjs keys (.zkey)
 *   LIBSNARK = ark_groth16::LibsnarkReduction, the default of `Groth16<Bn254>` used with
 *              arkworks-generated keys (reference tests/groth16.rs:9,25-35; README.md:69-74 explains
 *              why the two must not be mixed).  Its H query has domain_size - 1 points: pass it
 *              padded with the point at infinity (all-zero) to domain_size entries.
 * The matrices handed to g16_ctx_create hold A and B only (as read_zkey produces them,
 * src/zkey.rs:188-192); c_i = a_i * b_i is used where LibsnarkReduction evaluates C.w, which is
 * the same value for a satisfying assignment (g16_check_satisfied tests that).                     */
enum { G16_REDUCTION_CIRCOM = 0, G16_REDUCTION_LIBSNARK = 1 };

#define G16_PROOF_BYTES 256   /* A(64) | B(128) | C(64), affine */
#define G16_PARTIAL_BYTES 1024 /* A | B1 | B2 | L | H | s*A | r*B1: one rank's sums, XYZZ (x, y, zz, zzz;
                                  x/zz, y/zzz affine), Montgomery; G1 128 B, G2 256 B; zz = 0: infinity */

enum { G16_QUERY_A = 0, G16_QUERY_B1 = 1, G16_QUERY_L = 2, G16_QUERY_H = 3 };

/* Uploads the key and the matrices once, precomputes NTT tables and MSM point planes.
 * Replaces: holding `(ProvingKey<Bn254>, ConstraintMatrices<Fr>)` from read_zkey (src/zkey.rs:53-60)
 * across calls.  num_constraints = matrices.num_constraints (src/zkey.rs:171).
 * Sizes: every domain the reference accepts is accepted -- G16_ERR_DOMAIN_TOO_LARGE exactly where
 * CircomReduction raises PolynomialDegreeTooLarge (num_constraints + num_inputs > 2^27: no 2n-domain,
 * src/circom/qap.rs:30-32,63-68).  The point planes are planned against the device memory that is free
 * at the call: full precomputation up to 2^25 constraints on a 288 GB device, fewer planes (more bucket
 * sets per MSM, same results) above; G16_ERR_INTERNAL "does not fit this device's memory even with
 * one plane per point" only when nothing fits.  opt->planes > 0 overrides the plan.               */
g16_status g16_ctx_create(const g16_key_desc* key, const g16_csr* a, const g16_csr* b,
                          uint32_t num_constraints, const g16_options* opt, g16_ctx** out);
void g16_ctx_destroy(g16_ctx* ctx);
/* A second prover over the SAME key on the donor's device that borrows the donor's point planes
 * (no second copy of the 21 GiB at 2^22) and owns everything else (streams, sort state, workspaces):
 * two host threads can then keep two proofs in flight, one per ctx -- the front of one (digit sort,
 * witness map) runs under the bucket reductions and the finalisation of the other.  key / a / b as
 * given to the donor (the descriptor's query pointers are not read again).  The planes are reference
 * counted: g16_ctx_destroy(donor) while siblings live only retires the donor's HANDLE (it must not be
 * used again) -- its device state is freed by the destroy of the last sibling.  Throughput mode of a
 * proving service; one proof's latency does not change.                                            */
g16_status g16_ctx_create_sibling(g16_ctx* donor, const g16_key_desc* key, const g16_csr* a, const g16_csr* b,
                                  uint32_t num_constraints, const g16_options* opt, g16_ctx** out);
const char* g16_last_error(const g16_ctx* ctx); /* ctx may be NULL: error of the last failed create */
/* g16_last_error(NULL) also holds the message of the last failed call that takes no ctx.  A call that ends with
 * G16_ERR_HIP or G16_ERR_INTERNAL because an exception was caught on the host records the exception's text there
 * (the failing HIP call with its file and line, or the allocation that failed).  That now includes the calls that
 * used to return the status alone: g16_key_check, g16_key_contribute, g16_key_contribution_check, g16_srs_check,
 * g16_srs_contribute, g16_srs_create, g16_srs_prepare, g16_srs_lagrange_check, g16_setup_from_srs /
 * _from_prepared, g16_verify_batch / _aggregate and their _keys forms, g16_verify_prepared / _inputs,
 * g16_pvk_prepare_inputs, g16_pairing_check, g16_proofs_rerandomize / _keys, g16_points_from_ark / _to_ark.
 * Not covered: g16_setup_create (its message stays internal) and the calls of g16_loaders.h, which keep their own
 * thread-local message (g16_loader_last_error).                                                        */

/* Single-process multi-device prover (`device_ids, n_dev`; section 8(e)).
 * One sharded rank per listed device INSIDE the library: the MSMs are cut over the devices as
 * opt->shard says (point ranges by default, G16_SHARD_* below) and (n_dev a power of two) the witness
 * map becomes four-step NTTs whose two
 * all-to-all transposes are hipMemcpyPeerAsync pushes over xGMI, one copy stream per peer link;
 * the 1 KiB partial records are peer-copied to device_ids[0] and summed there.  The returned ctx is
 * used like a single-device one: g16_prove / g16_prove_dev (w_dev on device_ids[0]) shard
 * transparently, nothing of a proof touches the host between the witness upload and the 256-byte
 * download.  Replaces the same reference call as g16_ctx_create + g16_prove
 * (benches/groth16.rs:52-60); a Rust caller needs no launcher and no collective library.
 * opt->device / rank / world / dist_wm are ignored (dist_wm < 0 forces a replicated witness map).
 * device_ids may repeat an ordinal (several ranks time-sharing one GPU: functional tests).
 * Direct peer access between the devices is requested and REPORTED (g16_ctx_info out[14]; one line on
 * stderr when the runtime will stage copies; G16_REQUIRE_PEER_ACCESS=1 makes that an error).
 * Creation ends with a self-test of every peer path (a 4 KiB-per-pair all-to-all echo and a gather of
 * the partial records through the copy streams, events and buffers a proof uses, known patterns
 * checked on the devices): a path that does not deliver what was sent is an ERROR here (G16_ERR_HIP,
 * g16_last_error(NULL) names the exchange and the source / destination ranks and devices), never a
 * wrong proof later.                                                                                */
g16_status g16_ctx_create_multi(const g16_key_desc* key, const g16_csr* a, const g16_csr* b,
                                uint32_t num_constraints, const int* device_ids, int n_dev,
                                const g16_options* opt, g16_ctx** out);

/* CircomReduction::witness_map_from_matrices (src/circom/qap.rs:23-88).
 * w: full_assignment, n_vars x 4 u64; h_out: domain_size x 4 u64 (natural order, Montgomery).   */
g16_status g16_witness_map(g16_ctx* ctx, const uint64_t* w, size_t n_vars, uint64_t* h_out);

/* VariableBaseMSM::msm_bigint over one resident query (ark-ec; reached from
 * create_proof_with_assignment).  scalars: len x 4 u64 Montgomery Fr; pairs scalar i with
 *   A/B1: query[1 + i]   (assignment = w[1..], as `msm(&query[1..], assignment)` upstream)
 *   L   : l_query[i]     (aux assignment = w[num_inputs..])
 *   H   : h_query[i]
 * out: affine point (64 bytes).  Only valid on a world == 1 ctx.                                  */
g16_status g16_msm_g1(g16_ctx* ctx, int which, const uint64_t* scalars, size_t len, uint8_t out[64]);
/* Same for b_g2_query[1 + i]; out: 128 bytes.                                                     */
g16_status g16_msm_g2(g16_ctx* ctx, const uint64_t* scalars, size_t len, uint8_t out[128]);
/* Device-resident variants (scalars / witness / h in HBM; BASELINE config 2 times the witness map
 * and each MSM separately without PCIe in the way).  h_dev_out: domain_size x 32 bytes, Montgomery. */
g16_status g16_witness_map_dev(g16_ctx* ctx, const void* w_dev, size_t n_vars, void* h_dev_out);
g16_status g16_msm_g1_dev(g16_ctx* ctx, int which, const void* scalars_dev, size_t len, uint8_t out[64]);
g16_status g16_msm_g2_dev(g16_ctx* ctx, const void* scalars_dev, size_t len, uint8_t out[128]);

/* Groth16::<Bn254,CircomReduction>::create_proof_with_reduction_and_matrices
 * (benches/groth16.rs:52-60, src/zkey.rs:903-911) with pk/matrices/num_inputs/num_constraints
 * taken from the ctx.  r, s: 4 u64 Montgomery Fr.  proof_out: A|B|C affine.  world == 1 only.     */
g16_status g16_prove(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4], const uint64_t* w,
                     size_t n_vars, uint8_t proof_out[G16_PROOF_BYTES]);
/* Same with the witness already resident in HBM (device pointer, n_vars x 32 bytes).             */
g16_status g16_prove_dev(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4], const void* w_dev,
                         size_t n_vars, uint8_t proof_out[G16_PROOF_BYTES]);

/* Batched proving: count proofs under the ctx's key.  Proof i equals, byte for byte, what
 * g16_prove(ctx, r + 4*i, s + 4*i, w + i*n_vars*4, n_vars, out) returns.
 * r, s: count x 4 u64 (Montgomery).  w: count x n_vars x 4 u64.  proofs_out: count x 256 bytes.
 * count == 0: G16_OK, nothing written.  On an error, proofs_out is unspecified.  Argument rules are those
 * of g16_prove_dev (world == 1; not on a dist_wm ctx).
 * Where g16_ctx_info out[15] bit 2 is set -- ctxs with fixed-base tables, and single-device bucket-path
 * ctxs up to a domain of 2^20 -- a chunk of proofs goes through every kernel in ONE pass (the bucket path:
 * one sort, accumulation and reduction per MSM for the whole chunk); the chunk is the largest that fits a
 * quarter of the device memory free at the call (at most 256; bucket path: also at most 2^24 buckets), larger
 * counts loop over chunks, and the workspace stays with the ctx until g16_ctx_destroy.  Larger bucket-path
 * keys and g16_ctx_create_multi ctxs loop over the single-proof path (same bytes).                  */
g16_status g16_prove_batch(g16_ctx* ctx, size_t count, const uint64_t* r, const uint64_t* s,
                           const uint64_t* w, size_t n_vars, uint8_t* proofs_out);
/* the same, with the witnesses resident in HBM: w_dev = count x n_vars x 32 bytes, contiguous       */
g16_status g16_prove_batch_dev(g16_ctx* ctx, size_t count, const uint64_t* r, const uint64_t* s,
                               const void* w_dev, size_t n_vars, uint8_t* proofs_out);
/* witness_map_from_matrices for count assignments in one pass (also on a witness-map-only ctx; not on
 * multi-device or dist_wm ctxs): h_out = count x domain_size x 4 u64, entry i == g16_witness_map(ctx, w_i) */
g16_status g16_witness_map_batch(g16_ctx* ctx, size_t count, const uint64_t* w, size_t n_vars,
                                 uint64_t* h_out);

/* Multi-GPU (one process per GPU): every rank computes the sums of ITS point range -- and, while
 * its remaining MSMs run, the two products s*A_rank and r*B1_rank the finalisation is linear in --
 * the host framework all-gathers the G16_PARTIAL_BYTES records (RCCL all_gather; EC addition is
 * not an ncclRedOp, so "all-reduce" = all-gather + local add), then any rank finishes the proof
 * with fixed-base table sums only.  partials: world x G16_PARTIAL_BYTES in rank order.             */
g16_status g16_prove_partial(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4],
                             const uint64_t* w, size_t n_vars,
                             uint8_t partial_out[G16_PARTIAL_BYTES]);
g16_status g16_prove_partial_dev(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4],
                                 const void* w_dev, size_t n_vars,
                                 uint8_t partial_out[G16_PARTIAL_BYTES]);
g16_status g16_prove_finish(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4],
                            const uint8_t* partials, int world, uint8_t proof_out[G16_PROOF_BYTES]);

/* Device-side hand-offs for host frameworks that own a stream (one process per GPU, torch / RCCL):
 * after g16_dist_set_exchange_stream(ctx, hipStream_t, 1) the phase calls below never block the
 * host -- the registered stream is made to wait (hipStreamWaitEvent) for each send buffer / partial
 * record, and every phase waits for what the caller has enqueued on that stream so far (its
 * all-to-all / all-gather).  g16_partial_buffer(): this rank's record in HBM (G16_PARTIAL_BYTES),
 * the all-gather's input; g16_gather_buffer(): world x G16_PARTIAL_BYTES, its output;
 * g16_prove_finish_dev() consumes the latter in place.  Without a registered stream the calls
 * block until their output is complete (frameworks that cannot share a stream).                    */
g16_status g16_dist_set_exchange_stream(g16_ctx* ctx, void* hip_stream, int enabled);
void* g16_partial_buffer(g16_ctx* ctx);
void* g16_gather_buffer(g16_ctx* ctx);
g16_status g16_prove_finish_dev(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4],
                                uint8_t proof_out[G16_PROOF_BYTES]);

/* Fully sharded prover (ctx created with options.dist_wm = 1, world a power of two): the witness map
 * (CircomReduction::witness_map_from_matrices, src/circom/qap.rs:23-88) is split over the ranks as
 * four-step NTTs whose two transposes are all-to-all exchanges the host framework performs
 * (RCCL all_to_all over xGMI) between the three phases.  send/recv: device buffers of
 * g16_dist_exchange_bytes() bytes, `world` equal chunks in rank order (all_to_all_single layout).
 *   phase1(r, s, w_dev, send)  -> exchange 1 -> phase2(recv, send) -> exchange 2
 *   -> phase3(recv, partial_out) -> all-gather of the partial records -> g16_prove_finish.
 * The rank's A / B1 / L / B2 MSMs run on the ctx's main stream during the exchanges.               */
size_t g16_dist_exchange_bytes(const g16_ctx* ctx);
g16_status g16_prove_dist_phase1(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4],
                                 const void* w_dev, size_t n_vars, void* send_dev);
g16_status g16_prove_dist_phase2(g16_ctx* ctx, const void* recv_dev, void* send_dev);
/* partial_out may be NULL when an exchange stream is registered: the record then stays in
 * g16_partial_buffer() and the registered stream waits for it.                                     */
g16_status g16_prove_dist_phase3(g16_ctx* ctx, const void* recv_dev,
                                 uint8_t partial_out[G16_PARTIAL_BYTES]);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------ */
#define G16_N_STAGES 10
g16_status g16_set_profiling(g16_ctx* ctx, int enabled);
/* HIP-event times accumulated since the last call; resets the accumulators.  Stages, in order:
 * witness_map, msm_sort, msm_accumulate_g1 (L, H), msm_accumulate_g2 (B2), msm_reduce, finalize,
 * msm_accumulate_g1_pair (A | B1 in one launch), msm_fixup (the exact additions behind an optimistic
 * G1 launch); g16_stage_name() returns the same strings.                                            */
g16_status g16_stage_times(g16_ctx* ctx, float ms[G16_N_STAGES], uint32_t launches[G16_N_STAGES]);
const char* g16_stage_name(int stage);
/* sizes chosen at create time: out[0]=c_w out[1]=W_w out[2]=planes_w out[3]=D_w, [4..7] same for H,
 * out[8] = domain_size, out[9] = log2(domain_size), out[10] / out[11] = points of the witness / H
 * shard (rank 0's for a multi-device ctx), out[12] = devices, out[13] = how a world > 1 ctx shards
 * (G16_SHARD_POINTS / G16_SHARD_BUCKETS; 0 for world = 1), out[14] = multi-device ctx: 1 when every
 * pair of its devices has direct peer access, 2 when some exchanges are staged by the runtime,
 * out[15] = bit 0: g16_prove goes through the fixed-base tables (g16_options.fixed_tables); bit 1: the
 * B2 (G2) MSM runs over a filtered view of the witness sort (>= 1/8 of b_g1_query / b_g2_query is the
 * point at infinity: wires that appear in no B row of a real circom circuit); bit 2: a chunk of
 * g16_prove_batch is enqueued once (table ctxs; single-device bucket ctxs up to a domain of 2^20)      */
g16_status g16_ctx_info(const g16_ctx* ctx, uint32_t out[16]);
/* Multi-device ctx (g16_ctx_create_multi with a distributed witness map): what every ordered (source,
 * destination) pair of its ranks delivered at create time, measured with the copies a proof makes --
 * gbps[src * n + dst] = GB/s of one peer copy of *probe_bytes (<= 64 MiB) from src's exchange buffer
 * into dst's; echo_us[src * n + dst] = microseconds of a 4 KiB copy there and back (host-timed, launch
 * latency included).  n = g16_ctx_info out[12]; at most `cap` entries of each table are written.  The
 * reference has nothing to compare (single process, CPU); this is the per-link figure the scaling
 * projection assumes, turned into a measurement on the first multi-GPU box.      */
g16_status g16_multi_links(const g16_ctx* ctx, float* gbps, float* echo_us, int cap, uint64_t* probe_bytes);
/* device pointer of the ctx's witness staging buffer (n_vars x 32 bytes) for g16_prove_dev        */
void* g16_witness_buffer(g16_ctx* ctx);
/* Makes the witness resident: copies it into the ctx's device staging buffer -- into EVERY device's
 * for a multi-device ctx -- and returns when it is there.  g16_prove_dev(ctx, r, s,
 * g16_witness_buffer(ctx), ...) then proves from the resident copies without moving the witness
 * (the multi-device ctx otherwise peer-broadcasts a device-resident witness from the first device
 * inside every call).
 * The resident witness is replaced by the calls that take a witness from the HOST -- they stage it in
 * the same buffer: g16_prove, g16_witness_map, g16_prove_partial, g16_prove_batch / g16_witness_map_batch,
 * their *_canonical variants (a refused one, value >= r, included) and the two uploads themselves -- and,
 * on a multi-device ctx, by g16_prove_dev from any other device pointer (the peer broadcast lands there).
 * No other call replaces it: g16_msm_g1 / g16_msm_g2 stage their host scalars in a buffer of their own
 * (allocated at the first such call), the other *_dev calls stage nothing, and a call refused for its arguments
 * (wrong n_vars, too many scalars) touches no device memory.                                            */
g16_status g16_witness_upload(g16_ctx* ctx, const uint64_t* w, size_t n_vars);
/* ---- canonical witnesses ----------------------------------------------------------------------------
 * The witness as snarkjs, rapidsnark and circom's C++ calculator write it (.wtns section 2; g16_wtns_values in
 * g16_loaders.h): n_vars x 32 bytes, each a little-endian integer below r.  The calls below take those bytes
 * where their namesakes take Montgomery limbs: the bytes are copied into the same device staging buffer on the
 * same stream and converted there in place by one kernel launch (one lane per element) ahead of the witness's
 * first consumer, so the proof is byte for byte that of g16_prove on the converted witness.
 * A value >= r: G16_ERR_INVALID, g16_last_error names the proof and the element, *first_bad (may be NULL) holds
 * the index of the first such element -- proof * n_vars + element in the batch call -- and -1 otherwise, and no
 * proof is written.  (The element itself reaches the device as 0, never unreduced.)
 * g16_fr_convert: host in, host out through `device`, the bulk form of g16_fr_from_canonical (witness lists, the
 * public inputs of large verification batches); n == 0: G16_OK; out_mont is written only when every value is
 * in range; its message is in g16_last_error(NULL).
 * g16_witness_upload_canonical: g16_witness_upload; a multi-device ctx converts on its first device and
 * peer-copies the result to the others.  g16_prove_batch_canonical: the witnesses go into the batch workspace's
 * witness staging, one conversion launch per chunk, then g16_prove_batch_dev's path.                           */
g16_status g16_fr_convert(int device, const uint8_t* in_le, uint64_t* out_mont, size_t n, int64_t* first_bad);
/* device milliseconds the calling thread's last g16_fr_convert spent in 0 upload, 1 the conversion kernel,
 * 2 download (HIP events); entries from 3 on are 0                                                            */
g16_status g16_fr_convert_times(float* ms, uint32_t cap);
g16_status g16_witness_upload_canonical(g16_ctx* ctx, const uint8_t* w_le, size_t n_vars, int64_t* first_bad);
g16_status g16_prove_canonical(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4], const uint8_t* w_le,
                               size_t n_vars, uint8_t proof_out[G16_PROOF_BYTES]);
g16_status g16_prove_batch_canonical(g16_ctx* ctx, size_t count, const uint64_t* r, const uint64_t* s,
                                     const uint8_t* w_le, size_t n_vars, uint8_t* proofs_out, int64_t* first_bad);
/* page-locked HOST staging buffer (n_vars x 32 bytes, owned by the ctx): a caller that writes the
 * full assignment here (instead of into a Vec) gets the H2D copy of g16_prove at PCIe line rate   */
void* g16_witness_host_buffer(g16_ctx* ctx);

/* Constraint satisfaction of a witness: (A_i . w)(B_i . w) == C_i . w for every row, the check
 * CircomBuilder::build performs in debug builds (reference src/circom/builder.rs:101-114; the
 * reference's unit test at src/circom/circuit.rs:92-107 asserts cs.is_satisfied()).  a, b, c: the
 * R1CS rows as CSR (g16_r1cs_matrices); *first_unsatisfied = row index, or -1 when satisfied.     */
g16_status g16_check_satisfied(int device, const g16_csr* a, const g16_csr* b, const g16_csr* c,
                               uint32_t num_constraints, const uint64_t* w, size_t n_vars,
                               int64_t* first_unsatisfied);

/* ---- batch verification (not on the proving path) --------------- */
/* VerifyingKey<Bn254> in the packed forms read_zkey produces (src/zkey.rs:241-257): ic =
 * gamma_abc_g1, ic_count = n_public + 1 points of 64 bytes.                                        */
typedef struct {
  uint8_t alpha_g1[64];
  uint8_t beta_g2[128], gamma_g2[128], delta_g2[128];
  const uint8_t* ic;
  uint32_t ic_count;
} g16_vk_desc;
/* Groth16::process_vk + verify_with_processed_vk (reference call sites src/zkey.rs:868-870,914-916;
 * tests/groth16.rs:33-35) for n_proofs proofs under one key, one GPU lane per proof:
 *   ok_out[i] = 1 iff e(A_i, B_i) = e(alpha, beta) e(IC_0 + sum_j pub_ij IC_{j+1}, gamma) e(C_i, delta)
 * proofs: n_proofs x G16_PROOF_BYTES (A | B | C as g16_prove writes them); public_inputs:
 * n_proofs x (ic_count - 1) x 4 u64 Montgomery Fr.  The reference only ever pairs a DESERIALISED
 * Proof, and ark-serialize (Validate::Yes) rejects what this call therefore rejects itself with
 * ok = 0 before any pairing: a coordinate that is not canonical (stored value >= q), a point off its
 * curve, a B outside the prime-order subgroup of the twist ([r] B != infinity).
 * This is g16_verify_batch_keys (below) with one group, and shares its limit: n_proofs + 3 lanes are
 * indexed in 32 bits, so n_proofs > 2^32 - 4 is G16_ERR_INVALID.                                    */
g16_status g16_verify_batch(int device, const g16_vk_desc* vk, const uint8_t* proofs,
                            const uint64_t* public_inputs, uint32_t n_proofs, uint8_t* ok_out);

/* All n_proofs proofs under one key in ONE combined pairing check (the small-exponent batch test):
 *   prod_i ML(B_i, rho_i A_i) * ML(beta, -(sum_i rho_i) alpha) * ML(gamma, -sum_i rho_i X_i)
 *       * ML(delta, -sum_i rho_i C_i)   --final exponentiation-->   1,
 *   X_i = IC_0 + sum_j pub_ij IC_{j+1},  sum_i rho_i X_i = (sum_i rho_i) IC_0 + sum_j (sum_i rho_i pub_ij) IC_{j+1}
 * i.e. per proof one Miller loop and two 128-bit G1 multiplications; the three key-side Miller
 * loops and the final exponentiation are paid once per batch.
 * *ok_out = 1 iff every proof passes the structural checks g16_verify_batch applies (canonical
 * coordinates, A and C on the curve, B on the twist and in the prime-order subgroup) AND the
 * combined equation holds.  A batch that contains an invalid proof passes with probability at most
 * 2^-127 PROVIDED the rho_i are unpredictable to whoever made the proofs.  They must be: a prover
 * who knows rho forges a pair of individually invalid proofs that cancel in the sum
 * (C_0' = C_0 + rho_1 D, C_1' = C_1 - rho_0 D for any D in G1), and the batch passes.
 * rho: n_proofs x 2 u64 (little-endian 128-bit integers, NOT Montgomery), every one non-zero, or
 *      NULL: the library then draws them from the operating system's CSPRNG (getrandom, else
 *      /dev/urandom; a failure to get randomness is G16_ERR_INTERNAL, never a fixed fallback).  A
 *      caller passes rho to derive it from its own transcript hash (one that covers the proofs), or
 *      to be reproducible in a test.
 * structural_out: NULL, or n_proofs bytes: 1 where proof i passed the structural checks (a caller
 *      learns which proofs were malformed without a second call).
 * proofs, public_inputs, vk and the treatment of infinity (a pair with an infinite side contributes
 * 1) are those of g16_verify_batch, so the verdict on a batch of one proof is g16_verify_batch's.
 * n_proofs == 0: G16_OK, *ok_out = 1.  A zero rho entry: G16_ERR_INVALID.
 * This is g16_verify_aggregate_keys (below) with one group, and shares its limit: n_proofs + 3 lanes
 * are indexed in 32 bits, so n_proofs > 2^32 - 4 is G16_ERR_INVALID.                                */
g16_status g16_verify_aggregate(int device, const g16_vk_desc* vk, const uint8_t* proofs,
                                const uint64_t* public_inputs, uint32_t n_proofs,
                                const uint64_t* rho, uint8_t* ok_out, uint8_t* structural_out);

/* Proofs under MANY keys in one pass.  A GROUP is one key together with the proofs under it: group k is
 * vks[k] with counts[k] proofs.  The two calls above cost a serial chain (front, one Miller loop, one
 * final exponentiation) that is almost flat in the batch size; a caller with n_keys keys pays it n_keys
 * times, one key after the other.  Here all groups share every kernel launch and the final
 * exponentiations of the groups run side by side, so n_keys groups cost about what one does.  The number
 * of launches, allocations, copies and synchronisations does not depend on n_keys.
 * proofs: N = sum_k counts[k] records of G16_PROOF_BYTES, group after group.
 * public_inputs: the groups' blocks one after the other, group k's being counts[k] x (vks[k]->ic_count - 1)
 *      x 4 u64 Montgomery Fr.  Keys may have different numbers of public inputs, including none.
 * The same key may appear in several groups; the groups stay separate.  One device; nothing is combined
 * across groups: there is no verdict "all groups hold" other than the AND of the per-group verdicts.
 *
 * g16_verify_aggregate_keys: ok_out[k] (n_keys bytes) is exactly what
 *   g16_verify_aggregate(device, vks[k], group k's proofs, its public inputs, counts[k], its slice of rho, ..)
 * writes to *ok_out: the same combined equation over group k ALONE, the same structural rules, the same
 * treatment of infinity; an empty group gives 1.  Each group has its own 2^-127 bound.  Sums never cross
 * a group boundary: the forged pair described above, split over two groups of the same key, fails both.
 * rho: N x 2 u64 in the encoding of g16_verify_aggregate, every one non-zero, or NULL: drawn from the
 *      operating system's CSPRNG exactly as that call does (no fixed fallback).
 * structural_out: NULL, or N bytes as in that call, indexed over all N proofs.
 *
 * g16_verify_batch_keys: ok_out[i] (N bytes) is what g16_verify_batch writes for proof i under its
 * group's key.
 *
 * G16_ERR_INVALID: a NULL where data is needed, vks[k] NULL, ic NULL or ic_count < 1 in any key, a zero
 * rho entry, N + 3 n_keys not fitting 32 bits.  n_keys == 0: G16_OK, nothing is written.               */
g16_status g16_verify_aggregate_keys(int device, const g16_vk_desc* const* vks, const uint32_t* counts,
                                     uint32_t n_keys, const uint8_t* proofs, const uint64_t* public_inputs,
                                     const uint64_t* rho, uint8_t* ok_out /* n_keys */,
                                     uint8_t* structural_out /* sum(counts) or NULL */);
g16_status g16_verify_batch_keys(int device, const g16_vk_desc* const* vks, const uint32_t* counts,
                                 uint32_t n_keys, const uint8_t* proofs, const uint64_t* public_inputs,
                                 uint8_t* ok_out /* sum(counts) */);

/* ---- proving-key validation (not on the proving path) ------------------------------------------- */
/* The loaders (g16_zkey_open, like the reference's deserialize_g1 / deserialize_g2, src/zkey.rs:328-360:
 * `new_unchecked`) copy the point sections of a key as they come, and g16_ctx_create builds tables from
 * whatever it is given: a key with a flipped bit, a b_g2_query point outside G2 or a b_g1_query that does
 * not match b_g2_query proves at full speed and every proof is garbage.  g16_key_check is what
 * ark-serialize's Validate::Yes / `snarkjs zkey verify` (its point checks) do for such a key, on the GPU:
 * call it once after loading a key that was not minted locally.  Standalone: no ctx is needed, a ctx
 * alive on the device is left untouched.
 *
 * Structural checks, on EVERY point of every query and on the single points -- the three tests
 * g16_verify_batch applies to the points of a proof:
 *   G16_KEY_BAD_NONCANONICAL  one of the 8 (G1) / 16 (G2) stored 32-byte words is >= q
 *   G16_KEY_BAD_OFF_CURVE     not on y^2 = x^3 + 3 / on the twist y^2 = x^3 + 3 / (9 + i)
 *   G16_KEY_BAD_SUBGROUP      G2 only: [r] P != infinity (the twist has the cofactor 2q - r; G1 has 1)
 * A point's reason is the FIRST test it fails, in that order (field arithmetic on a value >= q and the
 * group law on a point off the curve mean nothing, so the later tests are not evaluated).  The all-zero
 * encoding is the point at infinity: valid, counted in n_infinity.
 * Queries: A, B1, B2, L, H of the key; IC = vk->ic (n_points 0 without vk); SINGLES, index 0 alpha_g1,
 * 1 beta_g1, 2 delta_g1, 3 beta_g2, 4 delta_g2, 5 vk->gamma_g2 (5 points without vk).
 * bad_out receives the first min(bad_cap, 65536) bad points in ascending (query, index) order -- the same
 * list on every run (built by scans, no atomics); n_bad counts all of them.
 *
 * Relations, evaluated only when no structural check failed (relations_checked = 0 and relations_failed
 * = 0 otherwise: a pairing of a malformed point means nothing):
 *   G16_KEY_PAIR_BETA    e(beta_g1, g2)  != e(g1, beta_g2)
 *   G16_KEY_PAIR_DELTA   e(delta_g1, g2) != e(g1, delta_g2)
 *   G16_KEY_PAIR_B       e(sum_i rho_i b_g1_query[i], g2) != e(g1, sum_i rho_i b_g2_query[i]) over all n_vars
 *                        entries: the two B queries hold the same scalars.  With unpredictable rho a key
 *                        whose queries differ in any entry passes with probability at most 2^-127 (the
 *                        small-exponent test of g16_verify_aggregate; whoever knows rho can make two
 *                        entries cancel: B1_j + rho_k D, B1_k - rho_j D).
 *   G16_KEY_VK_MISMATCH  vk given: vk->alpha_g1 / beta_g2 / delta_g2 differ from the key's bytes, or
 *                        vk->ic_count != n_public + 1
 * (g1, g2: the standard generators, against which snarkjs and arkworks keys are made.)
 * rho: n_vars x 2 u64 (little-endian 128-bit integers, NOT Montgomery), every one non-zero (a zero entry:
 *      G16_ERR_INVALID), or NULL: drawn from the operating system's CSPRNG as g16_verify_aggregate does (a
 *      failure to get randomness is G16_ERR_INTERNAL, never a fixed fallback).
 *
 * NOT checked: that the key belongs to a circuit.  The A / L / H queries and IC are tied to the R1CS only
 * through the ceremony's powers of tau, and the matrices are not looked at here: g16_setup_from_srs
 * recomputes the initial key from them and g16_key_contribution_check compares (the Python binding's
 * check_key_circuit does both).  report->ok = 1 means the key is well formed and internally consistent --
 * proofs made with it are then at least proofs under the key's own verifying key -- not that it is the key
 * of your circuit.
 *
 * Memory: the queries are streamed through two page-locked host slots and two device slots of
 * min(2^18, longest query) points (208 bytes per point), the copy of one chunk under the kernels of the
 * one before; device use does not grow with the key.  G16_KEYCHECK_CHUNK=<points> overrides the chunk
 * (tests).  Returns G16_OK when the check RAN (the verdict is in *report), G16_ERR_INVALID for bad
 * arguments, G16_ERR_NO_DEVICE without a device: there is no CPU fallback.                           */
enum { G16_KEY_Q_A = 0, G16_KEY_Q_B1, G16_KEY_Q_B2, G16_KEY_Q_L, G16_KEY_Q_H, G16_KEY_Q_IC,
       G16_KEY_Q_SINGLES /* index: 0 alpha_g1 1 beta_g1 2 delta_g1 3 beta_g2 4 delta_g2 5 vk.gamma_g2 */,
       G16_KEY_N_QUERIES };
enum { G16_KEY_BAD_NONCANONICAL = 1, G16_KEY_BAD_OFF_CURVE = 2, G16_KEY_BAD_SUBGROUP = 4 };   /* per-point reason bits */
enum { G16_KEY_PAIR_BETA = 1, G16_KEY_PAIR_DELTA = 2, G16_KEY_PAIR_B = 4, G16_KEY_VK_MISMATCH = 8 }; /* report.relations_failed */
typedef struct { uint32_t query, index, reason; } g16_key_bad_point;
typedef struct {
  uint8_t  ok;                 /* 1 iff no bad point and no failed relation */
  uint8_t  relations_checked;  /* 0 when a structural failure made the pairing relations meaningless */
  uint32_t relations_failed;   /* G16_KEY_PAIR_* | G16_KEY_VK_MISMATCH */
  uint64_t n_points[G16_KEY_N_QUERIES], n_bad[G16_KEY_N_QUERIES], n_infinity[G16_KEY_N_QUERIES];
  uint32_t n_listed;           /* entries written to bad_out */
} g16_key_report;
g16_status g16_key_check(int device, const g16_key_desc* key, const g16_vk_desc* vk /* NULL ok */,
                         const uint64_t* rho /* n_vars x 2 u64, NULL = CSPRNG */,
                         g16_key_bad_point* bad_out, uint32_t bad_cap, g16_key_report* report);

/* ---- phase-2 delta contributions (not on the proving path) --------------------------------------- */
/* g16_setup_create mints a key from toxic waste its caller knows.  g16_key_contribute re-randomises delta,
 * the point arithmetic of `snarkjs zkey contribute` / `zkey beacon`:
 *   delta_g1' = d delta_g1, delta_g2' = d delta_g2, l_query'[i] = d^-1 l_query[i], h_query'[i] = d^-1 h_query[i]
 * Everything else of the key is untouched and not read beyond the descriptor (A, B1, B2, alpha, beta, IC,
 * gamma).  The key of (tau, alpha, beta, gamma, delta) becomes, byte for byte, the key g16_setup_create mints
 * for (tau, alpha, beta, gamma, delta d).
 * d: 4 u64 Montgomery Fr, 1 <= d < r (0 or a non-canonical value: G16_ERR_INVALID), or NULL: the library draws
 *    d uniformly from [1, r) from the operating system's CSPRNG (rejection sampling; a failure to get
 *    randomness is G16_ERR_INTERNAL, never a fixed fallback), never returns it and overwrites every copy of d
 *    and of d^-1 (host and device) before it returns.
 * l_out: (n_vars - n_public - 1) x 64 bytes, h_out: domain_size x 64 bytes: canonical affine Montgomery x|y as
 *    in the key, infinity stays all-zero.  l_out / h_out may BE key->l_query / key->h_query (in place); any
 *    other overlap is not supported.
 * The key is expected to be well formed (g16_key_check): a point off the curve is multiplied like any other
 * and means nothing afterwards.
 * Standalone like g16_key_check: no ctx, a ctx alive on the device is left untouched.  The two queries are
 * streamed through two page-locked host slots and two device slots of min(2^18, longest query) points (64
 * bytes per point, plus one 128-byte work entry per point of ONE chunk): the copy of chunk k + 1 and the
 * download of chunk k - 1 run under the kernels of chunk k; device use does not grow with the key.
 * G16_CONTRIB_CHUNK=<points> overrides the chunk (tests).  No atomics: the bytes do not depend on scheduling.
 *
 * NOT built: the snarkjs section-10 transcript (Blake2b challenge, proof of knowledge of d, beacon mode) is
 * neither written nor verified, so a contributed .zkey carries no contribution record `snarkjs zkey verify`
 * would accept.                                                                                      */
g16_status g16_key_contribute(int device, const g16_key_desc* key,
                              const uint64_t d[4] /* Montgomery Fr, 1 <= d < r; NULL = CSPRNG */,
                              uint8_t* l_out, uint8_t* h_out, uint8_t delta_g1_out[64], uint8_t delta_g2_out[128]);

/* Is `after` the key `before` with only delta changed (the sameRatio checks of `snarkjs zkey verify`)?
 * In this order:
 *   1. bytes, on the host: n_vars, n_public, domain_size, alpha_g1, beta_g1, beta_g2, a_query, b_g1_query and
 *      b_g2_query must be identical; a difference sets G16_CONTRIB_UNCHANGED_MISMATCH (reported whatever
 *      else fails).  When the SIZES differ nothing can be compared entry by entry: the call returns G16_OK at
 *      once with ok = 0, relations_checked = 0 and that bit alone.
 *   2. structure of after's delta_g1, delta_g2, l_query, h_query: canonical, on the curve, delta_g2 in the
 *      r-torsion -- the predicates, reason bits and first-failure rule of g16_key_check.  bad_out receives the
 *      first min(bad_cap, 65536) bad points in ascending (query, index) order (G16_KEY_Q_L, G16_KEY_Q_H, then
 *      G16_KEY_Q_SINGLES with index 2 = delta_g1, 4 = delta_g2), built by scans: the same list on every run.
 *      The all-zero encoding is the point at infinity: valid.
 *   3. relations, evaluated only when nothing structural failed (relations_checked = 0 otherwise):
 *      G16_CONTRIB_DELTA_INFINITE  after's delta_g1 or delta_g2 is the point at infinity
 *      G16_CONTRIB_PAIR_DELTA      e(delta_g1', g2) != e(g1, delta_g2')
 *      G16_CONTRIB_PAIR_L          e(sum rho_i L_i, delta_g2) != e(sum rho_i L'_i, delta_g2')
 *      G16_CONTRIB_PAIR_H          the same for the H query, with its own rho
 *      With unpredictable rho a pair of keys whose L (H) queries differ by anything but the one factor that
 *      takes delta_g2' to delta_g2 passes with probability at most 2^-127 (the small-exponent test of
 *      g16_verify_aggregate and g16_key_check); whoever knows rho makes two entries cancel
 *      (L'_j + rho_k D, L'_k - rho_j D for any D in G1), and the relation holds.
 * `before` is expected to have passed g16_key_check: its points are not tested again.
 * rho: (len L + len H) x 2 u64 -- L's coefficients, then H's (little-endian 128-bit integers, NOT Montgomery),
 *      every one non-zero (a zero entry: G16_ERR_INVALID), or NULL: drawn from the operating system's CSPRNG (a
 *      failure to get randomness is G16_ERR_INTERNAL, never a fixed fallback).
 * NOT checked: the contribution transcript (see g16_key_contribute), and that either key belongs to a circuit.
 * Standalone and streamed like g16_key_check (144 bytes per point and slot; G16_CONTRIB_CHUNK).  Returns
 * G16_OK when the check RAN: the verdict is in *report.                                               */
enum { G16_CONTRIB_UNCHANGED_MISMATCH = 1, G16_CONTRIB_PAIR_DELTA = 2, G16_CONTRIB_PAIR_L = 4,
       G16_CONTRIB_PAIR_H = 8, G16_CONTRIB_DELTA_INFINITE = 16 };   /* report.relations_failed */
typedef struct {
  uint8_t  ok;                 /* 1 iff no bad point, no failed relation and nothing else changed */
  uint8_t  relations_checked;  /* 0 when a structural failure made the pairing relations meaningless */
  uint32_t relations_failed;   /* G16_CONTRIB_* */
  uint64_t n_bad_l, n_bad_h;   /* bad points of after's l_query / h_query (all of them, listed or not) */
  uint32_t n_listed;           /* entries written to bad_out */
} g16_contribution_report;
g16_status g16_key_contribution_check(int device, const g16_key_desc* before, const g16_key_desc* after,
                                      const uint64_t* rho /* (len L + len H) x 2 u64, NULL = CSPRNG */,
                                      g16_key_bad_point* bad_out, uint32_t bad_cap,
                                      g16_contribution_report* report);

/* ---- RCCL inside the library (north_star: "a final RCCL all-reduce of partial bucket sums over xGMI") ---- */
/* A host that is not PyTorch (the Rust shim) creates one per-rank ctx per process (g16_options.rank / world,
 * dist_wm = 1) and ONE ncclComm_t over the same ranks with its own RCCL (ncclGetUniqueId / ncclCommInitRank),
 * then hands it over: nccl_comm is that opaque handle.  The library resolves ncclAllToAll / ncclAllGather /
 * ncclCommCount from the RCCL already loaded in the process (dlsym(RTLD_DEFAULT)), else from librccl.so -- it does
 * not link RCCL.  The collectives MUST run in the same RCCL copy that created the communicator: a host that links
 * RCCL has it in the global symbol scope; a host that dlopen()s it (Python's ctypes) must open it with RTLD_GLOBAL
 * (tests/test_gpu_large.py, scripts/rccl_inlib_ranks.py do).  The library checks that the communicator has g16_options.world ranks, allocates the two exchange buffers and a
 * high-priority exchange stream.  Afterwards g16_prove_dist is one whole sharded proof per rank:
 *   phase 1 -> ncclAllToAll -> phase 2 -> ncclAllToAll -> phase 3 -> ncclAllGather of the 1 KiB records -> finish
 * (the g16_prove_dist_phase* calls with the collectives in between, ordered by events: the host never blocks
 * between phases).  Every rank returns the same 256 proof bytes.  EC addition is not an ncclRedOp: the
 * "all-reduce of bucket sums" is this all-gather + a local sum of world records.
 * g16_dist_rccl_ranks: ranks of the attached communicator, 0 when none is attached.                     */
g16_status g16_dist_attach_rccl(g16_ctx* ctx, void* nccl_comm);
int g16_dist_rccl_ranks(const g16_ctx* ctx);
g16_status g16_prove_dist(g16_ctx* ctx, const uint64_t r[4], const uint64_t s[4], const void* w_dev,
                          size_t n_vars, uint8_t proof_out[G16_PROOF_BYTES]);

/* ---- EvaluationDomain::fft_in_place / ifft_in_place ----------------------------- */
/* ark-poly Radix2EvaluationDomain::{fft_in_place, ifft_in_place} as called from reference
 * src/circom/qap.rs:60-61,72-73,79-81: in-place size-2^log_n transform of host data (Montgomery Fr),
 * natural order in and out, 1/n folded into the inverse.  impl selects which of the library's two
 * transform stacks runs it: 2 = the witness map's lazy-limb DIF kernels + bit reversal (ntt29.hip; the
 * default a caller wants), 3 = bit reversal + its DIT kernels (forward only); 0 / 1 = the same two
 * schedules on the saturated-limb kernels of ntt.hip, which the key generator uses.                */
g16_status g16_fft_in_place(int device, uint64_t* data, int log_n, int inverse, int impl);

#ifdef G16_DEBUG_ABI
/* Measurement only, NOT part of the product library: compiled when the library is built with
 * EXTRA=-DG16_DEBUG_ABI (scripts/alu_bench.py).  Integer-ALU ceilings: kind 0 = Fq Montgomery
 * multiplications, 1 = raw v_mad_u64_u32, 2 = G1 mixed additions (saturated limbs), 3 / 4 = G1 / G2 mixed
 * additions on the lazy limbs the MSM kernels use.  Returns elapsed seconds and the number of operations. */
g16_status g16_debug_alu_bench(int device, int kind, uint32_t blocks, uint32_t iters,
                               double* seconds, double* ops);
#endif

/* ---- synthetic keys (not on the proving path) --------------------- */
/* Trapdoor (known toxic waste) circom/snarkjs-style setup on the GPU: what
 * Groth16::generate_random_parameters_with_reduction::<CircomReduction> computes (call shape:
 * reference tests/groth16.rs:25; H basis: CircomReduction::h_query_scalars, src/circom/qap.rs:90-105).
 * at/bt/ct: TRANSPOSED constraint matrices (row = wire, col = constraint, Montgomery coefficients),
 * `at` including the n_public+1 rows snarkjs appends (row m+i holds coefficient 1 on signal i).
 * toxic: tau, alpha, beta, gamma, delta as 5 x 4 u64 Montgomery Fr.
 * The matrices are checked on the host before anything is allocated, copied or launched, here and in
 * g16_setup_from_srs / g16_setup_from_prepared -- G16_ERR_INVALID and *out = NULL for: a NULL row_ptr, or NULL
 * col / coeff with nnz > 0; row_ptr[0] != 0, row_ptr[n_vars] != nnz or a step back in between; a col of `at`
 * >= num_constraints + n_public + 1, of bt or ct >= num_constraints; n_vars < n_public + 1.          */
typedef struct g16_setup g16_setup;
g16_status g16_setup_create(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct,
                            uint32_t n_vars, uint32_t n_public, uint32_t num_constraints,
                            const uint64_t* toxic, g16_setup** out);
/* Same with the reduction named (G16_REDUCTION_*): the H query is CircomReduction's or
 * LibsnarkReduction's h_query_scalars (the rest of the key is identical: CircomReduction
 * delegates instance_map_with_evaluation to LibsnarkReduction, src/circom/qap.rs:16-21).          */
g16_status g16_setup_create_ex(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct,
                               uint32_t n_vars, uint32_t n_public, uint32_t num_constraints,
                               const uint64_t* toxic, int reduction, g16_setup** out);
/* host arrays owned by the handle; ic: (n_public+1) x 64 bytes = vk.gamma_abc_g1                  */
g16_status g16_setup_key(g16_setup* s, g16_key_desc* key, const uint8_t** ic, uint32_t* ic_count,
                         uint8_t gamma_g2[128]);
void g16_setup_destroy(g16_setup* s);

/* ---- setup from a powers-of-tau string: keys without toxic waste (not on the proving path) ------- */
/* The first step of `snarkjs zkey new <r1cs> <ptau>` -> `zkey contribute` -> `zkey verify`: the initial key
 * (gamma = delta = 1) of a circuit from a ceremony's structured reference string, with nobody knowing tau,
 * alpha or beta.  The SRS holds packed affine points in the zkey encoding (Montgomery limbs, all-zero =
 * infinity), sections 2-6 of a snarkjs .ptau:
 *   tau_g1[i] = tau^i G1 (>= 2 domain - 1 entries), tau_g2[i] = tau^i G2, alpha_tau_g1[i] = alpha tau^i G1,
 *   beta_tau_g1[i] = beta tau^i G1 (>= domain entries each), beta_g2 = beta G2
 * with domain the smallest power of two >= num_constraints + n_public + 1 (g16_setup_create's rule and its
 * G16_ERR_DOMAIN_TOO_LARGE limit, which is tested before anything is dereferenced).  Entries beyond those
 * counts are ignored.  at / bt / ct, n_vars, n_public, num_constraints and reduction are g16_setup_create_ex's.
 * The Lagrange bases L_j(tau) G1, alpha L_j(tau) G1, beta L_j(tau) G1 and L_j(tau) G2 are inverse size-domain
 * transforms over the group; every query entry is a sparse combination of them with the circuit's
 * coefficients; the H query is the odd half of a size-2 domain transform of tau_g1 (circom) or
 * tau_g1[i + domain] - tau_g1[i] (libsnark).  alpha_g1 = alpha_tau_g1[0], beta_g1 = beta_tau_g1[0],
 * delta_g1 = G1, delta_g2 = gamma_g2 = G2.  Canonical affine encodings are unique: the key is, byte for
 * byte, what g16_setup_create_ex mints for toxic = (tau, alpha, beta, 1, 1).  No atomics: the same bytes on
 * every run.  The result is the g16_setup handle of g16_setup_create: g16_setup_key / g16_setup_destroy.
 * Memory: the whole transform is resident on the device, 144 bytes per G1 and 288 per G2 point of
 * max(domain, n_vars), plus 64 bytes of twiddle schedule per domain point.
 * An SRS too short for the domain, a NULL pointer or an unknown reduction: G16_ERR_INVALID.
 *
 * NOT checked HERE: that the SRS is a consistent powers-of-tau string.  g16_setup_from_srs takes the points as
 * they come; a malformed SRS yields a key that means nothing (g16_key_check then still tells whether it is
 * well formed).  Run g16_srs_check (below) once on an SRS that was not minted locally -- it tests every point
 * for the curve and the subgroup and the ratios between neighbours; g16_ptau_open (g16_loaders.h) reads the
 * arrays from a snarkjs .ptau file.
 * NOT built: the transcripts -- section 7 of a .ptau (the ceremony's contributions) and section 10 of a .zkey
 * (see g16_key_contribute) are neither written nor verified.
 *
 * g16_srs_create mints an SRS of 2^log2_domain (tests, synthetic keys) from a trapdoor its caller knows --
 * toxic: tau, alpha, beta as 3 x 4 u64 Montgomery Fr -- with the kernels of g16_setup_create.  The arrays
 * g16_srs_desc_of points at are owned by the handle.
 * g16_setup_from_srs_times: milliseconds the calling thread's last g16_setup_from_srs spent in
 * 0 upload + twiddle schedules, 1 G1 transforms (three of size domain), 2 the G2 transform, 3 the H
 * transform, 4 affine passes, 5 combinations, 6 downloads; entries from 7 on are 0.               */
typedef struct {
  uint32_t n_tau_g1;            /* entries of tau_g1; need >= 2*domain - 1 */
  uint32_t n_tau;               /* entries of tau_g2, alpha_tau_g1, beta_tau_g1; need >= domain */
  const uint8_t *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1;
  uint8_t beta_g2[128];
} g16_srs_desc;
typedef struct g16_srs g16_srs;
g16_status g16_srs_create(int device, uint32_t log2_domain, const uint64_t* toxic, g16_srs** out);
g16_status g16_srs_desc_of(g16_srs* s, g16_srs_desc* out);
void g16_srs_destroy(g16_srs* s);
g16_status g16_setup_from_srs(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct,
                              uint32_t n_vars, uint32_t n_public, uint32_t num_constraints,
                              const g16_srs_desc* srs, int reduction, g16_setup** out);
g16_status g16_setup_from_srs_times(float* ms, uint32_t cap);

/* ---- powers-of-tau validation (not on the proving path) ------------------------------------------ */
/* g16_setup_from_srs and the binding's check_key_circuit build on the SRS they are given: a crafted SRS makes
 * the circuit-binding check vouch for a forged key, one flipped bit makes it reject every honest one.
 * g16_srs_check is the point arithmetic of `snarkjs powersoftau verify` on the GPU: call it once on an SRS
 * that was not minted locally (g16_ptau_open).  Standalone like g16_key_check: no ctx is needed, a ctx alive on
 * the device is left untouched.
 *
 * Structural checks, on EVERY entry handed over (all n_tau_g1 and n_tau of them, not only those some domain
 * needs) and on beta_g2: the predicates, reason bits (G16_KEY_BAD_*) and first-failure rule of g16_key_check;
 * the all-zero encoding is the point at infinity, valid and counted in n_infinity.  Queries: G16_SRS_Q_TAU_G1,
 * _TAU_G2, _ALPHA_TAU_G1, _BETA_TAU_G1 and _SINGLES (index 0 = beta_g2).  bad_out receives the first
 * min(bad_cap, 65536) bad points in ascending (query, index) order -- the same list on every run (scans, no
 * atomics); n_bad counts all of them.
 *
 * Relations, evaluated only when no structural check failed (relations_checked = 0, relations_failed = 0
 * otherwise).  For an array P of m points and its own segment of coefficients rho_0 .. rho_{m-2},
 *   Lo(P) = sum_{i<m-1} rho_i P[i]        Hi(P) = sum_{i<m-1} rho_i P[i+1]
 *   G16_SRS_BASE          tau_g1[0] != the G1 generator or tau_g2[0] != the G2 generator (bytes)
 *   G16_SRS_DEGENERATE    tau_g1[1], tau_g2[1], alpha_tau_g1[0], beta_tau_g1[0] or beta_g2 is infinity
 *                         (tau, alpha or beta = 0)
 *   G16_SRS_PAIR_TAU      e(tau_g1[1], g2) != e(g1, tau_g2[1])            the two arrays hold the same tau
 *   G16_SRS_PAIR_TAU_G1   e(Hi(tau_g1), g2) != e(Lo(tau_g1), tau_g2[1])   every neighbour ratio of tau_g1 is tau
 *   G16_SRS_PAIR_TAU_G2   e(tau_g1[1], Lo(tau_g2)) != e(g1, Hi(tau_g2))   the same for tau_g2
 *   G16_SRS_PAIR_ALPHA    e(Hi(alpha_tau_g1), g2) != e(Lo(alpha_tau_g1), tau_g2[1])
 *   G16_SRS_PAIR_BETA     the same for beta_tau_g1
 *   G16_SRS_PAIR_BETA_G2  e(beta_tau_g1[0], g2) != e(g1, beta_g2)
 * (g1, g2: the standard generators.)  Soundness: every point that reaches a relation is in its prime-order
 * group (G1 has cofactor 1, G2 points are subgroup-tested), so P[i+1] - tau P[i] = d_i G for scalars d_i and
 * a relation holds iff sum rho_i d_i = 0 mod r: with unpredictable rho a string whose neighbours are not all
 * in the one ratio tau passes with probability at most 2^-127 (the small-exponent test of
 * g16_verify_aggregate and g16_key_check).  Whoever knows rho makes two entries cancel (d_j = rho_k,
 * d_k = -rho_j), and the relation holds.
 * rho: ((n_tau_g1 - 1) + 3 (n_tau - 1)) x 2 u64 in the order tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1
 *      (little-endian 128-bit integers, NOT Montgomery), every one non-zero (a zero entry: G16_ERR_INVALID), or
 *      NULL: drawn from the operating system's CSPRNG (a failure to get randomness is G16_ERR_INTERNAL, never
 *      a fixed fallback).
 * n_tau_g1 < 2, n_tau < 2 or a NULL pointer: G16_ERR_INVALID.
 *
 * NOT checked: the section-7 contribution transcript of the ceremony (challenge hashes, proofs of knowledge,
 * the beacon), so nothing is said about WHO knows tau, alpha or beta -- report->ok = 1 means the string is a
 * well formed powers-of-tau string over the standard generators for SOME (tau, alpha, beta) != 0.
 *
 * Memory: the arrays are streamed through two page-locked host slots and two device slots of
 * min(2^18, longest array) points (128 bytes per point plus 16 per coefficient), the copy of one chunk under
 * the kernels of the one before; device use does not grow with the SRS.  G16_SRSCHECK_CHUNK=<points>
 * overrides the chunk (tests).  No atomics: the same report and list on every run.  Returns G16_OK when the
 * check RAN (the verdict is in *report), G16_ERR_NO_DEVICE without a device: there is no CPU fallback.    */
enum { G16_SRS_Q_TAU_G1 = 0, G16_SRS_Q_TAU_G2, G16_SRS_Q_ALPHA_TAU_G1, G16_SRS_Q_BETA_TAU_G1,
       G16_SRS_Q_SINGLES /* index 0: beta_g2 */, G16_SRS_N_QUERIES };
enum { G16_SRS_BASE = 1, G16_SRS_DEGENERATE = 2, G16_SRS_PAIR_TAU = 4, G16_SRS_PAIR_TAU_G1 = 8,
       G16_SRS_PAIR_TAU_G2 = 16, G16_SRS_PAIR_ALPHA = 32, G16_SRS_PAIR_BETA = 64, G16_SRS_PAIR_BETA_G2 = 128 };
typedef struct {
  uint8_t  ok;                 /* 1 iff no bad point and no failed relation */
  uint8_t  relations_checked;  /* 0 when a structural failure made the pairing relations meaningless */
  uint32_t relations_failed;   /* G16_SRS_* */
  uint64_t n_points[G16_SRS_N_QUERIES], n_bad[G16_SRS_N_QUERIES], n_infinity[G16_SRS_N_QUERIES];
  uint32_t n_listed;           /* entries written to bad_out */
} g16_srs_report;
g16_status g16_srs_check(int device, const g16_srs_desc* srs, const uint64_t* rho /* NULL = CSPRNG */,
                         g16_key_bad_point* bad_out, uint32_t bad_cap, g16_srs_report* report);

/* ---- powers-of-tau contributions (not on the proving path) ---------------------------------------- */
/* g16_srs_contribute is the point arithmetic of `snarkjs powersoftau contribute` on the GPU: every entry of an
 * existing string is multiplied through by fresh secrets t, a, b, so that the string of (tau, alpha, beta)
 * becomes the string of (tau t, alpha a, beta b) and nobody knows the product:
 *   tau_g1'[i] = t^i tau_g1[i]              tau_g2'[i] = t^i tau_g2[i]
 *   alpha_tau_g1'[i] = a t^i alpha_tau_g1[i]   beta_tau_g1'[i] = b t^i beta_tau_g1[i]   beta_g2' = b beta_g2
 * Applied to the string whose every entry is a generator (g16_srs_create with toxic = (1, 1, 1)) it is
 * `powersoftau new` followed by the first contribution.  Canonical affine encodings are unique: the result
 * is, byte for byte, what g16_srs_create mints for (tau t, alpha a, beta b).  ALL n_tau_g1 / n_tau entries handed
 * over are multiplied.  Standalone like g16_key_contribute: no ctx is needed, a ctx alive on the device is
 * left untouched.  No atomics: the same bytes on every run.
 *
 * secrets: t, a, b as 3 x 4 u64 Montgomery Fr, each in [1, r) (zero or a non-canonical value:
 *          G16_ERR_INVALID), or NULL: the three are drawn from the operating system's CSPRNG, never returned, and
 *          wiped on the host and on the device before the call returns (a failure to get randomness is
 *          G16_ERR_INTERNAL, never a fixed fallback).
 * Outputs: tau_g1_out n_tau_g1 x 64 bytes, tau_g2_out n_tau x 128, alpha_tau_g1_out / beta_tau_g1_out
 *          n_tau x 64, beta_g2_out 128.  Each may be exactly the matching input array (in place); any other
 *          overlap is unsupported.  A NULL pointer, n_tau_g1 == 0 or n_tau == 0: G16_ERR_INVALID, and nothing is
 *          written.
 * The all-zero encoding (infinity) stays all-zero.  A point off the curve is multiplied like any other and means
 * nothing afterwards: run g16_srs_check first on a string that was not minted locally.
 *
 * Every point has its own full-width scalar c t^i.  The scalars of a chunk are generated on the device; one lane
 * per point then walks the 256 bit positions with a doubling at each and a mixed addition of the affine point
 * predicated on the lane's own bit, and one shared inversion per 8 points brings the chunk back to affine.
 * Memory: the arrays are streamed through two page-locked host slots and two device slots of
 * min(2^18, longest array) points, the copy of chunk k + 1 and the download of chunk k - 1 under the kernels of
 * chunk k; device use does not grow with the SRS.  G16_SRSCONTRIB_CHUNK=<points> overrides the chunk (tests).
 *
 * NOT built: the section-7 transcript of a .ptau (the Blake2b challenge chain, the proofs of knowledge of
 * t, a, b, beacon mode) is neither written nor verified.  Nothing here or in g16_srs_check proves that one
 * string was derived from another: without the transcript any consistent string is a rescaling of any other.
 * g16_srs_check on the result is the whole of what the points alone can tell.
 *
 * g16_srs_contribute_times: milliseconds of device time the calling thread's last g16_srs_contribute spent in
 * 0 uploads, 1 scalar generation, 2 G1 multiplications, 3 G2 multiplications, 4 affine passes, 5 downloads,
 * summed over the chunks (copies run under kernels, so the sum exceeds the wall time); entries from 6 on are 0. */
g16_status g16_srs_contribute(int device, const g16_srs_desc* srs,
                              const uint64_t* secrets /* 3 x 4 u64 Montgomery Fr: t, a, b; NULL = CSPRNG */,
                              uint8_t* tau_g1_out, uint8_t* tau_g2_out, uint8_t* alpha_tau_g1_out,
                              uint8_t* beta_tau_g1_out, uint8_t beta_g2_out[128]);
g16_status g16_srs_contribute_times(float* ms, uint32_t cap);

/* ---- prepared powers of tau: the Lagrange sections (not on the proving path) ----------------------- */
/* `snarkjs powersoftau prepare phase2`: a PREPARED .ptau carries, next to the four monomial arrays, their
 * Lagrange-basis copies for every domain size up to the file's power (sections 12-15); `snarkjs zkey new` builds
 * keys from those and refuses a file without them.  A LAGRANGE SET of power P is four packed arrays in the usual
 * point encoding (Montgomery LE, all-zero = infinity):
 *   tau_g1        (section 12)  levels p = 0 .. P+1   2^(P+2) - 1 points of  64 bytes
 *   tau_g2        (section 13)  levels p = 0 .. P     2^(P+1) - 1 points of 128 bytes
 *   alpha_tau_g1  (section 14)  levels p = 0 .. P     2^(P+1) - 1 points of  64 bytes
 *   beta_tau_g1   (section 15)  levels p = 0 .. P     2^(P+1) - 1 points of  64 bytes
 * Level p starts at point offset 2^p - 1 and holds 2^p points; entry j of level p is
 *   (1 / 2^p) sum_{i < 2^p} omega_p^(-i j) M[i]      natural order, omega_p the 2^p-th root g16_fft_in_place uses
 * with M the array's monomial section (M[i] = tau^i G1 and so on): L_j(tau) G of the domain of size 2^p.  Level
 * P+1 of tau_g1 reads M[2^(P+1) - 1] as infinity: a file holds only 2^(P+1) - 1 powers (g16_ptau_write), and
 * entries a longer g16_srs_desc holds beyond that are dropped.
 * THIS LAYOUT IS WRITTEN FROM KNOWLEDGE OF snarkjs; no snarkjs and no prepared file were on hand to pin it
 * (g16_loaders.h says the same of sections 1-7).  Supported: P <= 27 (level 28 is the last one Fr has a root
 * for); above that G16_ERR_DOMAIN_TOO_LARGE.
 *
 * g16_srs_prepare computes every level of the four arrays with the group transform of g16_setup_from_srs (one
 * copy of the kernels, csrc/gtransform.h).  One level is resident on the device at a time and is downloaded as it
 * finishes: 144 bytes per G1 and 288 per G2 point of the level, 64 per point of the level's input, 2 x 64 bytes
 * of twiddle schedule per pair.  No atomics: the same bytes on every run.  Standalone: no ctx is needed, a ctx
 * alive on the device is left untouched.  An SRS with fewer than 2^(P+1) - 1 / 2^P entries, a NULL pointer:
 * G16_ERR_INVALID, and nothing is written.  g16_srs_prepare_times: milliseconds the calling thread's last
 * g16_srs_prepare spent in the phases of g16_setup_from_srs_times (0 upload + twiddle schedules, 1 G1
 * transforms, 2 G2 transforms, 4 affine passes, 6 downloads; the others 0).
 *
 * g16_srs_lagrange_check verifies a Lagrange set against the monomial arrays it claims to come from -- what
 * nothing else does for sections 12-15 of a downloaded file (g16_srs_check looks at the monomial arrays only).
 * Structural part: every Lagrange point is tested as in g16_srs_check (canonical, on the curve, G2 in the
 * subgroup; infinity is valid and counted); bad_out receives the first min(bad_cap, 65536) bad points sorted by
 * (array, index), query = G16_SRS_Q_TAU_G1 .. _BETA_TAU_G1, index = the position in the section (level p,
 * entry j: 2^p - 1 + j).  Relation part, per array and only when no structural check failed: with a 128-bit
 * rho for every Lagrange point,
 *   sum_p sum_j rho^(p)_j Lambda^(p)[j]  ==  sum_i C_i M[i],      C = sum_p iNTT_{2^p}(rho^(p)) zero-extended
 * -- all levels of an array fold into ONE 128-bit combination over the Lagrange points and ONE full-width
 * combination over the monomial points; the two sums are compared as group elements on the device, no pairing.
 * C is computed on the device with the Fr transform of the witness map.  The pad entry of level P+1 of tau_g1
 * contributes nothing.  relations_failed has bit (1 << array) for an array whose sums differ.
 * Soundness: every point that reaches the relation is in its prime-order group (G1 has cofactor 1, G2 Lagrange
 * points are subgroup-tested, the monomial arrays are expected to have passed g16_srs_check), so a wrong entry
 * differs from the right one by d G for a scalar d and the relation holds iff sum rho d = 0 mod r: with
 * unpredictable rho a set with a wrong entry passes with probability at most 2^-127 (the small-exponent test of
 * g16_srs_check).  Whoever knows rho makes two entries cancel (d_j = rho_k, d_k = -rho_j), and the relation holds.
 * rho: ((2^(P+2) - 1) + 3 (2^(P+1) - 1)) x 2 u64 in array order (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1),
 *      levels ascending (little-endian 128-bit integers, NOT Montgomery), every one non-zero (a zero entry:
 *      G16_ERR_INVALID), or NULL: drawn from the operating system's CSPRNG (a failure to get randomness is
 *      G16_ERR_INTERNAL, never a fixed fallback).
 * A monomial point that is malformed (non-canonical or off the curve) is skipped, not dereferenced further.
 * Memory: the arrays are streamed through two page-locked host slots and two device slots of min(2^18, longest
 * array) points; besides them 32 + 2 x 36 bytes per point of the top level (C and the transform's planes).
 * G16_LAGCHECK_CHUNK=<points> overrides the chunk (tests).  No atomics: the same report and list on every run.
 *
 * g16_setup_from_prepared is g16_setup_from_srs with every transform skipped: the four Lagrange bases are level
 * k (domain = 2^k) of the four arrays, the circom H query is the odd entries of level k+1 of tau_g1 AS IT
 * STANDS, the libsnark H query comes from the monomial tau_g1 as in g16_setup_from_srs, the single points from
 * srs.  lag->power < k: G16_ERR_INVALID.  For k == power the key is byte for byte g16_setup_from_srs's.  For
 * k < power every field but the circom h_query is: g16_setup_from_srs follows the reference's witness map
 * (the transform of tau^0 .. tau^(2n-2) padded with ONE zero), whereas level k+1 below the power is the transform
 * of all 2n powers, tau^(2n-1) included -- what `snarkjs zkey new` takes.  The two queries differ point by point
 * by multiples of tau^(2n-1) G and yield the same proofs, since d = A B - C has degree <= 2n-2 and so no
 * coefficient at x^(2n-1); a pairing comparison of the two H queries (g16_contribution_check against a key
 * rebuilt the other way) does see the difference.  Its phase timer is g16_setup_from_srs_times.              */
typedef struct {
  uint32_t power;
  const uint8_t *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1;
} g16_srs_lagrange_desc;
enum { G16_LAGRANGE_N_ARRAYS = 4 };  /* indexed by G16_SRS_Q_TAU_G1 .. G16_SRS_Q_BETA_TAU_G1 */
typedef struct {
  uint8_t  ok;                 /* 1 iff no bad point and no failed relation */
  uint8_t  relations_checked;  /* 0 when a structural failure made the relations meaningless */
  uint32_t relations_failed;   /* bit (1 << array) */
  uint64_t n_points[G16_LAGRANGE_N_ARRAYS], n_bad[G16_LAGRANGE_N_ARRAYS], n_infinity[G16_LAGRANGE_N_ARRAYS];
  uint32_t n_listed;           /* entries written to bad_out */
} g16_srs_lagrange_report;
g16_status g16_srs_prepare(int device, const g16_srs_desc* srs, uint32_t power, uint8_t* tau_g1_out,
                           uint8_t* tau_g2_out, uint8_t* alpha_tau_g1_out, uint8_t* beta_tau_g1_out);
g16_status g16_srs_prepare_times(float* ms, uint32_t cap);
g16_status g16_srs_lagrange_check(int device, const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag,
                                  const uint64_t* rho /* NULL = CSPRNG */, g16_key_bad_point* bad_out,
                                  uint32_t bad_cap, g16_srs_lagrange_report* report);
g16_status g16_setup_from_prepared(int device, const g16_csr* at, const g16_csr* bt, const g16_csr* ct,
                                   uint32_t n_vars, uint32_t n_public, uint32_t num_constraints,
                                   const g16_srs_desc* srs, const g16_srs_lagrange_desc* lag, int reduction,
                                   g16_setup** out);

/* ---- arkworks serialization (not on the proving path) ---------------------------------------------- */
/* Every other entry point takes and returns points in the .zkey encoding (32-byte little-endian MONTGOMERY
 * coordinates, affine x|y, all-zero = infinity).  arkworks exchanges keys, verifying keys and proofs in
 * ark-serialize's canonical form (CanonicalSerialize::serialize_compressed / serialize_uncompressed); these calls
 * translate between the two on the GPU, so that a compressed ProvingKey<Bn254> is loaded without one square root
 * (and, on G2, one subgroup test) per point on the CPU.
 *
 * The format (BN254, ark-serialize 0.4 / 0.5):
 *   Fq       32 bytes: the CANONICAL integer, little-endian (q has 254 bits: two flag bits are free); Fq2 = c0 | c1
 *   flags    in the top two bits of the LAST byte of a point's record: 0x80 = "y is negative", 0x40 = infinity,
 *            both = invalid.  "Negative" is y > -y on canonical integers: y > (q-1)/2 in Fq; in Fq2 lexicographic
 *            with c1 FIRST (c1 > (q-1)/2, or c1 = 0 and c0 > (q-1)/2)
 *   G1       compressed: x with flags, 32 bytes; uncompressed: x, then y with flags, 64 bytes
 *   G2       compressed: x.c0 | x.c1 with flags, 64 bytes; uncompressed: x.c0 | x.c1 | y.c0 | y.c1 with flags, 128
 *   infinity all-zero coordinates + 0x40.  The writer sets the sign bit in uncompressed form too, the reader
 *            ignores it there
 *   Vec<T>   u64 little-endian length, then the items
 *   VerifyingKey  alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1: Vec<G1>
 *   ProvingKey    vk, beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query, l_query (h BEFORE l; four Vecs)
 *   Proof         a (G1), b (G2), c (G1): 128 bytes compressed, 256 uncompressed
 *
 * g16_points_from_ark   what G1Affine / G2Affine::deserialize_with_mode does for n points: in = n records in the
 *   form above, out = n packed points.  Per point, the FIRST test that fails is its reason (g16_key_check's rule):
 *     G16_KEY_BAD_ENCODING      both flag bits, or the infinity flag with any other bit of the record set
 *                               (DEVIATION: arkworks ignores those bits; no canonical writer produces them)
 *     G16_KEY_BAD_NONCANONICAL  a coordinate, flags masked off, is >= q
 *     G16_KEY_BAD_OFF_CURVE     compressed: x^3 + b has no square root (b = 3, on the twist 3 / (9 + i));
 *                               uncompressed: y^2 != x^3 + b -- ALWAYS tested, also where arkworks' Validate::No
 *                               would skip it
 *     G16_KEY_BAD_SUBGROUP      G2 with G16_ARK_VALIDATE only: [r] P != infinity
 *   The output record of a bad point is all-zero; a well-formed infinity record decodes to the all-zero record
 *   with reason 0.  reason_out: n bytes or NULL; *n_bad counts EVERY bad point.  Returns G16_OK when it RAN.
 * g16_points_to_ark     serialize_with_mode: Montgomery -> canonical, the sign flag, the infinity encoding.  The
 *   points are not tested for the curve; a stored word >= q is bad (its record is all-zero) and makes the call
 *   return G16_ERR_INVALID with the count in *n_bad.
 * group: G16_POINT_G1 / _G2.  flags: G16_ARK_COMPRESSED | G16_ARK_VALIDATE (Compress::Yes, Validate::Yes).
 * Strides in bytes between consecutive records, 0 = dense; in and out must not overlap.  n == 0: G16_OK.
 * One lane per point: a compressed G1 point costs one 252-bit exponentiation in Fq, a G2 point two (the norm
 * method, no inversion); a validated G2 point is dominated by the [r] P test g16_key_check pays as well.
 * Arrays stream through two page-locked host slots and two device slots of min(2^18, n) points
 * (G16_ARKSER_CHUNK=<points> overrides, tests).  No atomics: the same bytes and reasons on every run.
 * Standalone like g16_key_check: no ctx is needed, a ctx alive on the device is left untouched.
 * G16_ERR_NO_DEVICE without a device: there is no CPU fallback.
 *
 * g16_ark_proofs_read / _write   n x Proof::deserialize_with_mode / serialize_with_mode: n arkworks proofs (128 or
 *   256 bytes each) <-> n x G16_PROOF_BYTES, three strided codec calls.  reason_out: n x 3 bytes (a, b, c) or NULL.
 *   A container call like the key calls: g16_ark_proofs_read returns G16_ERR_IO when ANY point fails to decode
 *   (the message names the first proof, point and reason; *n_bad, reason_out and the zeroed records are still
 *   filled in), so a verifier that looks at the status alone never takes a zeroed point into its batch.
 * g16_ark_pk_read    ProvingKey::<Bn254>::deserialize_with_mode from memory.  n_vars = len(a_query), n_public =
 *   len(gamma_abc_g1) - 1, domain_size = the smallest power of two >= len(h_query); the H array is padded with
 *   infinity up to domain_size (a LibsnarkReduction key has domain_size - 1 points; the degenerate libsnark key
 *   of domain 2 has ONE H point and therefore reads back with domain_size 1).  The fixed points of a container are
 *   decoded in one codec call per group, every array in one of its own.  g16_ark_pk_key hands out
 *   arrays owned by the handle, valid until g16_ark_pk_close.
 * g16_ark_pk_write   ProvingKey::serialize_with_mode into out (g16_ark_pk_size bytes); the first h_len <=
 *   domain_size entries of h_query are written, so a libsnark key round-trips to the same bytes.
 * g16_ark_vk_read / _write   the same for VerifyingKey (g16_ark_vk_size bytes); ic_out receives gamma_abc_g1
 *   (g16_ark_vk_layout in g16_loaders.h tells how many points), vk->ic points at it afterwards.
 * G16_ERR_IO with a message in g16_loader_last_error: a truncated blob, a length prefix that overruns it,
 * inconsistent array lengths, trailing bytes (the layout walk, g16_loaders.h), or a point that fails to decode --
 * the message names the array, the index and the reason.
 *
 * NOT claimed: byte compatibility with arkworks rests on the description above and on known arkworks encodings
 * of single points (the generators, their negatives, infinity) that the tests pin; no arkworks build was
 * available to cross-check a whole ProvingKey blob.  ark-serialize 0.3 (a different flag layout) is not supported. */
enum { G16_KEY_BAD_ENCODING = 8 };   /* per-point reason bit, next to G16_KEY_BAD_* above */
enum { G16_POINT_G1 = 0, G16_POINT_G2 = 1 };
enum { G16_ARK_COMPRESSED = 1, G16_ARK_VALIDATE = 2 };
g16_status g16_points_from_ark(int device, int group, uint32_t flags, const uint8_t* in, size_t in_stride,
                               uint64_t n, uint8_t* out, size_t out_stride, uint8_t* reason_out, uint64_t* n_bad);
g16_status g16_points_to_ark(int device, int group, uint32_t flags, const uint8_t* in, size_t in_stride,
                             uint64_t n, uint8_t* out, size_t out_stride, uint64_t* n_bad);
g16_status g16_ark_proofs_read(int device, uint32_t flags, const uint8_t* in, uint64_t n, uint8_t* proofs_out,
                               uint8_t* reason_out, uint64_t* n_bad);
g16_status g16_ark_proofs_write(int device, uint32_t flags, const uint8_t* proofs, uint64_t n, uint8_t* out,
                                uint64_t* n_bad);
typedef struct g16_ark_pk g16_ark_pk;
uint64_t g16_ark_pk_size(uint32_t flags, uint64_t n_vars, uint64_t n_public, uint64_t h_len);
g16_status g16_ark_pk_read(int device, uint32_t flags, const uint8_t* data, size_t len, g16_ark_pk** out);
g16_status g16_ark_pk_key(const g16_ark_pk* h, g16_key_desc* key, g16_vk_desc* vk);
void g16_ark_pk_close(g16_ark_pk* h);
g16_status g16_ark_pk_write(int device, uint32_t flags, const g16_key_desc* key, const g16_vk_desc* vk,
                            uint64_t h_len, uint8_t* out, size_t cap);
uint64_t g16_ark_vk_size(uint32_t flags, uint64_t n_public);
g16_status g16_ark_vk_read(int device, uint32_t flags, const uint8_t* data, size_t len, g16_vk_desc* vk,
                           uint8_t* ic_out, uint32_t ic_cap);
g16_status g16_ark_vk_write(int device, uint32_t flags, const g16_vk_desc* vk, uint8_t* out, size_t cap);

/* ---- proof re-randomisation (not on the proving path) ----------------------------------------------- */
/* g16_proofs_rerandomize is ark_groth16::Groth16::rerandomize_proof(vk, proof, rng) for n_proofs proofs under
 * one key, one GPU lane per proof.  For a proof (A, B, C), the key's delta in G2, and r1 != 0, r2 in Fr:
 *   A' = r1^-1 A        B' = r1 B + (r1 r2) delta        C' = C + r2 A
 * (A', B', C') verifies for exactly the public inputs (A, B, C) verifies for and, for uniform (r1, r2), is
 * uniformly distributed among the proofs that do: a relayer makes a proof unlinkable to the one it received
 * without knowing the witness.  An invalid proof stays invalid.  Only delta_g2 of the key is used.
 *
 * proofs / proofs_out: n_proofs x G16_PROOF_BYTES (A | B | C as g16_prove writes them).  proofs_out may be
 *          exactly proofs (in place); any other overlap is unsupported.
 * scalars: n_proofs x 2 x 4 u64 Montgomery Fr, (r1, r2) per proof, r1 in [1, r), r2 in [0, r).  r1 == 0, or any
 *          value whose words are not below r: G16_ERR_INVALID, decided before any output byte is written.
 *          NULL: every r1 is drawn uniformly from [1, r) and every r2 from [0, r) from the operating system's
 *          CSPRNG by rejection; a failure to get randomness is G16_ERR_INTERNAL, never a fixed fallback.
 *          Given or drawn, the scalars and everything derived from them are wiped on the host and zeroed on
 *          the device before the call returns; drawn scalars are never returned.
 * ok_out:  NULL, or n_proofs bytes: 1 where proof i passed the structural tests, applied before any arithmetic
 *          on it: every stored coordinate canonical (< q), A and C on the curve, B on the twist.  A proof that
 *          fails gets ok_out[i] = 0 and an all-zero 256-byte record; its neighbours are unaffected.
 *          NOT applied: the prime-order subgroup test of B ([r] B = infinity, which g16_verify_batch applies).
 *          It would cost a third G2 ladder per proof, and the map above is well defined on the whole twist: a B
 *          outside G2 is transformed like any other (ok = 1) and the result fails verification as the input
 *          does.  A caller that forwards untrusted proofs verifies them first or afterwards; ok = 1 says
 *          nothing about validity.  delta_g2 comes from the caller's own key and is not tested.
 * The all-zero encoding is the point at infinity and is an operand like any other, in the proof or as delta;
 * equal and opposite operands (B = +-delta, C = +-A) take the doubling and cancelling branches of the addition.
 * n_proofs == 0: G16_OK, nothing is written.  A NULL where data is needed (delta_g2, proofs, proofs_out), a
 * device out of range, more than 2^24 - 1 proofs: G16_ERR_INVALID, nothing is written.
 *
 * g16_proofs_rerandomize_keys: proofs under MANY keys in the same launches.  Group k is counts[k] consecutive
 * proofs under delta_g2s[k] (n_keys x 128 bytes); proofs, scalars, proofs_out and ok_out run over all
 * N = sum_k counts[k] proofs, group after group.  Groups may be empty and the same delta may appear twice.  The
 * result is the concatenation of the one-key calls on the groups with the matching scalar slices; the number
 * of launches, allocations and copies does not depend on n_keys (g16_proofs_rerandomize is its n_keys == 1
 * case).  n_keys == 0 or N == 0: G16_OK, nothing is written.  counts NULL: G16_ERR_INVALID.
 *
 * One lane per proof: A' and C' are two 256-position ladders over Fq with a mixed addition of the affine A on
 * the lane's own bit (C is added at the end); B' is ONE joint ladder over Fq2 -- one doubling chain, a mixed
 * addition of B on the bit of r1 and one of delta on the bit of r1 r2 -- with delta, the same for every lane of
 * a block, held outside the lanes' registers.  r1^-1 is computed on the device.  One shared inversion per 8
 * points brings the results back to affine.  The G1 and the G2 kernels run on two streams.  Standalone like
 * g16_verify_batch: no ctx is needed, a ctx alive on the device is left untouched.  No atomics: with given
 * scalars the same bytes on every run.  G16_ERR_NO_DEVICE without a device: there is no CPU fallback.
 *
 * g16_proofs_rerandomize_times: milliseconds of device time the calling thread's last call spent in 0 upload,
 * 1 structural tests + scalar preparation, 2 G1 ladders, 3 the G2 ladder, 4 affine passes (G1 + G2), 5 download;
 * 2 and 3 run side by side, so the sum exceeds the wall time; entries from 6 on are 0. */
g16_status g16_proofs_rerandomize(int device, const uint8_t delta_g2[128], const uint8_t* proofs, uint32_t n_proofs,
                                  const uint64_t* scalars /* n x 2 x 4 u64 Montgomery Fr (r1, r2), or NULL */,
                                  uint8_t* proofs_out, uint8_t* ok_out /* n bytes or NULL */);
g16_status g16_proofs_rerandomize_keys(int device, const uint8_t* delta_g2s /* n_keys x 128 */, const uint32_t* counts,
                                       uint32_t n_keys, const uint8_t* proofs, const uint64_t* scalars,
                                       uint8_t* proofs_out, uint8_t* ok_out);
g16_status g16_proofs_rerandomize_times(float* ms, uint32_t cap);   /* per-phase device ms of the last call on this thread */

/* ---- low-latency verification: a prepared verifying key (not on the proving path) -------------------- */
/* g16_verify_batch and g16_verify_aggregate check a proof in ONE lane: right for tens of thousands of proofs, some
 * hundred milliseconds for one.  These calls check a proof in one WORKGROUP, the Fq12 arithmetic spread over its 64
 * lanes, under a key prepared once.
 *
 * g16_pvk_create is Groth16::process_vk: a device-resident handle with -alpha, beta, gamma, delta, the IC row, the
 *   Frobenius constants, the Miller value of (beta, -alpha) and the line coefficients of gamma and of delta for every
 *   step of the Miller loop (ark-ec's G2Prepared).  Unlike g16_verify_batch it TESTS the key: every coordinate
 *   canonical, alpha and the IC points on the curve, beta, gamma and delta on the twist and in G2.  A key that fails:
 *   G16_ERR_INVALID, and g16_last_error(NULL) names the point (alpha_g1, beta_g2, gamma_g2, delta_g2,
 *   gamma_abc_g1[j]) and the reason.  A point at infinity is accepted; its pair contributes 1.
 * g16_pvk_alpha_beta: the stored Miller value of (beta, -alpha), 12 Fq: out[32 i ..] = the coefficient of w^i in
 *   Fq12 = Fq[w] / (w^12 - 18 w^6 + 82), 8 x u32 Montgomery.  Its final exponentiation is e(-alpha, beta).
 * g16_verify_prepared is verify_with_processed_vk for n_proofs >= 0 proofs.  proofs, public_inputs and every rule
 *   are g16_verify_batch's, and ok_out[i] is exactly its verdict under the same key: the structural tests come
 *   first (canonical words, A and C on the curve, B on the twist and in the subgroup), a malformed proof gets 0 and
 *   its neighbours are untouched.  n_proofs == 0: G16_OK, nothing is written.  Calls on one handle serialise on a
 *   mutex in the handle; different handles run side by side.  The call uses the handle's own two streams and
 *   synchronises THOSE, not the device: a prover on the same card is not stalled.  Per proof: X = IC_0 + sum pub_j
 *   IC_{j+1} with one lane per term, ONE Miller loop for (A, B), (-X, gamma), (-C, delta) (64 squarings; the lines
 *   of gamma and delta from the handle's tables, those of B from inversion-free projective steps), the stored
 *   (beta, -alpha) value, one final exponentiation with one inversion; the subgroup test of B (psi(B) = [6 x^2] B,
 *   127 bits) runs beside all of that on the second stream.
 * g16_pairing_check: *ok_out = 1 iff prod_i e(P_i, Q_i) = 1 for 1 <= n_pairs <= 16 pairs, every pair through the
 *   on-the-fly line path in one workgroup, under the same structural tests (a malformed point: *ok_out = 0); a pair
 *   with an infinite side contributes 1.  Standalone: no handle.
 * g16_verify_prepared_times: device milliseconds of the calling thread's last g16_verify_prepared in 0 upload,
 *   1 prepared inputs, 2 the tests of B (beside 1 and 3), 3 Miller loop + final exponentiation, 4 download; 5 is the
 *   preparation kernel of the thread's last g16_pvk_create; entries from 6 on are 0.
 * Not here: fixed-base tables for IC in the handle (they would remove the ladder of X), multi-device forms.
 * G16_ERR_NO_DEVICE without a device: there is no CPU fallback.                                                  */
typedef struct g16_pvk g16_pvk;
g16_status g16_pvk_create(int device, const g16_vk_desc* vk, g16_pvk** out);
void g16_pvk_destroy(g16_pvk* pvk);
g16_status g16_pvk_alpha_beta(const g16_pvk* pvk, uint8_t out[384]);
g16_status g16_verify_prepared(g16_pvk* pvk, const uint8_t* proofs, const uint64_t* public_inputs, uint32_t n_proofs,
                               uint8_t* ok_out);
g16_status g16_pairing_check(int device, const uint8_t* g1 /* n x 64 */, const uint8_t* g2 /* n x 128 */,
                             uint32_t n_pairs, uint8_t* ok_out);
g16_status g16_verify_prepared_times(float* ms, uint32_t cap);

/* ---- prepared inputs: arkworks' prepare_inputs / verify_proof_with_prepared_inputs ----------------------- */
/* g16_pvk_prepare_inputs: out[64 i ..] = X_i = IC_0 + sum_j pub_ij IC_{j+1} for n input vectors (public_inputs as
 *   g16_verify_prepared's), a packed affine G1 point (Montgomery; all-zero = infinity): the sum g16_verify_prepared
 *   forms per proof, normalised.  n == 0: G16_OK, nothing is written.
 * g16_verify_prepared_inputs: g16_verify_prepared with X_i GIVEN (prepared: n x 64 bytes) instead of computed: the
 *   input ladder is skipped, every other rule and the verdicts are g16_verify_prepared's.  A prepared point with a
 *   non-canonical word or off the curve gives ok_out[i] = 0 for that proof only.                                    */
g16_status g16_pvk_prepare_inputs(g16_pvk* pvk, const uint64_t* public_inputs, uint32_t n, uint8_t* out /* n x 64 */);
g16_status g16_verify_prepared_inputs(g16_pvk* pvk, const uint8_t* proofs, const uint8_t* prepared /* n x 64 */,
                                      uint32_t n_proofs, uint8_t* ok_out);

/* ---- pairing values: elements of GT (not on the proving path) ------------------------------------------------- */
/* Every other pairing call answers "is this product 1?".  These return the VALUE, multiply and raise such values and
 * carry them to and from the forms other software reads.
 *
 * Convention: a pairing value is ML(Q, P)^((q^12 - 1) / r * m) with m = 2 x (6 x^2 + 3 x + 1), x = 4965661367192848881:
 *   the m-th power of the "plain" reduced pairing.  m is the cofactor of the Fuentes-Castaneda hard part, gcd(m, r) = 1,
 *   and this is the value arkworks' Bn254::pairing and snarkjs (vk_alphabeta_12) give.
 * Flat form: 12 x 32 bytes, the coefficient of w^i in Fq12 = Fq[w] / (w^12 - 18 w^6 + 82) at 32 i, 8 x u32 Montgomery
 *   (g16_pvk_alpha_beta's basis).  Every gt / gt_out below is in it, 384 bytes per element.
 * Ark form: ark-ff's Fq12::serialize, 384 bytes, 12 canonical little-endian Fq in tower order: for i < 6 the Fq2
 *   coefficient (a_i + 9 a_{i+6}, a_{i+6}) is slot 3 (i & 1) + (i >> 1) of six 64-byte slots.  snarkjs' JSON nests
 *   the same order as [2][3][2] decimal strings.
 *
 * g16_pairing_products: gt_out[i] = prod_{p in offsets[i] .. offsets[i+1]} e(g1[p], g2[p]) for n_products products,
 *   one workgroup each, 0 to 16 pairs per product in ONE Miller loop (offsets: n_products + 1 entries from 0, non-
 *   decreasing).  The structural rules are g16_pairing_check's: every word canonical, P on the curve, Q on the twist
 *   and in G2; a pair with an infinite side contributes 1; an empty product is 1.  A product with a malformed point
 *   is written as the all-zero element (not a member of GT) with ok_out[i] = 0, its neighbours are untouched.
 *   ok_out may be NULL.  More than 16 pairs in a product: G16_ERR_INVALID, g16_last_error(NULL) names the product.
 * g16_gt_multiexp: gt_out[i] = prod_{j in offsets[i] .. offsets[i+1]} gt[j]^scalars[j], one workgroup per output,
 *   plain square-and-multiply in input order: the bytes depend on the input alone.  scalars: 4 x u64 little-endian
 *   canonical integers, each BELOW r -- a scalar >= r is REFUSED (G16_ERR_INVALID, g16_last_error(NULL) names it),
 *   never reduced silently.  The inverse of an element of GT is its (r - 1)-th power.  The inputs are not tested.
 * g16_gt_to_ark / g16_gt_from_ark: the codec, one lane per element.  Decoding tests every word against q; with
 *   validate != 0 it also tests membership, g^r = 1 (the same square-and-multiply with the exponent r).
 *   reason_out[i] (may be NULL): 0 accepted, G16_KEY_BAD_NONCANONICAL, G16_KEY_BAD_SUBGROUP (outside GT); a refused
 *   element is written as all-zero.  The status stays G16_OK.
 * g16_pvk_alpha_g1_beta_g2: e(alpha_g1, beta_g2) of a prepared key, arkworks' PreparedVerifyingKey::alpha_g1_beta_g2,
 *   flat form; computed on first use and kept.  (g16_pvk_alpha_beta is the raw Miller value of (beta, -alpha).)
 * g16_gt_times: device milliseconds of the calling thread's last call above in 0 upload, 1 the G2 tests (products
 *   only; beside 2 on a second stream), 2 kernels, 3 download; entries from 4 on are 0.
 * n == 0: G16_OK and nothing is written.  Each call has its own streams and synchronises those, not the device.
 * G16_ERR_NO_DEVICE without a device: there is no CPU fallback.                                                   */
g16_status g16_pairing_products(int device, const uint8_t* g1, const uint8_t* g2, const uint32_t* offsets,
                                uint32_t n_products, uint8_t* gt_out /* n x 384 */, uint8_t* ok_out);
g16_status g16_gt_multiexp(int device, const uint8_t* gt, const uint64_t* scalars, const uint32_t* offsets,
                           uint32_t n_out, uint8_t* gt_out);
g16_status g16_gt_to_ark(int device, const uint8_t* gt, uint32_t n, uint8_t* out);
g16_status g16_gt_from_ark(int device, const uint8_t* in, uint32_t n, int validate, uint8_t* gt_out, uint8_t* reason_out);
g16_status g16_pvk_alpha_g1_beta_g2(const g16_pvk* pvk, uint8_t out[384]);
g16_status g16_gt_times(float* ms, uint32_t cap);

/* ---- MSM over caller-supplied bases (ark-ec VariableBaseMSM::msm / msm_bigint) ---------------- */
/* g16_msm_g1 / g16_msm_g2 run the MSM engine over the queries of a resident proving key.  The calls below point the
 * same engine -- the digit sort, the entry-balanced accumulation, its fix-up and the bucket reduction, unchanged -- at
 * any bases.
 * Handle: g16_msm_bases_create uploads n packed affine points (64 / 128 bytes, Montgomery, all-zero = infinity: the
 *   zkey encoding of every other call; group = G16_GROUP_G1 / G16_GROUP_G2), converts them to the engine's internal
 *   form and fills the precomputed planes.  n <= 2^27.  flags: G16_MSM_POINTS_DEVICE when `points` is device memory.
 *   opt may be NULL (all defaults).  opt->window_bits <= 0: the window msm_make_config picks for n.  opt->planes <= 0:
 *   as many planes as fit the device memory free at the call (the plan of g16_ctx_create), 1: no precomputation.
 *   opt->max_batch (<= 0: 1): scalar vectors handled by ONE sort, accumulation and reduction; the sort and partial-sum
 *   workspaces are sized for it (it is lowered where max_batch x n x windows would not fit a 32-bit entry index;
 *   g16_msm_bases_info out[6] has the value in use).  opt->validate != 0: every point is tested first with the
 *   predicates of g16_key_check -- canonical words, the curve, and for G2 the prime-order subgroup; the first point
 *   that fails gives G16_ERR_INVALID and g16_last_error(NULL) names its index and reason.  Without it the points are
 *   taken as they come (as g16_setup_from_srs takes an SRS).
 * g16_msm_bases_info: out[0] = group, [1] = n, [2] = window bits c, [3] = windows W, [4] = planes, [5] = bucket sets D,
 *   [6] = vectors per chunk, [7] = 1 when the points were validated.
 * g16_msm: out[k] = sum_{i < len} scalars[k * stride + i] * points[i] for k < count; len <= n, stride >= len (in
 *   scalars; ignored for count == 1).  flags: G16_MSM_SCALARS_CANONICAL -- 32-byte little-endian integers below r
 *   instead of 4 x u64 Montgomery Fr; they go through the conversion kernel of g16_fr_convert, and a value >= r gives
 *   G16_ERR_INVALID with its index (vector * len + element) in g16_last_error(NULL).  G16_MSM_SCALARS_DEVICE: `scalars`
 *   is device memory on the handle's device.  out: count affine points of 64 / 128 bytes on the host, all-zero =
 *   infinity (also the answer for len == 0).  Vectors are processed in chunks of the handle's batch.  One call in
 *   flight per handle (the handle holds a mutex); several handles run side by side.  The bytes do not depend on
 *   planes, window, batch or chunking: affine points have one encoding.
 * g16_msm_once: bases used once -- the planes = 1 configuration (as many bucket sets as windows, folded by the Horner
 *   kernel): no plane is computed and nothing allocated outlives the call.  flags as above (both kinds).           */
enum { G16_GROUP_G1 = 0, G16_GROUP_G2 = 1 };
enum { G16_MSM_SCALARS_CANONICAL = 1, G16_MSM_SCALARS_DEVICE = 2, G16_MSM_POINTS_DEVICE = 4 };
typedef struct {
  int window_bits;
  int planes;
  int max_batch;
  int validate;
} g16_msm_options;
typedef struct g16_msm_bases g16_msm_bases;
g16_status g16_msm_bases_create(int device, int group, const void* points, size_t n, uint32_t flags,
                                const g16_msm_options* opt, g16_msm_bases** out);
void g16_msm_bases_destroy(g16_msm_bases* h);
g16_status g16_msm_bases_info(const g16_msm_bases* h, uint32_t out[8]);
g16_status g16_msm(g16_msm_bases* h, const void* scalars, size_t len, size_t count, size_t stride, uint32_t flags,
                   uint8_t* out);
g16_status g16_msm_once(int device, int group, const void* points, const void* scalars, size_t n, uint32_t flags,
                        uint8_t* out);

/* ---- division by (X - z) ---------------------------------------------------------------------------------------- */
/* For each of count polynomials p_k of n coefficients (coeffs[k * n + i] is the coefficient of X^i) and its own point
 * z[k]:  p_k(X) = q_k(X) (X - z_k) + y_k.  quot_out: count x (n - 1) coefficients, rem_out: count values y_k = p_k(z_k).
 * 1 <= n <= 2^27.  Everything is 4 x u64 Montgomery Fr unless flags has G16_MSM_SCALARS_CANONICAL (then coeffs and z
 * are 32-byte little-endian integers below r, refused with their index otherwise; the outputs stay Montgomery).
 * G16_MSM_SCALARS_DEVICE: coeffs and quot_out are device memory (z and rem_out stay on the host).
 * The suffix recurrence s_i = a_i + z s_(i+1) in three phases: every thread runs Horner over its own run of
 * G16_POLY_RUN coefficients; the run values are combined across the G16_POLY_BLOCK threads of a block and then
 * across blocks with the weights z^RUN and z^(RUN x BLOCK); a second pass over each run, seeded with the carry from
 * the right, writes the quotient.  No atomics, a fixed combination order: the same bytes on every run.            */
#define G16_POLY_RUN 8
#define G16_POLY_BLOCK 256
g16_status g16_poly_divide_linear(int device, const void* coeffs, size_t n, size_t count, const void* z,
                                  uint32_t flags, void* quot_out, uint64_t* rem_out);

/* ---- KZG on a powers-of-tau string ------------------------------------------------------------------------------ */
/* Key: an MSM handle over srs->tau_g1[0, max_len) (max_len == 0: all n_tau_g1 entries) with planes -- a commitment key
 *   is reused -- and tau_g2[1].  opt as for g16_msm_bases_create (validate is ignored).  The SRS is taken as it comes:
 *   g16_srs_check is the call that verifies one, run it once on a string that was not minted locally.
 * g16_kzg_commit: g16_msm on the key's bases: out[k] = p_k(tau) G for coefficient vectors of len <= max_len.
 * g16_kzg_open: for each polynomial and its point z[k] (count x 32 bytes on the host, in the scalars' encoding):
 *   y_out[k] = p_k(z_k) (4 x u64 Montgomery) and proof_out[k] = q_k(tau) G (64 bytes).  The division above leaves the
 *   quotients in device memory and the chunked MSM reads them there: count x (32 + 64) bytes come back to the host.
 *   len == 1: the proof is the point at infinity.  len == 0 or len > max_len: G16_ERR_INVALID.
 * g16_kzg_verify: ONE verdict for n openings (C_i, z_i, y_i, pi_i):
 *     e(sum_i rho_i (C_i - y_i G + z_i pi_i), G2) = e(sum_i rho_i pi_i, tau_g2)
 *   two one-shot G1 MSMs, the scalar sum_i rho_i y_i and one two-pair pairing check.  commitments, proofs: n x 64
 *   bytes; z, y: n x 4 u64 Montgomery Fr; tau_g2: tau_g2[1] of the string.  rho: n x 2 u64 (128-bit integers, every
 *   one non-zero, else G16_ERR_INVALID) or NULL: drawn from the operating system's CSPRNG as g16_verify_aggregate
 *   does (no fixed fallback); a wrong opening passes with probability at most 2^-127 when rho is unpredictable.
 *   Commitments and proofs are tested for canonical words and the curve first, tau_g2 for the twist and the subgroup;
 *   any failure makes *ok_out = 0.  n == 0: *ok_out = 1.  No per-item verdicts: a caller bisects.
 * g16_kzg_times: device milliseconds of the calling thread's last open / verify: 0 upload + conversion, 1 division
 *   (open) or scalar preparation (verify), 2 MSM, 3 download (open) or pairing check (verify); from 4 on 0.
 * NOT built: multi-point openings, per-item verdicts, anything PLONK.                                              */
typedef struct g16_kzg_key g16_kzg_key;
g16_status g16_kzg_key_create(int device, const g16_srs_desc* srs, size_t max_len, const g16_msm_options* opt,
                              g16_kzg_key** out);
void g16_kzg_key_destroy(g16_kzg_key* k);
g16_status g16_kzg_key_info(const g16_kzg_key* k, uint32_t out[8]);
g16_status g16_kzg_commit(g16_kzg_key* k, const void* coeffs, size_t len, size_t count, size_t stride, uint32_t flags,
                          uint8_t* out);
g16_status g16_kzg_open(g16_kzg_key* k, const void* coeffs, size_t len, size_t count, size_t stride, const void* z,
                        uint32_t flags, uint64_t* y_out, uint8_t* proof_out);
g16_status g16_kzg_verify(int device, const uint8_t tau_g2[128], const uint8_t* commitments, const uint64_t* z,
                          const uint64_t* y, const uint8_t* proofs, size_t n, const uint64_t* rho, uint8_t* ok_out);
g16_status g16_kzg_times(float* ms, uint32_t cap);

/* ---- loaders (host side, C++): see g16_loaders.h ---------------------------------------------- */

#ifdef __cplusplus
}
#endif
#endif /* G16_AMD_H */
