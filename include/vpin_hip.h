/*
 * vpin_hip.h -- C ABI of the MI355X (gfx950) Spartan sat-proof hot path.
 *
 * This is the drop-in boundary for vt-asaplab/vPIN's prover.  The reference has no
 * FFI seam of its own; the seam is the set of plain Rust functions that
 * vPIN_proof_generation/src/commit_test.rs calls into libspartan (SURVEY.md 8(b),
 * rows B1-B5).  Each entry point below names the reference function it replaces
 * (paths relative to src/proof_generation/).  INTEGRATION.md shows the Rust `extern "C"`
 * block a vPIN maintainer would add.
 *
 * Conventions
 *  - A scalar is 32 bytes: the reference's in-memory `Scalar([u64;4])`, little-endian
 *    limbs, Montgomery form with R = 2^256 (Spartan/src/scalar/ristretto255.rs:199-200).
 *    A table is a flat array of scalars == the memory image of a Vec<Scalar>.
 *  - A group element crosses as 128 bytes of extended twisted-Edwards coordinates
 *    (X,Y,Z,T; each 32-byte canonical little-endian mod 2^255-19) or as a 32-byte
 *    compressed ristretto255 encoding (curve25519-dalek CompressedRistretto).
 *  - Every call returns 0 on success or a negative VPIN_E* code; nothing aborts across
 *    the boundary.  The caller owns host buffers; the library owns device memory behind
 *    opaque handles.  One host thread drives one ctx (the reference's protocol loop is
 *    single-threaded); calls are synchronous from the caller's point of view.
 *  - There is NO CPU fallback: every entry point fails with VPIN_ENODEV when no gfx950
 *    device is usable.
 */
#ifndef VPIN_HIP_H
#define VPIN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPIN_OK 0
#define VPIN_EINVAL (-1)  /* bad argument (null handle, length not a power of two, ...) */
#define VPIN_ENODEV (-2)  /* no usable HIP device */
#define VPIN_ENOMEM (-3)  /* device or host allocation failed */
#define VPIN_EHIP (-4)    /* a HIP runtime call failed; see vpin_last_error() */
#define VPIN_ESHAPE (-5)  /* operand shapes do not match (the reference would assert) */
#define VPIN_EVERIFY (-6) /* a verifier rejected the proof (ProofVerifyError / a failed assert in the reference) */

typedef struct vpin_ctx vpin_ctx;
typedef struct vpin_table vpin_table;

const char* vpin_strerror(int code);
/* text of the last HIP failure seen by this thread ("" if none) */
const char* vpin_last_error(void);
/* A host that is about to run something that may take the PROCESS down (a first outing of RCCL at world > 1 ...) leaves the line
 * it has already earned here: on SIGSEGV / SIGBUS / SIGABRT / SIGFPE / SIGTERM the handler writes these bytes to stdout and ends
 * the process with _exit(0) -- async-signal-safe calls only.  n = 0 disarms (the previous handlers come back).  bench.py arms it
 * with the weak line before its strong sub-record (n <= 8192). */
int vpin_crash_line_set(const char* line, size_t n);
/* ABI version of this library (bumped on any signature change) */
int vpin_abi_version(void);

/* ---- context ------------------------------------------------------------------- */
int vpin_ctx_create(int device, vpin_ctx** out);
/* Same with a stream priority: < 0 high (its kernels are dispatched ahead of other streams' queued
 * workgroups), 0 normal, > 0 low.  For running latency-bound small proofs beside a large one. */
int vpin_ctx_create_prio(int device, int priority, vpin_ctx** out);
/* Same with the context's stream confined to a subset of the device's compute units (hipExtStreamCreateWithCUMask): bit i
 * of cu_mask (n_words x 32 bits) enables CU i in the runtime's numbering -- on an 8-XCD part consecutive bits go round-robin
 * over the XCDs, so the first 8k bits are k CUs of every XCD.  A service that proves one large instance beside many small
 * ones gives each side its own CUs (a spatial split) instead of letting their workgroups share every CU; the row-commitment
 * kernels size their grids to the enabled CUs.  A masked stream has normal priority. */
int vpin_ctx_create_cumask(int device, const uint32_t* cu_mask, uint32_t n_words, vpin_ctx** out);
/* A second stream for an (unmasked) context, confined to the CUs of cu_mask: every proof on the context moves to it when
 * its phase-1 sum-check is over -- the point where the progress word (vpin_ctx_set_progress_flag) becomes 1 -- and returns
 * to the first stream when the call returns.  For a scheduler that holds other contexts back during phase 1 and gives the
 * chip a spatial split afterwards: the large proof's commitments then own their CUs (row-per-lane strips stay in step).
 * cu_mask = NULL removes the second stream. */
int vpin_ctx_set_cumask_after_phase1(vpin_ctx* ctx, const uint32_t* cu_mask, uint32_t n_words);
void vpin_ctx_destroy(vpin_ctx* ctx);
/* hipStream_t the ctx launches on (as void*), for callers that time with HIP events */
void* vpin_ctx_stream(vpin_ctx* ctx);
/* Optional progress word in host memory: a proof stores 1 to it when its phase-1 sum-check is over (and again
 * when the whole sat part is) and 2 when its derefs commitment -- the largest MSM of a SNARK -- is done, so that a
 * caller running other proofs on other contexts can hold them back while the phase-1 kernels of this one are being
 * timed, or until its power-bound MSM has had the chip to itself.  NULL clears it. */
int vpin_ctx_set_progress_flag(vpin_ctx* ctx, int* flag);
/* Several contexts prove on this device at the same time (a service, bench.py's lanes): the long VALU-bound row-commitment
 * kernels of this context then run ONE workgroup per CU instead of three (a wave per SIMD), so that a large instance's
 * commitment no longer stalls every other stream for its whole duration and the latency-bound proofs of the other lanes
 * keep most of every CU (LeNet step on four lanes: 451 -> 435 ms against two workgroups per CU, 513 before any limit). */
int vpin_ctx_set_shared_device(vpin_ctx* ctx, int on);
/* commitment rows this context has handed to the row-per-lane kernel (msm_strip_kernel) since it was created: lets a test
 * or a scheduler see that the path it asked for is the one that ran */
unsigned long long vpin_ctx_strip_rows_taken(vpin_ctx* ctx);
/* (ABI 11) sums this context has taken through the shared-scalar bucket walk (e2_sh_window_kernel): every sum of a
 * vpin_e2_msm_shared call, and the random-linear-combination sums of the layers whose shape the selection rule sends there.  A
 * call that is rejected adds nothing */
unsigned long long vpin_ctx_rlc_shared_sums(vpin_ctx* ctx);
/* Test hook: the bytes of per-window results (sums x windows x 96) the walk holds at once on this context; above it the sums are
 * taken in chunks.  0 restores the library's 128 MiB.  The results do not depend on it */
int vpin_ctx_set_rlc_shared_cap(vpin_ctx* ctx, size_t bytes);
/* Test hook: on != 0 makes the context's device pool fill every block it hands out from now on -- fresh from the driver or
 * recycled, the whole size class and not only the bytes asked for -- with `word`, on the context's stream, before the block is
 * returned; a temporary then never arrives zeroed or holding the previous call's results.  on = 0 restores the plain allocator.
 * Covers the pooled temporaries and tables only: not the context's fixed scratch, the pinned mailboxes or the window tables.
 * The results do not depend on it */
int vpin_ctx_set_pool_poison(vpin_ctx* ctx, uint32_t word, int on);
/* Test hook: blocks and bytes the pool has filled on this context since it was created (either pointer may be NULL) */
int vpin_ctx_pool_poison_stats(vpin_ctx* ctx, unsigned long long* blocks, unsigned long long* bytes);
/* rows committed through the row-table kernels so far (tests: the path under test is the one that ran) */
unsigned long long vpin_ctx_row_table_rows(vpin_ctx* ctx);
/* scalars (rows x columns, a blind column included) from which a row commitment on this context goes to the row-table kernels
 * when its stream has a row table: the library's default, or VPIN_MSM_ROW_MIN when that is set (read per call).  part_short != 0:
 * for the callers whose scalars are partly short (the provers' witness commitments).  0 for a NULL ctx. */
size_t vpin_msm_row_min_scalars(vpin_ctx* ctx, int part_short);
/* row chunks the bucket method (vpin_hyrax_commit_pippenger, VPIN_MSM_PIPPENGER) has launched on this context: a commitment
 * whose digit buffer would pass 2 GiB takes its rows in several (the 2^14 x 2^15 polynomials of a 2^25-constraint instance: 15) */
unsigned long long vpin_ctx_pip_row_chunks(vpin_ctx* ctx);
/* operations of the last vpin_gadget_point_mult_dev call on this context whose witness the step-by-step kernel wrote
 * (gd_mult_witness_kernel): those the batched-inversion kernel flagged because a denominator or a Z vanished, or all N
 * under VPIN_WITNESS_LITERAL.  0 for a batch of honest inputs: lets a test see which kernel produced a witness. */
unsigned long long vpin_ctx_witness_redo_ops(vpin_ctx* ctx);
/* the context's device memory pool: out = {bytes obtained from the driver and still held (handles + temporaries + cached
 * blocks), bytes of those sitting in the free lists (reusable by the next proof), blocks}.  What bench.py's hbm_breakdown and a
 * service's admission control are made of. */
int vpin_ctx_pool_stats(vpin_ctx* ctx, size_t out[3]);
/* out = {calls, bytes}: allocations this library has taken from the driver (hipMalloc) since the process started, all contexts
 * (the contexts' pools, the unpooled tables of a split proof; generator tables not counted).  A proof of a shape its context
 * has already proven must leave both unchanged: tests/test_gpu_pool.py (round 5's SNARK::encode took 20 GB from the driver
 * per call -- 0.3 ms most of the time, 0.2-2.8 s every few calls). */
int vpin_driver_alloc_stats(unsigned long long out[2]);
/* hand the pool's cached (free) blocks back to the driver: after set-up work whose temporaries no proof will reuse (gadget
 * synthesis, SNARK::encode), or when a service changes workload.  Synchronises the context's stream. */
int vpin_ctx_pool_trim(vpin_ctx* ctx);
/* Low-memory mode: proofs on this context keep a smaller working set at a small cost in time.  Today: the SPARK mem forest
 * (4 product circuits over M leaves) is built after the ops forest has been proven, into the memory it frees, its roots coming
 * first from a product reduction -- 16 GiB less for a 2^25-constraint instance, ~1 % more time.  Same bytes. */
int vpin_ctx_set_low_memory(vpin_ctx* ctx, int on);
/* How many proofs the generator window tables built through this context will serve: 0 (default) = many -- the widest
 * windows the table budget allows (fewest additions per scalar; the table costs ~0.2 s to build for the largest
 * instance); n > 0 = a process that proves n times and exits (vpin_prove: a process per label, like `cargo run -- <label>`):
 * the window width then minimises table construction + n proofs' commitments (10 instead of 12 bits for the 2^25
 * instance, 8 for the small ones). */
int vpin_ctx_set_expected_proofs(vpin_ctx* ctx, int n);
/* compute units and shader clock (kHz) of the context's device: the VALU-issue ceiling bench.py prices the MSM against */
int vpin_ctx_device_props(vpin_ctx* ctx, int* num_cus, int* clock_khz);
/* free / total HBM of the context's device, bytes (the table budgets are chosen from `total`) */
int vpin_ctx_mem_info(vpin_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
int vpin_ctx_sync(vpin_ctx* ctx);

/* Host buffers that cross the bus often (a service's witness buffers, the triplets of an instance it proves again and again)
 * can be page-locked once: the host-buffer entry points (vpin_r1cs_upload, vpin_table_upload, vpin_sat_prove, vpin_snark_prove)
 * then copy at the bus rate instead of through the driver's staging buffers (CNN A's sat proof from host buffers: 18.9 -> see
 * DESIGN.md section 5).  hipHostRegister / hipHostUnregister: the range must stay valid until unregistered. */
int vpin_host_register(void* p, size_t bytes);
int vpin_host_unregister(void* p);

/* ---- tables: device-resident Vec<Scalar> ---------------------------------------- */
/* DensePolynomial::new (Spartan/src/dense_mlpoly.rs:132-138): len must be a power of 2 */
int vpin_table_upload(vpin_ctx* ctx, const uint8_t* mont32, size_t len, vpin_table** out);
int vpin_table_alloc(vpin_ctx* ctx, size_t len, vpin_table** out); /* zero-filled */
/* adopt caller-owned device memory (e.g. a framework tensor) without copying */
int vpin_table_wrap(vpin_ctx* ctx, void* device_ptr, size_t len, vpin_table** out);
int vpin_table_clone(vpin_ctx* ctx, const vpin_table* src, vpin_table** out);
void vpin_table_free(vpin_ctx* ctx, vpin_table* t);
size_t vpin_table_len(const vpin_table* t); /* DensePolynomial::len(), halves on every bind */
void* vpin_table_device_ptr(const vpin_table* t);
/* Index<usize> for DensePolynomial (dense_mlpoly.rs:295-302): read n scalars from off */
int vpin_table_read(vpin_ctx* ctx, const vpin_table* t, size_t off, size_t n, uint8_t* out);
/* the reverse: n scalars from host memory into the table's allocation at element offset `off` (len is unchanged) */
int vpin_table_write(vpin_ctx* ctx, vpin_table* t, size_t off, size_t n, const uint8_t* src);

/* ---- sum-check round reductions -------------------------------------------------- */
/* Round evaluation loop of ZKSumcheckInstanceProof::prove_cubic_with_additive_term
 * (Spartan/src/sumcheck.rs:624-652) with R1CSProof::prove_phase_one's combiner
 * A*(B*C-D) (Spartan/src/r1csproof.rs:104-108).  out = e0|e2|e3, 3 x 32 B Montgomery. */
int vpin_sc_cubic_round(vpin_ctx* ctx, const vpin_table* tau, const vpin_table* Az,
                        const vpin_table* Bz, const vpin_table* Cz, uint8_t out_e0_e2_e3[96]);
/* Round evaluation loop of ZKSumcheckInstanceProof::prove_quad (sumcheck.rs:460-469)
 * with prove_phase_two's combiner A*B (r1csproof.rs:139-140).  out = e0|e2. */
int vpin_sc_quad_round(vpin_ctx* ctx, const vpin_table* A, const vpin_table* B,
                       uint8_t out_e0_e2[64]);
/* DensePolynomial::bound_poly_var_top (dense_mlpoly.rs:229-236) on k tables at once
 * (sumcheck.rs:673-676 / :485-486): Z[i] += r*(Z[i+n]-Z[i]); len /= 2. In place. */
int vpin_sc_bind(vpin_ctx* ctx, vpin_table* const* tables, int k, const uint8_t r[32]);
/* Fused single pass: bind the four (two) tables with r, then evaluate the NEXT round on
 * the folded tables -- one read of every live element and one write of every folded
 * element per round (SURVEY.md 8(d) "algorithmic bytes").  Same results as
 * vpin_sc_bind followed by vpin_sc_*_round.  Requires len >= 4. */
int vpin_sc_cubic_bind_round(vpin_ctx* ctx, vpin_table* tau, vpin_table* Az, vpin_table* Bz,
                             vpin_table* Cz, const uint8_t r[32], uint8_t out_e0_e2_e3[96]);
int vpin_sc_quad_bind_round(vpin_ctx* ctx, vpin_table* A, vpin_table* B, const uint8_t r[32],
                            uint8_t out_e0_e2[64]);

/* EqPolynomial::evals (dense_mlpoly.rs:78-94): r = ell x 32 B, result has 2^ell entries */
int vpin_eq_table(vpin_ctx* ctx, const uint8_t* r, int ell, vpin_table** out);

/* Eq-factored phase 1 (same e0,e2,e3 as vpin_sc_cubic_*, cheaper): the folded eq(tau,.) table of round j
 * equals a scalar times the suffix table eq(tau_{j+1..}, .), so it is neither stored per round nor folded.
 * vpin_eq_suffix_tables builds all suffix tables once (one table of 2^ell elements); the round calls take
 * (Az,Bz,Cz) and level = j+1 and return the UNSCALED sums S_x = sum_i E[i]*(Az_x[i]*Bz_x[i] - Cz_x[i]) for
 * x = 0, 2, 3 (the reference's comb is tau*(Az*Bz - Cz), r1csproof.rs:104-108); the caller multiplies by
 * c_{j,x} = s_j*((1-tau_j) + x*(2*tau_j-1)) with s_j = prod_{i<j} eq1(tau_i, r_i) to get e0, e2, e3. */
int vpin_eq_suffix_tables(vpin_ctx* ctx, const uint8_t* tau, int ell, vpin_table** out);
int vpin_sc_cubic3_round(vpin_ctx* ctx, const vpin_table* pyramid, int ell, int level, vpin_table* Az,
                         vpin_table* Bz, vpin_table* Cz, uint8_t out_S0_S2_S3[96]);
int vpin_sc_cubic3_bind_round(vpin_ctx* ctx, const vpin_table* pyramid, int ell, int level, vpin_table* Az,
                              vpin_table* Bz, vpin_table* Cz, const uint8_t r[32], uint8_t out_S0_S2_S3[96]);
/* Leading-coefficient form of the same round, the one vpin_sat_prove runs while phase 1's claim is consistent: with
 * the eq factor split off the round polynomial is l(x) * t(x), t(x) = sum_i E[i]*(Az_x*Bz_x - Cz_x)[i] quadratic, and
 * the kernel returns t(0), the x^2 coefficient sum_i E[i]*(dAz*dBz)[i] and -- only when r == NULL (first round) --
 * t(1).  The same e0, e2, e3 of Spartan/src/sumcheck.rs:624-652 follow by exact field identities.  r != NULL binds
 * the tables with r first (dense_mlpoly.rs:229-236). */
int vpin_sc_cubic3_lead_round(vpin_ctx* ctx, const vpin_table* pyramid, int ell, int level, vpin_table* Az,
                              vpin_table* Bz, vpin_table* Cz, const uint8_t* r, uint8_t out[96]);
/* One round of SumcheckInstanceProof::prove_cubic_batched (Spartan/src/sumcheck.rs:273-330,346-370) as
 * ProductCircuitEvalProofBatched::prove issues it (Spartan/src/product_tree.rs:258-385): `ncirc` product circuits of
 * `n` leaves each (tree t = forest[t*2n ..), level l at offset 2n - (2n >> l), left/right halves = poly_A/poly_B) proven
 * in lock-step, eq-factored (E = eq suffix table of this round at E[e_off..], len/2 entries, or len/4 when r != NULL and
 * the tables are first bound with r).  out: per circuit 3 scalars -- lead == 0: sum_i E[i]*(A_x*B_x)[i] at x = 0, 2, 3;
 * lead == 1: the value at 0, the x^2 coefficient sum_i E[i]*(dA*dB)[i], and zero.  derefs != NULL (ncirc == 12,
 * level == 0) adds the six DotProductCircuit halves of Spartan/src/sparse_mlpoly.rs:1103-1125 (A*B*C over derefs row |
 * col slices (6 x n) and the val slices (3 x n); first fold into scratch, 18 x n/4): out[12..18) = sums at 0, 2, 3. */
int vpin_spark_batched_round(vpin_ctx* ctx, vpin_table* forest, size_t n, int ncirc, int level, size_t len,
                             const vpin_table* E, size_t e_off, const uint8_t* r, int lead, const vpin_table* derefs,
                             const vpin_table* vals, vpin_table* scratch, int first_fold, uint8_t* out);

/* ---- Pedersen generators and fixed-base MSM ----------------------------------------- */
/* The generator stream of MultiCommitGens::new (Spartan/src/commitments.rs:20-38):
 * nb points g[0..nb) as 128-byte X|Y|Z|T each.  Builds the device window table
 * T[w][j][k] = (k+1) * 2^(8w) * g_j once; every MSM below is a gather-and-add over it.
 * For R1CSGens (Spartan/src/r1csproof.rs:84-89) the stream is g[0..R+2): G = g[0..R),
 * gens_1.G[0] = g[R], h = g[R+1]; gens_3 / gens_4 are prefixes with h = g[3] / g[4]. */
typedef struct vpin_gens vpin_gens;
int vpin_gens_create(vpin_ctx* ctx, const uint8_t* gens_xyzt, size_t nb, vpin_gens** out);
/* RistrettoPoint::from_uniform_bytes for nb generators at once on the device: stream64 = 64 x nb bytes of the label's SHAKE256
 * stream (Spartan/src/commitments.rs:20-38), out_xyzt = nb x 128 bytes X|Y|Z|T like vpin_host_gens_derive (same points;
 * the projective representative may differ) */
int vpin_gens_map_stream(vpin_ctx* ctx, const uint8_t* stream64, size_t nb, uint8_t* out_xyzt);
/* Shared form: one immutable table per (device, label), holding the longest prefix of the label's
 * generator stream requested so far -- MultiCommitGens::new(n, label) for every n is a prefix of the same
 * SHAKE256 stream (Spartan/src/commitments.rs:20-38), so all contexts / streams / polynomial sizes of a
 * label share it.  gens_xyzt (nb points) is only read when a new table has to be built.  budget_gb = 0:
 * default table budget.  The returned handle is owned by the registry (never pass it to vpin_gens_free). */
int vpin_gens_shared(vpin_ctx* ctx, const char* label, const uint8_t* gens_xyzt, size_t nb, size_t budget_gb,
                     const vpin_gens** out);
/* frees every shared table; only when no context uses them any more */
void vpin_gens_shared_clear(void);
/* bytes of the process-wide window tables on `device` */
size_t vpin_gens_shared_bytes(int device);
void vpin_gens_free(vpin_ctx* ctx, vpin_gens* g);
size_t vpin_gens_count(const vpin_gens* g);
/* Window layout the table budget chose: out = {c, W, split, c_hi, W_hi, bases}: generators [0, split) have c-bit signed
 * windows (W per scalar), [split, bases) c_hi-bit ones (0 when the table has a single segment); `bases` counts the
 * nb generators plus the prefix-sum bases S_k = g_0 + ... + g_{2^k - 1} behind them. */
int vpin_gens_layout(const vpin_gens* g, size_t out[6]);
/* The row table beside it, if the table has one: out = {c_row, W_row, bases covered, columns per segment of the row kernel}.
 * T1[j][k] = (k+1) g_j for one window of c_row bits per generator; the row commitments of vpin_msm_row_min_scalars and more accumulate one
 * sum per window from it and apply the powers of two once per row.  All 0 for a table without one. */
int vpin_gens_row_layout(const vpin_gens* g, size_t out[4]);
/* TEST ENTRY POINT, not for callers: the provers reach this commitment through vpin_snark_prove*; it validates its indices on the
 * host and copies synchronously.  The derefs commitment on its own: Z = 8N scalars as L rows of R = 8N / L, whose rows [3N/R, 6N/R) are the col-derefs
 * vectors e_ry[col_idx[m][i]] of the three matrices; col_idx = 3 x N column indices on the host, hot[m] = the column of matrix m
 * whose entries are added as hot[m]-multiples computed once (0xffffffff: none).  out_compressed: L x 32 bytes, the bytes of
 * DensePolynomial::commit(gens, None). */
int vpin_hyrax_commit_derefs(vpin_ctx* ctx, const vpin_gens* g, const vpin_table* Z, size_t L, size_t N, const uint32_t* col_idx,
                             const uint32_t hot[3], const vpin_table* e_ry, uint8_t* out_compressed);
/* bytes per window-table entry (affine Niels point, possibly padded to a cache line) */
size_t vpin_gens_entry_bytes(void);
/* DensePolynomial::commit_inner (Spartan/src/dense_mlpoly.rs:160-175): Z viewed as L rows
 * of R = len/L scalars; out[i] = compress( sum_j Z[iR+j]*g[j] + blinds[i]*g[blind_base] ).
 * blinds = L x 32 B Montgomery scalars on the host. */
int vpin_hyrax_commit(vpin_ctx* ctx, const vpin_gens* g, const vpin_table* Z, const uint8_t* blinds,
                      size_t L, size_t blind_base, uint8_t* out_compressed /* L*32 */);
/* Rows [row0, row0 + nrows) of the same commitment (Z viewed as L rows; blinds = nrows x 32 B for those rows, or NULL
 * for DensePolynomial::commit(gens, None)).  The L row commitments are independent MSMs over shared generators
 * (rayon's into_par_iter at dense_mlpoly.rs:166-173), so a commitment splits across GPUs by rows: every rank commits
 * a contiguous block and the 32-byte results are all-gathered -- no point crosses a link. */
int vpin_hyrax_commit_rows(vpin_ctx* ctx, const vpin_gens* g, const vpin_table* Z, size_t L, size_t row0, size_t nrows,
                           const uint8_t* blinds, size_t blind_base, uint8_t* out_compressed);
/* The same commitment (DensePolynomial::commit_inner, Spartan/src/dense_mlpoly.rs:160-175) computed the way
 * GroupElement::vartime_multiscalar_mul does above 190 terms (Spartan/src/group.rs:103-122, dalek's Pippenger): signed
 * c_bits-bit digits, bucket accumulation staged in LDS, running-sum reduction -- from the generators alone, no window table
 * walked.  A measured alternative, NOT what the provers call (it is slower on this part: profiles/r05_pippenger.txt).
 * blinds may be NULL (commit(gens, None)); c_bits in 9..12, or 0 = the measured best (9).  Same bytes as
 * vpin_hyrax_commit. */
int vpin_hyrax_commit_pippenger(vpin_ctx* ctx, const vpin_gens* g, const vpin_table* Z, const uint8_t* blinds, size_t L,
                                size_t blind_base, int c_bits, uint8_t* out_compressed);
/* The two commitments of proof_point_{add,mult}.rs:44-52 plus their row-wise sum
 * (:75-80) in one call: out_sum[i] = compress(decompress(a[i]) + decompress(b[i])). */
int vpin_hyrax_commit_pair(vpin_ctx* ctx, const vpin_gens* g, const vpin_table* Za, const vpin_table* Zb,
                           const uint8_t* blinds_a, const uint8_t* blinds_b, size_t L, size_t blind_base,
                           uint8_t* out_a, uint8_t* out_b, uint8_t* out_sum);
/* The same three outputs the way the provers form them: the two row MSMs without blinds first, then blind_i * g[blind_base]
 * for the 2L blinds as single-base multiples (eight lanes per scalar) added per row.  Same bytes as vpin_hyrax_commit_pair;
 * public so that the blind path of the provers can be driven with chosen blinds. */
int vpin_hyrax_commit_pair_split(vpin_ctx* ctx, const vpin_gens* g, const vpin_table* Za, const vpin_table* Zb,
                                 const uint8_t* blinds_a, const uint8_t* blinds_b, size_t L, size_t blind_base,
                                 uint8_t* out_a, uint8_t* out_b, uint8_t* out_sum);
/* GroupElement::vartime_multiscalar_mul (Spartan/src/group.rs:103-122) over a prefix of the
 * generator stream: out[r] = sum_{j<ncols} s[r][j] * g[j] for `rows` independent rows of
 * host scalars (Montgomery).  Either output may be NULL. */
int vpin_gens_msm(vpin_ctx* ctx, const vpin_gens* g, const uint8_t* scalars_mont, size_t rows, size_t ncols,
                  uint8_t* out_compressed /* rows*32 */, uint8_t* out_xyzt /* rows*128 */);

/* GroupElement::vartime_multiscalar_mul (Spartan/src/group.rs:103-122) over ARBITRARY points, given as compressed
 * ristretto255 encodings (n x 32 B) with n Montgomery scalars: out = sum_i s_i * decompress(P_i).  One lane per term
 * (decompression, double-and-add, block tree): sized for the row counts of Hyrax commitments (the verifier's <L, C> of
 * dense_mlpoly.rs:381-404), not for millions of points.  VPIN_EVERIFY when an encoding does not decode.  Either output
 * may be NULL. */
int vpin_msm(vpin_ctx* ctx, const uint8_t* scalars_mont, const uint8_t* points_compressed, size_t n, uint8_t* out_compressed,
             uint8_t* out_xyzt);
/* The same sum by a windowed bucket method (signed windows of c or c - 1 bits, one decompression per point, buckets
 * accumulated with the complete addition, running-sum reduction per window, windows combined on the device).  Measured
 * (profiles/r07_ab_msm_var_bucket.txt): slower than vpin_msm by a quarter up to 2^16 terms, faster by 11 % at 2^17;
 * vpin_snark_verify_batch uses it from 2^17 terms on.  Same contract as vpin_msm, the compressed result is byte-identical.
 * n < 2^31. */
int vpin_msm_bucket(vpin_ctx* ctx, const uint8_t* scalars_mont, const uint8_t* points_compressed, size_t n, uint8_t* out_compressed,
                    uint8_t* out_xyzt);
/* out[i] = compress(decompress(a[i]) + decompress(b[i])), n points: the row-wise sum of two commitment vectors
 * (vPIN_proof_generation/src/commit_test.rs:340-361).  VPIN_EVERIFY when an encoding does not decode. */
int vpin_points_add(vpin_ctx* ctx, const uint8_t* a_compressed, const uint8_t* b_compressed, size_t n, uint8_t* out_compressed);

/* Same MSM for the few-row, latency-bound case: returns the per-workgroup partial points
 * (X|Y|Z|T, 128 B each, rows x vpin_gens_msm_parts_count(ncols)); the caller adds them. */
size_t vpin_gens_msm_parts_count(size_t ncols);
int vpin_gens_msm_parts(vpin_ctx* ctx, const vpin_gens* g, const uint8_t* scalars_mont, size_t rows, size_t ncols,
                        uint8_t* parts_xyzt);

/* DensePolynomial::bound (Spartan/src/dense_mlpoly.rs:220-227): LZ[i] = sum_j L[j]*Z[j*R+i],
 * Lvec = L_size host scalars, out = R = len/L_size host scalars. */
int vpin_poly_bound(vpin_ctx* ctx, const vpin_table* Z, const uint8_t* Lvec, size_t L_size, uint8_t* out_LZ);
/* The hash layer's slice pass (sparse_mlpoly.rs:740-849; single GPU): Z holds 2^nbits slices of N = 2^r_len scalars each.
 * One pass over the first `used` slices yields (i) their evaluations at r -- DensePolynomial::evaluate, dense_mlpoly.rs:
 * 239-253 -- in evals_out (used x 32 bytes) and (ii), for combining challenges ch (nbits scalars; NULL: skip), what
 * PolyEvalProof::prove's first step computes for the whole Z at the point (ch, r): LZ = L^T Z with L = eq((ch, r)[..left])
 * (dense_mlpoly.rs:340-349; R = 2^(ell - ell/2) scalars in LZ_out), without reading Z again.  The slices from `used` on must be
 * zero (the reference pads the combined polynomials with zero slices).  Needs ell / 2 >= nbits (ell = r_len + nbits). */
int vpin_poly_slices_bound(vpin_ctx* ctx, const vpin_table* Z, int nbits, int used, const uint8_t* r, size_t r_len,
                           const uint8_t* ch, uint8_t* evals_out, uint8_t* LZ_out);
/* The same with the first n32 slices given as u32 values (host memory, n32 x 2^r_len: addresses and timestamps of the
 * computation decommitment, sparse_mlpoly.rs:418-428, whose field images Scalar::from(v) the proof never forms: 4 bytes and
 * eight 32-bit multiply-adds per entry instead of 32 bytes and a product mod q) and the remaining used - n32 slices as a table
 * of field elements (Zfq, NULL when used == n32).  Same elements as vpin_poly_slices_bound over the field images. */
int vpin_poly_slices_bound_u32(vpin_ctx* ctx, const uint32_t* slices_u32, int n32, const vpin_table* Zfq, int nbits, int used,
                               const uint8_t* r, size_t r_len, const uint8_t* ch, uint8_t* evals_out, uint8_t* LZ_out);

/* ---- the sat proof (host orchestration over the kernels above) ------------------------ */
/* R1CSInstance after Instance::new's padding and column remap (Spartan/src/lib.rs:138-244):
 * num_cons / num_vars are powers of two; col indexes z = [vars | 1 | inputs | 0...] of length
 * 2*num_vars; val = 32-byte Montgomery scalars. */
typedef struct {
  size_t num_cons, num_vars, num_inputs;
  size_t nnz[3];          /* A, B, C */
  const uint32_t* row[3];
  const uint32_t* col[3];
  const uint8_t* val[3];
} vpin_r1cs;
/* Device-resident instance: CSR + CSC copies of (A,B,C) in HBM (the reference's
 * SparseMatPolynomial, Spartan/src/sparse_mlpoly.rs:330-380), built once per instance. */
typedef struct vpin_r1cs_dev vpin_r1cs_dev;
int vpin_r1cs_upload(vpin_ctx* ctx, const vpin_r1cs* inst, vpin_r1cs_dev** out);
void vpin_r1cs_free(vpin_ctx* ctx, vpin_r1cs_dev* d);
void vpin_r1cs_dims(const vpin_r1cs_dev* d, size_t* num_cons, size_t* num_vars, size_t* num_inputs);
/* z = [vars | 1 | inputs | 0...] (vPIN_proof_generation/src/commit_test.rs:162-170); inputs on the host */
int vpin_r1cs_build_z(vpin_ctx* ctx, const vpin_r1cs_dev* d, const vpin_table* vars, const uint8_t* inputs,
                      vpin_table** out_z);
/* R1CSInstance::multiply_vec (Spartan/src/r1csinstance.rs:272-285 -> sparse_mlpoly.rs:467-481) */
int vpin_r1cs_multiply_vec(vpin_ctx* ctx, const vpin_r1cs_dev* d, const vpin_table* z, vpin_table** Az,
                           vpin_table** Bz, vpin_table** Cz);
/* R1CSInstance::compute_eval_table_sparse (r1csinstance.rs:287-295 -> sparse_mlpoly.rs:483-498) folded with
 * the three challenges r_A|r_B|r_C as at commit_test.rs:257-268: out[i] = r_A*A(rx,i)+r_B*B(rx,i)+r_C*C(rx,i) */
int vpin_r1cs_eval_table(vpin_ctx* ctx, const vpin_r1cs_dev* d, const vpin_table* evals_rx, const uint8_t r_abc[96],
                         vpin_table** out);
/* R1CSInstance::evaluate (r1csinstance.rs:297-302) from the two eq tables; out = Ar|Br|Cr */
int vpin_r1cs_evaluate(vpin_ctx* ctx, const vpin_r1cs_dev* d, const vpin_table* evals_rx, const vpin_table* evals_ry,
                       uint8_t out[96]);

/* One gadget instance's satisfiability proof exactly as vPIN drives it:
 * proof_point_{add,mult}.rs:38-94 (commit para / input under RandomTape::new(&[2]), combine)
 * + commit_test.rs:59-109 my_lib_prove up to the Ar/Br/Cr claims (= my_R1CSProof_prove,
 * commit_test.rs:136-334, + inst.evaluate).  The reference seeds its two RandomTapes from
 * OsRng (Spartan/src/random.rs:14-22); the two 64-byte draws are explicit inputs here, which
 * is what makes proofs reproducible.  Outputs: bincode bytes of R1CSProof, the two L x 32 B
 * commitments the verifier needs, inst_evals = Ar|Br|Cr, rx (log2 num_cons scalars),
 * ry (log2 num_vars + 1 scalars).  rx_out / ry_out may be NULL. */
int vpin_sat_prove(vpin_ctx* ctx, const vpin_r1cs* inst, const uint8_t* vars_para, const uint8_t* vars_input,
                   const uint8_t* vars, const uint8_t* inputs, const uint8_t seed_commit64[64],
                   const uint8_t seed_proof64[64], uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                   uint8_t* comm_para_out, uint8_t* comm_input_out, uint8_t inst_evals_out[96],
                   uint8_t* rx_out, uint8_t* ry_out);
/* Same proof with the instance and the three assignments already resident in HBM (what bench.py times). */
int vpin_sat_prove_resident(vpin_ctx* ctx, const vpin_r1cs_dev* inst, const vpin_table* vars_para,
                            const vpin_table* vars_input, const vpin_table* vars, const uint8_t* inputs,
                            const uint8_t seed_commit64[64], const uint8_t seed_proof64[64], uint8_t* proof_out,
                            size_t proof_cap, size_t* proof_len, uint8_t* comm_para_out, uint8_t* comm_input_out,
                            uint8_t inst_evals_out[96], uint8_t* rx_out, uint8_t* ry_out);
size_t vpin_sat_proof_max_bytes(size_t num_cons, size_t num_vars);
/* my_dense_mlpoly_commit (vPIN_proof_generation/src/commit_test.rs:27-57) as proof_point_{add,mult}.rs:58-59 call it: the
 * Hyrax commitment of the WHOLE assignment under the element-wise sum of the blinds of the two commitments made before it
 * (RandomTape::new(&[2]), labels b"poly_blinds" x L twice).  The reference computes it inside its timed span and then reads
 * row 0 only (assert_eq!(c, c_prime), proof_point_mult.rs:69-73): the proof carries the row-wise sum of the two partial
 * commitments, which is the same vector.  vpin_sat_prove* / vpin_snark_prove* therefore never compute it (SURVEY.md 8(f) row
 * N4); this entry point exists so that a host which wants the reference's assert, or the reference's span "with" the dead
 * work, can have it: out = L x 32 B, L = 2^(log2(len) / 2), equal to comm_para + comm_input row by row. */
int vpin_dense_mlpoly_commit_sum(vpin_ctx* ctx, const vpin_table* vars, const uint8_t seed_commit64[64], uint8_t* out_compressed);
/* R1CSGens::new (Spartan/src/r1csproof.rs:84-89) for this polynomial size ahead of the first proof: host
 * fixed-base tables + the shared device window table (built on demand by the prove calls otherwise). */
int vpin_sat_prepare(vpin_ctx* ctx, size_t num_vars);
/* R1CSCommitmentGens::new (Spartan/src/r1csinstance.rs:29-49; SparseMatPolyCommitmentGens::new,
 * sparse_mlpoly.rs:300-329) for an instance of this shape ahead of the first encode / proof: derives the
 * b"gens_r1cs_eval" stream and builds (or finds) the shared device window table.  Call it for the LARGEST instance
 * first: smaller ones then share its table instead of each leaving a superseded one behind. */
int vpin_spark_prepare(vpin_ctx* ctx, size_t num_cons, size_t num_vars, size_t max_nnz);

/* wall-clock spans of the last vpin_sat_prove call on this thread's process, seconds:
 * [0] polycommit (uploads + 2 commits + combine)  [1] prove_sc_phase_one (eq table, SpMV, 4 uploads, rounds)
 * [2] prove_sc_phase_two  [3] polyeval  [4] total  [5] generators (0 when cached)
 * [6] host SpMV share of [1]+[2]  [7] inst.evaluate */
void vpin_sat_last_timings(double out[8]);

/* ------------------------------------------------------------------------------------------------
 * SPARK: the computation commitment and the sparse-polynomial evaluation proof that complete the
 * reference's SNARK.
 * ---------------------------------------------------------------------------------------------- */

/* ComputationDecommitment (Spartan/src/lib.rs:70-73): MultiSparseMatPolynomialAsDense
 * (Spartan/src/sparse_mlpoly.rs:285-292) resident in HBM. */
typedef struct vpin_spark_decomm vpin_spark_decomm;

/* ---- one proof over the GPUs of one node -----------------------------------------------------------
 * SPMD: every rank (one process per GPU, or one thread per rank in a rehearsal) holds the same instance, creates a
 * vpin_comm, attaches it to its context with vpin_ctx_set_comm and calls the SAME vpin_snark_prove_* / vpin_sat_prove_*
 * with the same inputs and seeds.  Inside the call the heavy steps are sharded and their small results all-gathered:
 *   - every Hyrax row commitment by interleaved rows r, r + world, .. (the witness pair of proof_point_mult.rs:44-52 and
 *     the derefs commitment of sparse_mlpoly.rs:525-531; rows are independent MSMs over shared generators,
 *     dense_mlpoly.rs:160-175) -- 32 bytes per row cross the links, no point and no reduction;
 *   - power-of-two worlds: BY RESIDUE CLASS.  The folds pair (i, i + len/2) (dense_mlpoly.rs:229-236), so rank r keeps the
 *     entries = r (mod world) of every table -- Az, Bz, Cz, z and the eval table of the sat proof's two sum-checks
 *     (sumcheck.rs:428-776), the leaves, trees and dot-product vectors of all 12 + 4 product circuits
 *     (product_tree.rs:259-385) -- and folds them with the single-GPU kernels; no table entry ever moves.  Per round a rank
 *     publishes its partial sums (3 scalars per circuit, 96 bytes in the sat rounds); the last log2(world) rounds of every
 *     sum-check run on the host from the world gathered entries per table;
 *   - other worlds (3, 5, 6, ..): the 12 + 4 product circuits and the 6 dot-product halves by circuit index
 *     (vpin_dist_plan below); the sat sum-checks stay replicated;
 *   - the 23 slice evaluations of the hash layer (sparse_mlpoly.rs:740-849) by residue class or by slice, and
 *     DensePolynomial::bound of the evaluation proofs (dense_mlpoly.rs:220-227) by rows (partial vectors all-gathered on
 *     the device: RCCL ncclAllGather when enabled, staged through the host transport otherwise).
 * The bullet reductions, the sigma protocols and the transcript stay replicated.  Every rank returns the same bytes, equal
 * to the single-GPU proof.  Without a comm (or with world == 1) the calls are the single-GPU ones.
 *
 * Transports for the small host-side exchanges (results are already on the host, where the transcript lives):
 *   vpin_comm_create_shm        ranks = processes of one node; a POSIX shared-memory segment `name`, which MUST be unique per
 *                               job (two live jobs under one name attach to each other; only the segment of a job that
 *                               has died is recognised and replaced).  Rank 0 creates it and unlinks it once everyone is
 *                               attached.  A flat all-gather of a few
 *                               hundred bytes costs ~1-3 us, against ~20-30 us for a RCCL kernel launch.
 *   vpin_comm_create_local      `world` handles for the threads of one process (rehearsals, tests)
 *   vpin_comm_create_callbacks  the caller's own all-gather (gloo in the CPU tests; a host's existing fabric)
 * Every wait is bounded (VPIN_COMM_TIMEOUT_S, default 120 s) and watches a shared abort word: a rank that fails or
 * disappears makes the others return VPIN_ECOMM instead of hanging. */
#define VPIN_ECOMM (-7) /* a peer failed or timed out, or the ranks disagree on a collective */
typedef struct vpin_comm vpin_comm;
typedef int (*vpin_allgather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
/* slot_bytes: largest message sent in one piece (larger ones are chunked); 0 = default (1 MiB) */
int vpin_comm_create_shm(const char* name, int rank, int world, size_t slot_bytes, vpin_comm** out);
int vpin_comm_create_local(int world, size_t slot_bytes, vpin_comm** out_handles /* world entries */);
int vpin_comm_create_callbacks(int rank, int world, vpin_allgather_fn fn, void* user, vpin_comm** out);
void vpin_comm_destroy(vpin_comm* cm);
int vpin_comm_rank(const vpin_comm* cm);
int vpin_comm_world(const vpin_comm* cm);
/* host buffers: recv = world x bytes */
int vpin_comm_allgather(vpin_comm* cm, const void* send, void* recv, size_t bytes);
/* RCCL for device buffers: rank 0 draws the ncclUniqueId, the host transport carries it, every rank runs
 * ncclCommInitRank on the context's device (librccl is dlopen'ed; VPIN_ENODEV when it is absent).  Collective. */
int vpin_comm_enable_rccl(vpin_comm* cm, vpin_ctx* ctx);
/* device buffers on the context's stream: ncclAllGather when RCCL is enabled, else staged through the host transport */
int vpin_comm_allgather_dev(vpin_comm* cm, vpin_ctx* ctx, const void* d_send, void* d_recv, size_t bytes);
/* Rehearsal of N ranks on fewer GPUs: on != 0 makes the ranks compute ONE AT A TIME (a token is held between
 * collectives and passed on inside them), so that the time a rank spends between two collectives is its own work and
 * nothing else; the statistics then give the critical path of the N-GPU run: sum over the collectives of the slowest
 * rank's section.  Collective on first use. */
int vpin_comm_set_serialize(vpin_comm* cm, int on);
typedef struct {
  uint64_t collectives;
  double bytes;   /* payload this rank sent */
  double wait_s;  /* time inside collectives (waiting for peers + copying) */
  double busy_s;  /* time between collectives (this rank's own sections) */
  double crit_s;  /* sum over collectives of max over ranks of the section before it */
} vpin_comm_stats;
int vpin_comm_stats_read(vpin_comm* cm, vpin_comm_stats* out, int reset);
/* the same per step of the protocol (the section before a collective is booked on the call site's tag; under
 * vpin_comm_set_serialize the proofs add empty marker collectives between their steps): text, one line per tag
 * "<tag> <collectives> <busy_s> <crit_s>"; returns the buffer size needed */
size_t vpin_comm_stats_tags(vpin_comm* cm, char* buf, size_t cap);
/* seconds per all-gather of `bytes` per rank over `iters` back-to-back collectives issued inside the library. Collective. */
int vpin_comm_latency(vpin_comm* cm, size_t bytes, int iters, double* seconds_per_collective);
/* Marks the group dead: every peer's current or next wait returns VPIN_ECOMM at once instead of running into the timeout
 * (shared-memory and local transports; a callbacks transport is the caller's to tear down).  The proving entry points do
 * this themselves when a rank leaves a collective proof with VPIN_ENOMEM / VPIN_EHIP / VPIN_ECOMM; a host calls it when a
 * rank fails outside the library (a witness that could not be read, a signal). */
void vpin_comm_abort(vpin_comm* cm);
/* attach (or detach with NULL): proofs on this context become collective calls over `cm`'s ranks */
int vpin_ctx_set_comm(vpin_ctx* ctx, vpin_comm* cm);
/* the b"gens_r1cs_eval" view a polynomial of 2^ell scalars is committed under (PolyCommitmentGens::new(ell, ..)) */
int vpin_spark_gens_view(vpin_ctx* ctx, size_t ell, const vpin_gens** out, size_t* L, size_t* R);
/* How the circuits of one proof are dealt to the ranks (deterministic; every rank computes the same plan):
 * owner_ops[12] / owner_dotp[6] / owner_mem[4] = owning rank of each "ops" circuit (row read A,B,C | row write A,B,C |
 * col read | col write), dot-product half (matrix, half) and "mem" circuit (row init, row audit, col init, col audit). */
int vpin_dist_plan(int world, int owner_ops[12], int owner_dotp[6], int owner_mem[4]);

/* bincode size of R1CSCommitment (Spartan/src/r1csinstance.rs:53-58) for this instance. */
size_t vpin_spark_comm_bytes(const vpin_r1cs* inst);
/* upper bound on bincode(SNARK) (Spartan/src/lib.rs:334-338) for this instance. */
size_t vpin_snark_proof_max_bytes(const vpin_r1cs* inst);

/* SNARK::encode (Spartan/src/lib.rs:347-359) = R1CSInstance::commit (r1csinstance.rs:309-322) =
 * SparseMatPolynomial::multi_commit (sparse_mlpoly.rs:382-438,500-520): dense representation
 * (ops_addr / read_ts / audit_ts / val), comb_ops and comb_mem committed row-wise under the
 * b"gens_r1cs_eval" generators.  comm_out receives bincode(R1CSCommitment): num_cons, num_vars,
 * num_inputs, batch_size = 3, num_ops, num_mem_cells, comm_comb_ops, comm_comb_mem.
 * The generators are sized from the instance's own max nnz (the reference passes a hand-tuned
 * num_non_zero_entries, point_mult.rs:67 / point_addition.rs:70, which must round to the same
 * power of two or its commit asserts, commitments.rs:95).
 * Limits: with N = next_pow2(max nnz of A, B, C) and M = max(num_cons, 2 * num_vars), VPIN_ESHAPE when N < 4 or M < 4
 * (so for every instance of fewer than 3 entries in its fullest matrix, the empty one included).  At N = 1 the reference's
 * product circuit has no layer to prove; at N = 2 it does produce a proof, which this library does not: the round kernels
 * start from tables of four.  VPIN_ESHAPE also for a row index >= num_cons or a column index >= 2 * num_vars in any triplet
 * (Instance::new's InvalidIndex, lib.rs:171-178) and for num_inputs >= num_vars; the context stays usable after each. */
int vpin_spark_encode(vpin_ctx* ctx, const vpin_r1cs* inst, vpin_spark_decomm** out, uint8_t* comm_out,
                      size_t comm_cap, size_t* comm_len);
void vpin_spark_decomm_free(vpin_ctx* ctx, vpin_spark_decomm* d);
/* The column SNARK::encode found to carry a large share of matrix A / B / C's entries (the constant 1 of an R1CS, or the
 * first input), 0xffffffff where there is none or the instance is too small for it to matter.  Derefs::new
 * (Spartan/src/sparse_mlpoly.rs:56-71) puts the SAME scalar eq(ry)[col] at every one of those entries, so the derefs
 * commitment of each proof (sparse_mlpoly.rs:525-531) adds v * g_j for them instead of walking a window table. */
void vpin_spark_decomm_hot_cols(const vpin_spark_decomm* d, uint32_t out[3]);

/* my_lib_prove in full (vPIN_proof_generation/src/commit_test.rs:59-133): the sat proof of
 * vpin_sat_prove_resident, then inst_evals, then R1CSEvalProof::prove (r1csinstance.rs:330-354 ->
 * sparse_mlpoly.rs:1466-1533) on the same transcript and RandomTape.  proof_out receives
 * bincode(SNARK { r1cs_sat_proof, inst_evals, r1cs_eval_proof }) -- what proof_point_mult.rs:96
 * measures as "Proof size". */
int vpin_snark_prove_resident(vpin_ctx* ctx, const vpin_r1cs_dev* inst, const vpin_spark_decomm* decomm,
                              const vpin_table* vars_para, const vpin_table* vars_input, const vpin_table* vars,
                              const uint8_t* inputs, const uint8_t seed_commit64[64], const uint8_t seed_proof64[64],
                              uint8_t* proof_out, size_t proof_cap, size_t* proof_len, uint8_t* comm_para_out,
                              uint8_t* comm_input_out);
/* proof_point_mult.rs:38-94 from host buffers (instance triplets + the three assignments in host memory):
 * SNARK::encode, then my_lib_prove in full.  comm_out receives bincode(R1CSCommitment). */
int vpin_snark_prove(vpin_ctx* ctx, const vpin_r1cs* inst, const uint8_t* vars_para, const uint8_t* vars_input,
                     const uint8_t* vars, const uint8_t* inputs, const uint8_t seed_commit64[64],
                     const uint8_t seed_proof64[64], uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                     uint8_t* comm_out, size_t comm_cap, size_t* comm_len, uint8_t* comm_para_out,
                     uint8_t* comm_input_out);
/* Verifiers (host C++; the evaluation proofs' fixed-base MSMs run on the device tables).  VPIN_OK = accept,
 * VPIN_EVERIFY = reject.
 * vpin_sat_verify   = my_r1csproof_verify (vPIN_proof_generation/src/commit_test.rs:340-496) with claimed inst_evals;
 * vpin_snark_verify = my_lib_verify (commit_test.rs:498-548): sat part, inst_evals, R1CSEvalProof::verify
 *                     (Spartan/src/r1csinstance.rs:356-372 -> sparse_mlpoly.rs:1535-1571) against
 *                     comm = bincode(R1CSCommitment) from vpin_spark_encode. */
int vpin_sat_verify(vpin_ctx* ctx, const uint8_t* proof, size_t proof_len, size_t num_cons, size_t num_vars,
                    const uint8_t* inputs, size_t num_inputs, const uint8_t inst_evals[96], const uint8_t* comm_para,
                    const uint8_t* comm_input);
int vpin_snark_verify(vpin_ctx* ctx, const uint8_t* proof, size_t proof_len, const uint8_t* comm, size_t comm_len,
                      const uint8_t* inputs, size_t num_inputs, const uint8_t* comm_para, const uint8_t* comm_input);
/* SHA-256 (FIPS 180-4) of n bytes, as vpin_snark_verify_batch digests its items; touches no device.  Exported for the
 * known-answer test of that digest (tests/test_sha256_kat.py), not as a service of the library. */
void vpin_sha256(const uint8_t* data, size_t n, uint8_t out32[32]);

typedef struct {
  const uint8_t* proof; size_t proof_len;
  const uint8_t* comm;  size_t comm_len;
  const uint8_t* inputs; size_t num_inputs;
  const uint8_t* comm_para; const uint8_t* comm_input;
} vpin_verify_item;

/* my_lib_verify over n proofs at once: every deferrable group equation of every proof in one random
 * linear combination. ok_out[k] = 1 accept / 0 reject; return VPIN_OK when all accept, VPIN_EVERIFY
 * when any is rejected (ok_out says which), other codes for infrastructure errors. seed32 may be NULL.
 * Each proof's transcript runs as in vpin_snark_verify (its scalar checks, byte comparisons and the points it must derive for
 * the transcript reject that proof at once); the sigma-protocol, sum-check and DotProductProofLog equations are collected as
 * (scalar, point) terms, weighted by 128-bit values drawn from SHAKE256(domain, seed32, SHA-256 of every item) and summed:
 * fixed-base terms per generator table, variable-base terms in one vpin_msm (vpin_msm_bucket from 2^17 terms on, or from
 * VPIN_VERIFY_BATCH_BUCKET_MIN terms when that is set).  When the combined sum is
 * not the identity every proof's own weighted sum is evaluated to find the rejected ones.  comm_para / comm_input hold the
 * row count the commitment's num_vars implies (32 B per row).  seed32 = NULL: 32 bytes from the operating system. */
int vpin_snark_verify_batch(vpin_ctx* ctx, const vpin_verify_item* items, size_t n, const uint8_t seed32[32], uint8_t* ok_out);
/* wall-clock spans of the last encode / snark prove on this thread, seconds: [0] encode
 * [1] derefs + commit  [2] network build  [3] product-layer proofs  [4] hash-layer proofs
 * [5] sat part  [6] whole prove  [7] unused */
void vpin_spark_last_timings(double out[8]);

/* ---- gadgets: the R1CS instances vPIN proves (host, no GPU needed) ----------------------- */
/* Owns the (A,B,C) triplets after Instance::new padding (Spartan/src/lib.rs:138-244) and the
 * three padded assignments vPIN commits to (para / input / all). */
typedef struct vpin_instance vpin_instance;
/* vPIN_proof_generation/src/point_addition.rs:67-327.  px,py,rx,ry: N x 32 LE bytes as in
 * rust_files/<label>/pointAdd/point_add_{px,py,rx,ry}_byte.json; rz: N bytes 0/1 (load_data_add.rs) */
int vpin_gadget_point_add(const uint8_t* px, const uint8_t* py, const uint8_t* rx, const uint8_t* ry,
                          const uint8_t* rz, size_t N, vpin_instance** out);
/* vPIN_proof_generation/src/point_mult.rs:61-704 (n = 128 bits, load_data.rs:62).
 * weights: N x 16 bytes (u128 little-endian, weight.json parsed as u128); px,py: N x 32 LE bytes */
int vpin_gadget_point_mult(const uint8_t* weights_le16, const uint8_t* px, const uint8_t* py, size_t N,
                           vpin_instance** out);
void vpin_instance_free(vpin_instance* g);
const vpin_r1cs* vpin_instance_r1cs(const vpin_instance* g);
size_t vpin_instance_num_cons_unpadded(const vpin_instance* g);
size_t vpin_instance_num_vars_unpadded(const vpin_instance* g);
const uint8_t* vpin_instance_vars_para(const vpin_instance* g);  /* num_vars (padded) x 32 B */
const uint8_t* vpin_instance_vars_input(const vpin_instance* g);
const uint8_t* vpin_instance_vars(const vpin_instance* g);
const uint8_t* vpin_instance_inputs(const vpin_instance* g);     /* num_inputs x 32 B or NULL */
/* Instance::is_sat (lib.rs:246-275): 1 satisfied, 0 not */
int vpin_instance_is_sat(const vpin_instance* g);
/* synthetic stand-in for the Python inference service's witness dump: count points k*G on the
 * curve E2 (src/convolution/Client.py:134-143), k from SplitMix64(seed); 32-byte LE x and y */
int vpin_synthetic_points(uint64_t seed, size_t count, uint8_t* out_x, uint8_t* out_y);

/* ---- gadgets built on the device ---------------------------------------------------------------
 * The same two gadgets with the instance never existing on the host: per-operation template replicated by
 * kernels into CSR/CSC, witness synthesis (one thread per operation), Instance::new's padding and column
 * remap, is_sat, and SNARK::encode's dense representation (addresses, read/audit timestamps) in closed form.
 * Replaces, inside the reference's timed span (proof_point_mult.rs:24-101): point_mult.rs:61-704,
 * point_addition.rs:67-327, Spartan/src/lib.rs:138-244, r1csinstance.rs:240-270, sparse_mlpoly.rs:232-265,368-438.
 * Results are bit-identical to vpin_gadget_point_* + vpin_r1cs_upload + vpin_spark_encode on the same inputs. */
typedef struct vpin_dev_instance vpin_dev_instance;
int vpin_gadget_point_add_dev(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* rx, const uint8_t* ry,
                              const uint8_t* rz, size_t N, vpin_dev_instance** out);
int vpin_gadget_point_mult_dev(vpin_ctx* ctx, const uint8_t* weights_le16, const uint8_t* px, const uint8_t* py, size_t N,
                               vpin_dev_instance** out);
void vpin_dev_instance_free(vpin_ctx* ctx, vpin_dev_instance* g);
const vpin_r1cs_dev* vpin_dev_instance_r1cs(const vpin_dev_instance* g);
const vpin_table* vpin_dev_instance_vars_para(const vpin_dev_instance* g);
const vpin_table* vpin_dev_instance_vars_input(const vpin_dev_instance* g);
const vpin_table* vpin_dev_instance_vars(const vpin_dev_instance* g);
const uint8_t* vpin_dev_instance_inputs(const vpin_dev_instance* g); /* host bytes, num_inputs x 32 B or NULL */
size_t vpin_dev_instance_num_cons_unpadded(const vpin_dev_instance* g);
size_t vpin_dev_instance_num_vars_unpadded(const vpin_dev_instance* g);
size_t vpin_dev_instance_nnz(const vpin_dev_instance* g, int m);
/* push-order triplets of matrix m (0 = A, 1 = B, 2 = C) after Instance::new's column remap, copied to the host */
int vpin_dev_instance_triplets(vpin_ctx* ctx, const vpin_dev_instance* g, int m, uint32_t* row_out, uint32_t* col_out,
                               uint8_t* val_out /* nnz x 32 B */);
/* R1CSInstance::is_sat on the device: 1 satisfied, 0 not, < 0 error */
int vpin_dev_instance_is_sat(vpin_ctx* ctx, const vpin_dev_instance* g);
/* SNARK::encode for a device-built instance (same outputs as vpin_spark_encode) */
int vpin_spark_encode_dev(vpin_ctx* ctx, const vpin_dev_instance* g, vpin_spark_decomm** out, uint8_t* comm_out,
                          size_t comm_cap, size_t* comm_len);
size_t vpin_dev_instance_comm_bytes(const vpin_dev_instance* g);
size_t vpin_dev_instance_proof_max_bytes(const vpin_dev_instance* g);
/* proof_point_mult.rs:38-94 for a device-built instance: SNARK::encode + my_lib_prove in full */
int vpin_snark_prove_dev(vpin_ctx* ctx, const vpin_dev_instance* g, const uint8_t seed_commit64[64],
                         const uint8_t seed_proof64[64], uint8_t* proof_out, size_t proof_cap, size_t* proof_len,
                         uint8_t* comm_out, size_t comm_cap, size_t* comm_len, uint8_t* comm_para_out,
                         uint8_t* comm_input_out);

/* ---- the encrypted convolution layer (the inference server's own work) ------------------------------------------
 * The homomorphic convolution over exponential-ElGamal ciphertext planes on E2 (y^2 = x^3 + a x + b over F_q; the curve of
 * vpin_synthetic_points) and the random-linear-combination check that reduces one convolution to fh*fw multiplications and
 * fh*fw - 1 additions: the type-1 path of myConv2d with rLCL / rLCR of src/convolution/Server.py and src/LeNet/Server.py.
 * A point crosses as x and y (32-byte canonical little-endian each) and an identity flag byte (1 = the identity; its x, y are
 * ignored on input apart from the range check and written as zeros on output).
 * VPIN_EINVAL: a coordinate >= q, a non-identity point off the curve (checked on the device), prf_bytes outside 1..16, a
 * zero dimension, a window that does not fit the padded plane.  vpin_last_error() names the rule. */

/* sum_i s_i * P_i: n scalars (u128 little-endian, n x 16 bytes), n points; exact for any n >= 1, identities and repeated
 * points included (one lane per term, double-and-add, complete additions in the reduction trees) */
int vpin_e2_msm(vpin_ctx* ctx, const uint8_t* scalars_le16, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t n,
                uint8_t out_x[32], uint8_t out_y[32], uint8_t* out_inf);
/* (ABI 11) Many linear combinations at once whose sums share their scalar vectors:
 *   sum[s] = sum over t < n_terms of  r[vec[s]][t] * P[base[s] + off[pat[s]][t]]        s < n_sums
 * scalars_le16: n_vec x n_terms u128 values, 16 bytes little-endian each, every one below 2^scalar_bits (scalar_bits in 1 .. 128:
 * the walk skips the windows above it).  px, py, pinf: n_points points as in vpin_e2_msm, validated on the device.  off: n_pat x
 * n_terms int32, a negative entry means "no term" (padding).  vec, pat, base: one uint32 per sum.  out_x, out_y, out_inf: n_sums
 * affine points in canonical bytes, the identity as zeros with flag 1.  Sums of one vector share a wave of a bucket walk over
 * signed 3-bit windows (e2_msm_shared.hip), so the call pays off when many sums use each vector; the sums may come in any order.
 * Exact for identity points, repeated points (the same point at every term included), P and -P in one sum, zero scalars and
 * sums with no term at all (the identity).
 * VPIN_EINVAL, the rule named in vpin_last_error(): a null argument or a zero count; scalar_bits outside 1 .. 128; a scalar with a
 * set bit at or above scalar_bits; vec[s] >= n_vec or pat[s] >= n_pat; an address base + off outside [0, n_points); a coordinate
 * >= q or a point off the curve; n_sums or n_sums * n_terms above 2^31 - 1. */
int vpin_e2_msm_shared(vpin_ctx* ctx, const uint8_t* scalars_le16, size_t n_vec, size_t n_terms, int scalar_bits, const uint8_t* px,
                       const uint8_t* py, const uint8_t* pinf, size_t n_points, const int32_t* off, size_t n_pat, const uint32_t* vec,
                       const uint32_t* pat, const uint32_t* base, size_t n_sums, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
/* The tail of a layer's RLC check as a stage of its own (rLCR of src/LeNet/Server.py and of src/cnn_networks/Server.py: the
 * products w[k] * B'[k], or s_k * X[k] in FCLayer, and the running sum the additions of the list come from): P chains of K
 * terms, term (p, k) at index p * K + k, each a u128 scalar (16 bytes little-endian) and a point.
 *   t[p][k]   = s[p][k] * X[p][k]
 *   acc[p][k] = t[p][0] + .. + t[p][k], the inclusive prefixes
 * Both as P * K affine points in canonical bytes, an identity written as zeros with flag 1.  Every addition is complete: an
 * identity term (s = 0, or a flagged X) adds nothing, equal operands double, opposite operands give the identity, and a chain
 * goes on from an identity prefix.  The prefixes are a workgroup scan, which associates differently from a left-to-right loop;
 * the group elements and therefore the bytes are the same.  One shared inversion per 256 output points.  No VPIN_ESHAPE
 * judgement is made here: the flags are reported and the layers decide.  VPIN_EINVAL: a null argument, P or K zero, P * K
 * above 2^31 - 1, a coordinate >= q, a non-identity point off the curve. */
int vpin_e2_mul_chain(vpin_ctx* ctx, const uint8_t* scalars_le16, const uint8_t* px, const uint8_t* py, const uint8_t* pinf,
                      size_t P, size_t K, uint8_t* t_x, uint8_t* t_y, uint8_t* t_inf, uint8_t* acc_x, uint8_t* acc_y,
                      uint8_t* acc_inf);
/* One plane of H x W points (row-major) under an fh x fw filter of u128 weights (row-major, 16 bytes little-endian each):
 * out[i][j] = sum_{ii,jj} w[ii][jj] * X[i*stride + ii][j*stride + jj], X = the plane padded with `pad` identities on every side;
 * oh = (H + 2 pad - fh) / stride + 1, ow likewise; out_* hold oh x ow points. */
int vpin_e2_conv2d(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t H, size_t W,
                   const uint8_t* filter_le16, size_t fh, size_t fw, size_t pad, size_t stride, uint8_t* out_x, uint8_t* out_y,
                   uint8_t* out_inf);
/* The layer: P planes (the c1 image's batch x channel planes, then the c2 image's) of H x W points under ONE filter, and per
 * plane the check  sum_t r_t * out[t] == sum_k w[k] * (sum_t r_t * window[t][k])  with
 * r_t = int.from_bytes(HMAC-SHA256(key_p, ascii_decimal(t))[:prf_bytes], "big"), t = 0 .. oh*ow - 1 row-major, restarting
 * for every plane.  keys32 = P x 32 bytes (the reference draws them with os.urandom: explicit here, like the provers' seeds).
 * The trace holds the output ciphertext and, in plane order, the multiplications (w[k], B'[k]) and the additions
 * (acc, T_k = w[k] * B'[k]; an identity T_k as rz = 1, rx = ry = 0) in the format of vpin_gadget_point_mult / _add.
 * VPIN_ESHAPE when a B'[k] or an accumulator is the identity (no witness format for it: a filter whose first tap is 0, an
 * all-identity plane); VPIN_EVERIFY when the two sides differ.  No trace is returned on failure. */
typedef struct vpin_conv_trace vpin_conv_trace;
int vpin_enc_conv2d(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t H, size_t W,
                    const uint8_t* filter_le16, size_t fh, size_t fw, size_t pad, size_t stride, const uint8_t* keys32, int prf_bytes,
                    vpin_conv_trace** out);
void vpin_conv_trace_free(vpin_conv_trace* t);
/* out = {P, oh, ow, multiplications, additions} */
int vpin_conv_trace_dims(const vpin_conv_trace* t, size_t out[5]);
/* Borrowed views, valid until vpin_conv_trace_free: the output ciphertext (P x oh x ow points) */
int vpin_conv_trace_output(const vpin_conv_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf);
/* the multiplication list: weights n x 16 bytes, points n x 32 bytes each */
int vpin_conv_trace_mults(const vpin_conv_trace* t, const uint8_t** weights_le16, const uint8_t** px, const uint8_t** py);
/* the addition list: n x 32 bytes each, rz n bytes */
int vpin_conv_trace_adds(const vpin_conv_trace* t, const uint8_t** px, const uint8_t** py, const uint8_t** rx, const uint8_t** ry,
                         const uint8_t** rz);
/* the left side sum_t r_t * out[t] of every plane (P points) */
int vpin_conv_trace_left(const vpin_conv_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf);
/* the two lists through vpin_gadget_point_mult_dev / vpin_gadget_point_add_dev: instances ready for vpin_snark_prove_dev
 * (*add_out stays NULL for a 1 x 1 filter, which has no additions, *mult_out for a pooling trace, which has no
 * multiplications); free them with vpin_dev_instance_free */
int vpin_conv_trace_instances(vpin_ctx* ctx, const vpin_conv_trace* t, vpin_dev_instance** mult_out, vpin_dev_instance** add_out);
/* wall-clock spans of the last encrypted-layer call on this thread (vpin_enc_conv2d, vpin_enc_fc, vpin_enc_avgpool2d), seconds:
 * [0] validate (upload + checks)  [1] the layer's own compute: convolution, matrix-vector product (+ bias) or pooling
 * (+ normalisation, outputs to the host)  [2] PRF (HMAC-SHA256, host team)  [3] RLC sums  [4] host tail  [5] total; a stage the
 * layer does not have (pooling: PRF, RLC) reads 0 */
void vpin_enc_conv_last_timings(double out[8]);
/* (ABI 9) Which units made the last encrypted-layer call on this thread answer VPIN_ESHAPE: the planes p of vpin_enc_conv2d,
 * vpin_enc_avgpool2d and (ABI 12) vpin_enc_add, the groups g of vpin_enc_conv2d_mc[_bias], the rows p of vpin_enc_fc[_signed] (for these the folded weight
 * that does not fit 128 bits and the accumulator rule of the chain included).  Ascending, no duplicates: at most cap of them
 * into units, *n is their number.  The code and the text of the call stay the first hit's; the scan that refuses runs to its end
 * and names every unit that breaks ITS rule.  A call that fails at one stage names that stage's units only: the later stages were
 * not reached, so a unit not named may still break a later rule.  Every layer entry point clears the list on entry, and it stays
 * empty after VPIN_OK and after VPIN_EVERIFY, VPIN_EINVAL, VPIN_EHIP and VPIN_ENOMEM, which are not a unit's doing or cannot be
 * attributed here.  VPIN_EINVAL for n = NULL, or units = NULL with cap > 0 */
int vpin_enc_last_refusals(uint32_t* units, size_t cap, size_t* n);

/* The fully connected layer: FCLayer (flag 1) with the type-1 branch of rLCL / rLCR of src/LeNet/Server.py, where the random
 * scalars fold into the WEIGHTS.  P rows of K input points (the c1 vector, then the c2 vector), one K x N matrix of u32 weights
 * (W[k][j] row-major, 4 bytes little-endian each), P x N encrypted bias points and one 32-byte key per row.  Per row p, in
 * this order:
 *   1. C[j] = sum_k W[k][j] * X[k], out[j] = C[j] + bias[j]: N additions (C[j], bias[j]); an identity bias as rz = 1,
 *      rx = ry = 0.  VPIN_ESHAPE if a C[j] is the identity (an accumulator has no flag).
 *   2. r_j = the PRF of vpin_enc_conv2d under key_p, j = 0 .. N - 1; left = sum_j r_j * C[j] (over C, not out).
 *   3. s_k = sum_j r_j * W[k][j] as an exact integer; VPIN_ESHAPE if an s_k does not fit 128 bits (the gadget's weights are
 *      u128; with u32 weights it stays far below q, so the reference's reduction mod the base field never fires).
 *   4. K multiplications (s_k, X[k]); VPIN_ESHAPE if an X[k] is the identity.
 *   5. T_k = s_k * X[k]; acc = T_0 and, for k >= 1, the addition (acc, T_k), then acc += T_k: K - 1 additions; an identity
 *      T_k as rz = 1.  VPIN_ESHAPE if acc is the identity before a step.
 *   6. VPIN_EVERIFY unless acc == left.
 * The trace's dims are {P, 1, N, P * K, P * (N + K - 1)}; its output is out (P x N points, an identity allowed and flagged),
 * its left sides are P points.  VPIN_EINVAL as for vpin_enc_conv2d, for the inputs and the bias: a null argument, P, K or N
 * zero, prf_bytes outside 1..16, a coordinate >= q, a point off the curve.  No trace is returned on failure. */
int vpin_enc_fc(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t K,
                const uint8_t* weights_le4, size_t N, const uint8_t* bx, const uint8_t* by, const uint8_t* binf,
                const uint8_t* keys32, int prf_bytes, vpin_conv_trace** out);
/* The fully connected layer of a trained model: vpin_enc_fc over int32 weights (K x N row-major, signed).  The same arguments,
 * trace, dims and rules; what the signs change, per row:
 *   1. C[j] = sum_k W[k][j] * X[k] with a negative weight adding |w| times -X[k].  A C[j] that is the identity (VPIN_ESHAPE) is
 *      now reachable by plain inputs: X[0] = X[1] under the weights w, -w.
 *   3. s_k = sum_j r_j * W[k][j] = pos_k - neg_k, two unsigned sums over the positive and the negative weights (|INT32_MIN| =
 *      2^31); VPIN_ESHAPE if either leaves 128 bits.
 *   4. the multiplication is (|s_k|, S_k), S_k = X[k] for s_k >= 0 and -X[k] = (x, q - y) for s_k < 0: the gadget's weight is a
 *      u128 bit string, so the sign goes into the point (as in vpin_enc_conv2d_mc).  s_k = 0 records (0, X[k]).
 *   5. T_k = |s_k| * S_k, and the chain as before.
 * With every weight non-negative the trace is vpin_enc_fc's byte for byte. */
int vpin_enc_fc_signed(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t K,
                       const int32_t* weights, size_t N, const uint8_t* bx, const uint8_t* by, const uint8_t* binf,
                       const uint8_t* keys32, int prf_bytes, vpin_conv_trace** out);
/* The average pooling: myAvgPool2d (type1 = 1, flag = 1) of src/LeNet/Server.py over P planes of H x W points with a k x k
 * window.  oh = (H - k) / stride + 1, ow likewise, outputs row-major.  Per output, with the window's elements e_0 .. e_{k*k-1}
 * taken row-major: acc = e_0 and, for m >= 1, the addition (acc, e_m), then acc += e_m; out = scale * acc (scale: u128
 * little-endian; the reference's is 2^10 / k^2).  An identity e_m, m >= 1, is written as rz = 1.  VPIN_ESHAPE if an accumulator is
 * the identity (e_0 is, or a partial sum cancels before the last step); the last sum may be the identity, the output is then
 * flagged.  No multiplication is recorded and no RLC check runs: dims are {P, oh, ow, 0, P * oh * ow * (k*k - 1)},
 * vpin_conv_trace_mults and _left give NULL views, vpin_conv_trace_instances leaves *mult_out NULL (and *add_out too for
 * k = 1).  VPIN_EINVAL: a null argument, a zero dimension, k > H, k > W, stride = 0, a coordinate >= q, a point off the curve. */
int vpin_enc_avgpool2d(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t H, size_t W,
                       size_t k, size_t stride, const uint8_t scale_le16[16], vpin_conv_trace** out);

/* The trained convolution layer: one filter per (output channel, input channel), signed weights, the channel mixing inside the
 * proven check.  The reference's convolution is one non-negative filter for all planes with the channels summed beforehand and
 * unproven (vpin_e2_plane_sums); this is its own check -- myConv2d type 1 with rLCL / rLCR type 0 -- per output plane with one
 * chain over all (channel, tap) terms.  groups x C planes of H x W points, group-major (a group: the c1 or the c2 image, or a batch
 * element); weights W[o][c][ii][jj] as n_out * C * fh * fw int32, row-major; connect[o][c], n_out * C bytes, non-zero = connected,
 * NULL = all connected (the table is architecture, public; weights of unconnected pairs are not read).
 *   out[g][o][i][j] = sum_{c connected to o} sum_{ii,jj} W[o][c][ii][jj] * X[g][c][i*stride + ii][j*stride + jj]
 * X padded with identities; the output planes are group-major, then o.  One key per (g, o), group-major: keys32 = groups * n_out
 * x 32 bytes.  The check per (g, o), with r_t the PRF of vpin_enc_conv2d under that pair's key:
 *   left = sum_t r_t * out[g][o][t];  B'[c][k] = sum_t r_t * window_t(X[g][c])[k] for the connected c ascending, the taps k row-major.
 *   Term m = (c, k) in that order records the multiplication (|w_m|, S_m), S_m = B'[c][k] for w_m >= 0 and -B'[c][k] = (x, q - y)
 *   for w_m < 0: the gadget's weights are u128, so the sign goes into the point.  T_m = |w_m| * S_m; acc = T_0 and every later
 *   term records the addition (acc, T_m), an identity T_m as rz = 1; acc == left at the end.
 * VPIN_ESHAPE when a B'[c][k] is the identity or the accumulator is the identity before a step (as in vpin_enc_conv2d: a zero
 * FIRST weight of a pair's chain, an all-identity connected channel, terms that cancel before the last step; the accumulator
 * after the last step may be the identity, it is only compared).  VPIN_EVERIFY when the two sides differ.  VPIN_EINVAL as for
 * vpin_enc_conv2d, and for groups, C or n_out zero and a row of connect that selects no channel.
 * The trace's dims are {groups * n_out, oh, ow, M, M - groups * n_out} with M = groups * fh * fw * (connected pairs); with
 * C = n_out = 1, groups = P and non-negative weights it is vpin_enc_conv2d's trace byte for byte. */
int vpin_enc_conv2d_mc(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C, size_t n_out,
                       size_t H, size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw, size_t pad, size_t stride,
                       const uint8_t* keys32, int prf_bytes, vpin_conv_trace** out);
/* The trained convolution with a bias per output channel (nn.Conv2d's): vpin_enc_conv2d_mc plus bx, by, binf, groups * n_out
 * encrypted bias points, group-major then o; an identity bias is allowed and flagged.  C is what vpin_enc_conv2d_mc calls out;
 *   out[g][o][t] = C[g][o][t] + bias[g][o]
 * and the check runs over C, not out (as in vpin_enc_fc).  The multiplication list and the left sides are those of
 * vpin_enc_conv2d_mc on the same inputs and keys, byte for byte.  The addition list per (g, o) is first the oh * ow additions
 * (C[t], bias[g][o]), t row-major, an identity bias as rz = 1, rx = ry = 0, then that pair's chain additions as before.  out =
 * identity (bias = -C[t]) and C[t] = bias (a doubling) are cases of the addition, not errors.  Dims: {groups * n_out, oh, ow, M,
 * M - groups * n_out + groups * n_out * oh * ow}.  VPIN_ESHAPE also when a C[t] is the identity: it is the first operand of an
 * addition, which has no flag.  VPIN_EINVAL also for a null bias array, a bias coordinate >= q or a bias point off the curve. */
int vpin_enc_conv2d_mc_bias(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C,
                            size_t n_out, size_t H, size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw,
                            size_t pad, size_t stride, const uint8_t* bx, const uint8_t* by, const uint8_t* binf, const uint8_t* keys32,
                            int prf_bytes, vpin_conv_trace** out);
/* (ABI 12) The addition layer: the skip connection of a residual block.  Two encrypted tensors of the same shape, P planes of
 * H x W points each (px, py, pinf: the first operand X; rx, ry, rinf: the second operand R);
 *   out[p][t] = X[p][t] + R[p][t]
 * the complete addition by case, as for the bias above with one second operand per element instead of one per plane.  No
 * multiplication is recorded and no RLC check runs: dims are {P, H, W, 0, P * H * W}, vpin_conv_trace_mults and _left give NULL
 * views (as for pooling) and vpin_conv_trace_instances leaves *mult_out NULL.  The addition list is plane-major, then t
 * row-major: (X[p][t], R[p][t], rz) with rz R's identity flag, an identity R written as rx = ry = 0.  R[p][t] = X[p][t] (a
 * doubling) and R[p][t] = -X[p][t] (out is the flagged identity) are cases of the addition, not errors, exactly as for the bias;
 * like there, such a row makes the add instance unsatisfiable: the gadget's addition is the chord rule, which neither case meets.
 * VPIN_ESHAPE when an X[p][t] is the identity: it is the first operand of an addition, which has no flag; the text names the
 * first such plane and element, vpin_enc_last_refusals every such plane.  VPIN_EINVAL: a null argument, a zero dimension, H or W
 * above 2^24, more than 65535 planes, 2^31 points or more, a coordinate >= q, a point off the curve (the text says "first
 * operand" or "second operand").  vpin_enc_conv_last_timings: [0] validate, [1] the additions, [4] host tail, [5] total. */
int vpin_enc_add(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, const uint8_t* rx, const uint8_t* ry,
                 const uint8_t* rinf, size_t P, size_t H, size_t W, vpin_conv_trace** out);
/* the bare stage beside vpin_e2_conv2d: the output ciphertext only (groups * n_out * oh * ow points), no check; a cancelled
 * output is the flagged identity */
int vpin_e2_conv2d_mc(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C, size_t n_out,
                      size_t H, size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw, size_t pad, size_t stride,
                      uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);

/* ---- the client side: exponential ElGamal on E2 (key generation, encryption, decryption with a discrete-log table) ------
 * What the reference's client does around every layer (src/LeNet/Client.py: encrypt, decrypt, bsgs): with the generator G of
 * prime order n, a key sk and H = sk * G, a signed message m is (c1, c2) = (r * G, m * G + r * H), and
 * m = log_G(c2 - sk * c1) is found by baby steps / giant steps.  The randomness r and the key are explicit inputs, like the
 * provers' seeds.  Points cross as in vpin_e2_msm (an identity is written as zeros with flag 1); scalars mod n as 32 bytes
 * little-endian; messages as int64_t.
 * VPIN_EINVAL: a null argument, cnt = 0, a scalar >= n (for r and sk also 0), |msg| >= 2^62, a coordinate >= q or a point off
 * the curve (checked on the device), an identity base point, nb outside 2 .. 2^28, max_giant * nb past 2^62.  VPIN_ENOMEM: a
 * table does not fit.  vpin_last_error() names the rule.  A table belongs to the context that made it and is freed before it. */

/* window table of one fixed base point B, device-resident: the affine points d * 2^(10 k) * B for every window k and digit d
 * (1.7 MB), so that s * B is at most 26 mixed additions and no doubling.  x = y = NULL: B = G */
typedef struct vpin_e2_base vpin_e2_base;
int vpin_e2_base_create(vpin_ctx* ctx, const uint8_t* x, const uint8_t* y, vpin_e2_base** out);
/* the same with an explicit window width w in 4 .. 12 (tools/time_e2_client.py measures the widths; 10 is the default) */
int vpin_e2_base_create_w(vpin_ctx* ctx, const uint8_t* x, const uint8_t* y, int w, vpin_e2_base** out);
void vpin_e2_base_free(vpin_e2_base* b);
/* out[i] = s_i * B, 0 <= s_i < n (s_i = 0 gives the flagged identity) */
int vpin_e2_base_mul(vpin_ctx* ctx, const vpin_e2_base* b, const uint8_t* scalars_le32, size_t cnt, uint8_t* out_x, uint8_t* out_y,
                     uint8_t* out_inf);
/* out[i] = s_i * P_i, 0 <= s_i < n, by double-and-add: the variable-base form (decryption multiplies every c1 by sk with it) */
int vpin_e2_mul256(vpin_ctx* ctx, const uint8_t* scalars_le32, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt,
                   uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
/* c1[i] = r_i * G, c2[i] = msg_i * G + r_i * H; baseG / baseH: the tables of G and of the public key H = sk * G
 * (vpin_e2_base_mul of sk under baseG).  The last addition is complete: c2 may be the identity (flagged).  One launch chain
 * for all cnt elements */
int vpin_e2_encrypt(vpin_ctx* ctx, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const int64_t* msgs, const uint8_t* r_le32,
                    size_t cnt, uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf);
/* (ABI 7) vpin_e2_encrypt with one public key per element and no table of any H: c1[i] = r_i * G, c2[i] = msg_i * G + r_i *
 * H[key_of[i]].  hx, hy: n_pub public keys, canonical little-endian, n_pub x 32 bytes each.  r * G and msg * G come from G's
 * table as in vpin_e2_encrypt; r * H is a double-and-add over the key's affine coordinates, one lane per element, a launch of
 * its own in the same chain.  The results are canonical, so they are byte for byte those of vpin_e2_encrypt under a table of
 * the same H.  For many elements under few keys a table per key is faster; this form is for a server that
 * encrypts a few hundred values under each of many clients' keys.
 * VPIN_EINVAL, each with its rule in vpin_last_error(): a null argument, cnt = 0, n_pub = 0, a key_of[i] >= n_pub (the first
 * such i is named), a public key that is the identity, has a coordinate >= q or is off the curve (the key's index is named),
 * and, as in vpin_e2_encrypt, r_i = 0, r_i >= n, |msg_i| >= 2^62 */
int vpin_e2_encrypt_keyed(vpin_ctx* ctx, const vpin_e2_base* baseG, const uint8_t* hx, const uint8_t* hy, size_t n_pub, const uint32_t* key_of,
                          const int64_t* msgs, const uint8_t* r_le32, size_t cnt, uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x,
                          uint8_t* c2y, uint8_t* c2inf);
/* the baby steps j * G, 0 <= j < nb, device-resident: 32 bytes of x and a parity byte per entry and an open-addressing index
 * of 2^ceil(log2(2 nb)) 64-bit slots (49 to 65 bytes per entry in all; 2^24 entries: 0.8 GB).  2 <= nb <= 2^28 */
typedef struct vpin_e2_dlog vpin_e2_dlog;
int vpin_e2_dlog_create(vpin_ctx* ctx, uint64_t nb, vpin_e2_dlog** out);
void vpin_e2_dlog_free(vpin_e2_dlog* t);
/* out = {nb, device bytes held} */
int vpin_e2_dlog_info(const vpin_e2_dlog* t, uint64_t out[2]);
/* v_out[i] = the v with P_i = v * G and |v| <= max_giant * nb + nb - 1, found_out[i] = 1; found_out[i] = 0 (and v_out[i] = 0)
 * when there is none in that range, which is not an error.  Exact: a hit is confirmed on the full coordinates, never on a
 * truncated hash.  A step is two affine additions whose inversion the lanes of a workgroup share; a point has up to 64 lanes
 * that take the giant steps in turn, so the walk is max_giant / 64 to max_giant shared inversions deep */
int vpin_e2_dlog_solve(vpin_ctx* ctx, const vpin_e2_dlog* t, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt,
                       uint64_t max_giant, int64_t* v_out, uint8_t* found_out);
/* M_i = c2_i - sk * c1_i, then as vpin_e2_dlog_solve */
int vpin_e2_decrypt(vpin_ctx* ctx, const vpin_e2_dlog* t, const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y,
                    const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint64_t max_giant,
                    int64_t* v_out, uint8_t* found_out);
/* One round of the client between two layers: what main of src/LeNet/Client.py does with one message of the server
 * (receive_decrypt, then relu and / or shifting, then encryptInputImage_send), as ONE launch chain on the context's stream with
 * no host copy between the decryption and the encryption: sk * c1, the subtraction, the walk of vpin_e2_dlog_solve, the
 * activation, the three fixed-base multiplications of vpin_e2_encrypt.
 *   v_out[i]    the raw decryption
 *   act_out[i]  a = v, then max(a, 0) when relu != 0, then, when shift_bits != 0, the reference's shifting(a, shift_bits) =
 *               (float32(a) / 2^shift_bits * 2^16).astype(int32): a rounded to nearest-even into float32, an exact power-of-two
 *               scale, truncation toward zero.  This is not the integer shift of a: the rounding into float32 comes first.
 *   c1o / c2o   the encryption of act_out under r_le32 (cnt scalars, as for vpin_e2_encrypt); reencrypt = 0 is the last round:
 *               nothing is encrypted and baseG, baseH, r_le32 and the six outputs may be NULL
 * VPIN_ESHAPE, with the first such index named in vpin_last_error(): an element has no value within +-(max_giant * nb + nb - 1)
 * (the activation needs every value), or its shifted value does not fit int32 (numpy's result is undefined there), or
 * without a shift |act| >= 2^62.  v_out and act_out are written all the same (0 at such an element's act_out).
 * VPIN_EINVAL as for vpin_e2_decrypt and vpin_e2_encrypt, and shift_bits outside 0 .. 62. */
int vpin_e2_client_round(vpin_ctx* ctx, const vpin_e2_dlog* t, const vpin_e2_base* baseG, const vpin_e2_base* baseH,
                         const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                         const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint64_t max_giant, int relu, int shift_bits, int reencrypt,
                         const uint8_t* r_le32, int64_t* v_out, int64_t* act_out, uint8_t* c1ox, uint8_t* c1oy, uint8_t* c1oinf,
                         uint8_t* c2ox, uint8_t* c2oy, uint8_t* c2oinf);
/* (ABI 13) vpin_e2_client_round with max pooling between the decryption and the activation: the server cannot take a maximum of
 * ElGamal ciphertexts, the client, which decrypts every value anyway, can.  The cnt = planes * H * W inputs are `planes` planes of
 * H x W values, row-major; Ho = (H - k) / stride + 1 and Wo = (W - k) / stride + 1, rounded down, a remainder of rows or columns
 * dropped as in vpin_enc_avgpool2d; cnt_out = planes * Ho * Wo.  The same launch chain (the activation launch is
 * e2_act_pool_kernel, one lane per output element; the encryption runs over cnt_out elements); a window never crosses a plane.
 *   v_out[cnt]        the raw decryptions, every one, also of elements that belong to no window (0 where the walk met no value)
 *   act_out[cnt_out]  for output (p, oy, ox): a = the maximum of v[p][oy stride + i][ox stride + j] over 0 <= i, j < k, then
 *                     max(a, 0) when relu, then shifting(a, shift_bits) when shift_bits != 0, exactly as above.  ReLU and shifting
 *                     are non-decreasing (the rounding to float32, the exact power-of-two scale and the truncation toward zero each
 *                     preserve order), so this IS the elementwise activation followed by the maximum: act(max v) = max act(v)
 *   c1o / c2o         cnt_out points: act_out under cnt_out scalars of r_le32; reencrypt = 0 (the last round may pool): nothing is
 *                     encrypted and baseG, baseH, r_le32 and the six outputs may be NULL
 * k = 1, stride = 1 gives vpin_e2_client_round's bytes.
 * VPIN_ESHAPE: "element i, inside a window, has no value within the walk's range" with the first such INPUT index (the walk's
 * found bytes are read back on this path only; an element that belongs to no window -- a dropped remainder, a gap of stride > k
 * -- is no error); then "the activated value of output element o (the maximum decrypted, a) does not fit" with the first such
 * OUTPUT index, by vpin_e2_client_round's rules.
 * VPIN_EINVAL: everything vpin_e2_client_round rejects (r_le32: cnt_out scalars), and, each with its text: planes, H or W zero;
 * k or stride zero; k > H or k > W; planes * H * W >= 2^30. */
int vpin_e2_client_round_pool(vpin_ctx* ctx, const vpin_e2_dlog* t, const vpin_e2_base* baseG, const vpin_e2_base* baseH,
                              const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                              const uint8_t* c2y, const uint8_t* c2inf, size_t planes, size_t H, size_t W, size_t k, size_t stride,
                              uint64_t max_giant, int relu, int shift_bits, int reencrypt, const uint8_t* r_le32, int64_t* v_out,
                              int64_t* act_out, uint8_t* c1ox, uint8_t* c1oy, uint8_t* c1oinf, uint8_t* c2ox, uint8_t* c2oy, uint8_t* c2oinf);

/* ---- the channel sums of the LeNet server loop ---------------------------------------------------------------------------
 * secondConv and thirdConv of src/LeNet/Server.py add whole ciphertext planes pixel by pixel (np.sum(planes, axis=0)) before
 * the convolution: out[o][p] = sum over the input planes j with connect[o][j] != 0 of in[j][p], for n_in planes of H x W points
 * (plane-major, row-major inside a plane), a table of n_out x n_in bytes and n_out output planes.  thirdConv is the table of
 * all ones.  The additions are complete: an identity pixel adds nothing, the same point in two planes doubles, P and -P
 * cancel to a flagged identity (zeros, flag 1), which is not an error -- the convolution takes identity pixels.  These
 * additions belong to no witness list (the reference does not prove them).
 * VPIN_EINVAL: a null argument, a zero dimension, a row of the table that selects no plane, a coordinate >= q, a point off the
 * curve; n_in or n_out above 65535, or 2^31 points or more on either side. */
int vpin_e2_plane_sums(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t n_in, size_t H, size_t W,
                       const uint8_t* connect, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
/* (ABI 8) vpin_e2_plane_sums over `groups` sets of planes under the one table, by one upload, one kernel launch and one copy
 * back: groups x n_in planes in, group-major, groups x n_out planes out; group g's output is byte for byte what
 * vpin_e2_plane_sums gives on group g's planes alone.  A batch of B images hands its 2 B halves (image b's c1 planes, then its c2
 * planes) as the groups.  VPIN_EINVAL as there, naming vpin_e2_plane_sums_batch: a point off the curve fails the whole call;
 * groups above 65535, or 2^31 points or more on either side over all groups */
int vpin_e2_plane_sums_batch(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t n_in,
                             size_t H, size_t W, const uint8_t* connect, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);

/* ---- the whole encrypted LeNet inference ---------------------------------------------------------------------------------
 * What inferenceCNN of src/LeNet/Server.py and main of src/LeNet/Client.py do together: the encrypted image goes in, the
 * encrypted class scores come out, and with them the witness lists of the seven labels L1 .. L7 the prover takes.
 *   L1 conv1: n1 kernels, each the one filter over the c1 image and then over the c2 image   R1: ReLU
 *   L2 pool1 on each of the 2 n1 planes                                                       R2: shifting(., 26)
 *   L3 conv2: per output the connected planes summed (vpin_e2_plane_sums), then the filter    R3: ReLU
 *   L4 pool2                                                                                  R4: shifting(., 26)
 *   L5 conv3: n3 times the sum of all n2 planes through the filter -> 1 x 1                   R5: ReLU, shifting(., 26)
 *   L6 FC1 n3 -> N1: the bias encrypted by the server, FCLayer on the c1 row, then the c2 row R6: ReLU, shifting(., 33)
 *   L7 FC2 N1 -> N2                                                                           R7: ReLU, the result
 * A label's lists are those of its layer call (vpin_enc_conv2d, vpin_enc_avgpool2d, vpin_enc_fc) over the planes in the order
 * (kernel 0, c1), (kernel 0, c2), (kernel 1, c1), ..; the plane additions of the channel sums enter no list (the reference does
 * not prove them).  Keys and randomness are the caller's, consumed in the order the reference draws them: one 32-byte key per
 * myConv2d / FCLayer call in call order (2 n1 + 2 n2 + 2 n3 + 4), one r per encrypt call of encryptBias (N1, then N2). */
typedef struct vpin_lenet_cfg {
  size_t H, W;                   /* the image (square) */
  size_t n1, n2, n3;             /* kernels of the three convolutions */
  const uint8_t* connect;        /* n2 x n1 bytes: conv2's output o takes input plane j when connect[o * n1 + j] != 0 (conv3: all) */
  size_t f;                      /* the one f x f filter .. */
  const uint8_t* filter_le16;    /* .. of u128 weights, row-major, 16 bytes little-endian each */
  size_t pool_k, pool_stride;
  uint8_t pool_scale_le16[16];   /* u128, the reference's 2^10 / k^2 */
  int relu[7], shift_bits[7];    /* per round R1 .. R7: ReLU or not, the bits of shifting (0: none) */
  uint64_t max_giant[7];         /* per round: the discrete-log range of the ready-made client */
  int prf_bytes;
  size_t N1, N2;
  const int32_t *w1, *w2;        /* n3 x N1 and N1 x N2, row-major, non-negative: the 16-bit fixed point of the model's weights */
  const int64_t *b1, *b2;        /* N1 and N2 bias values */
} vpin_lenet_cfg;
/* the reference's network: 32 x 32, 6 / 16 / 120 kernels, 5 x 5, pooling 2 / 2 with scale 256, the rounds of the table above,
 * 13 PRF bytes, 84 and 10 outputs; max_giant for a table of 2^24 baby steps (2^11 giant steps, 2^15 for R6 and R7, whose values
 * reach 2^38.4).  The connection table, the filter and the weights stay NULL: they are the caller's data */
int vpin_lenet_cfg_default(vpin_lenet_cfg* cfg);
/* what a run consumes: out[0..6] multiplications and out[7..13] additions of L1 .. L7, out[14..20] decryptions of R1 .. R7,
 * out[21] decryptions in all, out[22] client encryptions (the image included), out[23] PRF keys, out[24] bias r.  VPIN_EINVAL for
 * a zero dimension, a window that does not fit, a third convolution whose output is not 1 x 1, a connection row without a plane */
int vpin_lenet_cfg_counts(const vpin_lenet_cfg* cfg, size_t out[32]);
/* One interaction with the client (interactionClient / receiveEncryptedImage of Server.py): round = 0 .. 6, flags =
 * VPIN_LENET_RELU | VPIN_LENET_REENCRYPT, cnt ciphertexts (c1, c2) out, the activated values encrypted again back (the six
 * outputs are NULL in the last round, which has no VPIN_LENET_REENCRYPT).  Returns VPIN_OK or an error code; the error text is
 * cleared before the call, and a callback that fails without setting one is reported as "the round callback failed" */
#define VPIN_LENET_RELU 1
#define VPIN_LENET_REENCRYPT 2
/* (ABI 13) vpin_net_infer and its family only: the round pools by maximum, the six outputs hold fewer points (vpin_net_round_pool) */
#define VPIN_LENET_MAXPOOL 4
typedef int (*vpin_lenet_round_fn)(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y,
                                   const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt,
                                   uint8_t* c1ox, uint8_t* c1oy, uint8_t* c1oinf, uint8_t* c2ox, uint8_t* c2oy, uint8_t* c2oinf);
typedef struct vpin_lenet_trace vpin_lenet_trace;
/* The server loop: the table above as seven steps of the driver vpin_net_infer runs too, here with the planes interleaved, the
 * plane sums before L3 and L5 and the repeats of L1 and L5.  The driver holds no secret key: baseG / baseH (the client's public
 * key) are there because the server encrypts the bias itself.  What the client sends back is validated by the layer that takes
 * it.  A failing layer or round frees everything, returns its code and names the label or round in vpin_last_error()
 * ("vpin_lenet_infer: L3: ..", "vpin_lenet_infer: R6: ..").  VPIN_EINVAL also for a negative weight and for n_keys / n_bias_r
 * other than vpin_lenet_cfg_counts says */
int vpin_lenet_infer(vpin_ctx* ctx, const vpin_lenet_cfg* cfg, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                     const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH,
                     const uint8_t* keys32, size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn,
                     void* user, vpin_lenet_trace** out);
void vpin_lenet_trace_free(vpin_lenet_trace* t);
/* label 1 .. 7 as the trace of its layer call, borrowed until vpin_lenet_trace_free: vpin_conv_trace_dims / _output / _mults /
 * _adds / _left read it (the pooling labels have no multiplications) */
int vpin_lenet_trace_label(const vpin_lenet_trace* t, int label, const vpin_conv_trace** out);
/* a label's two lists through vpin_gadget_point_mult_dev / _add_dev, as vpin_conv_trace_instances */
int vpin_lenet_trace_instances(vpin_ctx* ctx, const vpin_lenet_trace* t, int label, vpin_dev_instance** mult_out,
                               vpin_dev_instance** add_out);
/* the last layer's ciphertext: 2 x n points, the c1 row and then the c2 row */
int vpin_lenet_trace_result(const vpin_lenet_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf, size_t* n);
/* host-clock milliseconds of the last vpin_lenet_infer on this thread: [0..6] L1 .. L7, [7..13] R1 .. R7, [14] the whole */
void vpin_lenet_last_timings(double out[16]);
/* The ready-made client is vpin_net_client below, made for the seven rounds: vpin_net_client_create(.., n_rounds = 7, ..) */

/* ---- an encrypted inference as a list of layers: the CNN A .. E service ---------------------------------------------------
 * What inferenceCNN of src/cnn_networks/Server.py and main of src/cnn_networks/Client.py do together, for any list of layers
 * over C planes of H x W ciphertexts (c1 and c2 apart, C * H * W points each, plane-major):
 *   VPIN_NET_CONV  one fh x fw filter of u128 weights with pad and stride over each of the C c1 planes and then each of the C c2
 *                  planes, one PRF key per plane in that order: vpin_enc_conv2d with P = 2 C (callConv2_ciphertext on c1, then
 *                  on c2).  LeNet's order is (kernel 0 c1, kernel 0 c2, ..): the one driver takes either
 *   VPIN_NET_POOL  k x k windows with a stride and a u128 scale: vpin_enc_avgpool2d over the c1 planes, then the c2 planes
 *   VPIN_NET_FC    K = the incoming C * H * W, flattened channel-major (flatten), N outputs, int32 weights K x N row-major and
 *                  non-negative, int64 bias: the server encrypts the bias under baseH with the caller's r, N values drawn
 *                  before the layer (encryptBias), then vpin_enc_fc with P = 2, the c1 row and then the c2 row, one key each.
 *                  After it C = 1, H = 1, W = N
 * After a layer comes, when has_round != 0, one interaction with the client: relu, shift_bits (0: none) as in
 * vpin_e2_client_round, reencrypt = 0 only on the last layer (the result stays with the client); max_giant is the range the
 * ready-made client is to be given for that round.  A layer without a round hands its ciphertext straight to the next layer.
 * Rounds are numbered 0, 1, .. over the layers that have one; layers 0, 1, .. in list order.
 * In cnn_networks all layers append to the same four global lists (points_mult, weights_array, point_one_Add, point_two_Add),
 * so a network has ONE label: the multiplication lists and the addition lists of its layers concatenated in layer order. */
#define VPIN_NET_CONV 0
#define VPIN_NET_POOL 1
#define VPIN_NET_FC 2
/*   VPIN_NET_CONVMC  the trained convolution: vpin_enc_conv2d_mc with groups = 2 (the C c1 planes, then the C c2 planes) under
 *                  n_out x C filters of fh x fw int32 weights (w_mc) and the optional table connect; 2 n_out keys, (c1, o) first;
 *                  n_out planes go on.  Its fields stand at the END of vpin_net_layer (ABI 3); the other kinds read none of them */
#define VPIN_NET_CONVMC 3
/*   (ABI 4) A CONVMC layer reads `bias`: NULL is the layer without one; otherwise n_out int64 values, which the server encrypts as
 *                  for FC (n_out of the caller's r, drawn before the layer) and hands to vpin_enc_conv2d_mc_bias, the c1 halves for
 *                  group 0 and the c2 halves for group 1: n_out more bias r and 2 n_out oh ow more additions
 *   VPIN_NET_FCS   VPIN_NET_FC over signed weights: K, N, w, bias as there, vpin_enc_fc_signed with P = 2; the same counts.
 *                  VPIN_NET_FC itself still answers VPIN_EINVAL for a negative weight */
#define VPIN_NET_FCS 4
/*   (ABI 8) What the reference's LeNet needs of a layer, again at the END of vpin_net_layer and all zero for today's behaviour:
 *   sum_table, sum_out  CONV: before the layer the channel sums (vpin_e2_plane_sums_batch over the 2 B halves) by a table of
 *                  sum_out x C bytes, C the planes that reach the layer; the layer then sees C = sum_out.  They enter no list
 *   repeat         CONV: the planes are handed to the call `repeat` times over (0 or 1: once), every one of the 2 C repeat
 *                  planes under a key of its own; C repeat planes go on
 *   plane_order    CONV and POOL: 0 the blocked order above, VPIN_NET_ORDER_INTERLEAVED LeNet's (0, c1), (0, c2), (1, c1), ..
 *                  for the call's planes, its keys and its output.  With a repeat the blocked order is the image's c1 planes
 *                  `repeat` times, then its c2 planes
 * vpin_lenet_as_net writes the reference's LeNet as such a list */
#define VPIN_NET_ORDER_INTERLEAVED 1
/*   (ABI 12) Tensor references, again at the END of vpin_net_layer and all zero for today's behaviour: a layer may read a tensor
 *   other than its predecessor's, and VPIN_NET_ADD adds two of them (a skip connection).  A reference on layer i is
 *     0                    the default: for input_from the previous layer's output (the encrypted input on layer 0), for
 *                          skip_from "none"
 *     k in 1 .. i          the output of layer k - 1 as the server holds it after that layer's round, or straight after the
 *                          layer when it has no round
 *     VPIN_NET_FROM_INPUT  the inference's encrypted input
 *   input_from     any kind: what the layer reads; the shape that reaches the layer is that tensor's
 *   skip_from      VPIN_NET_ADD only: the second operand
 *   VPIN_NET_ADD   vpin_enc_add over the 2 C planes per image in the blocked order (all c1 planes, then all c2 planes): the first
 *                  operand is the layer's input, the second the tensor skip_from names.  The shape goes through unchanged; no
 *                  keys, no bias r, 2 C H W additions per image; a round may follow as after any layer.  Adding the c1 halves and
 *                  the c2 halves adds the plaintexts.  The server keeps a referenced tensor, as host bytes, until its last use */
#define VPIN_NET_ADD 5
#define VPIN_NET_FROM_INPUT ((size_t)-1)
/*   (ABI 13) Max pooling inside the client's round, again at the END of vpin_net_layer and all zero for a round as before:
 *   round_pool_k, round_pool_stride  on a layer with has_round: the client pools the layer's C x H x W output by maximum over
 *                  k x k windows at that stride before it activates and encrypts again (vpin_e2_client_round_pool over planes =
 *                  B * C).  The callback is handed the usual cnt = B C H W ciphertexts, VPIN_LENET_MAXPOOL in flags and six outputs
 *                  of B C Ho Wo points, Ho = (H - k) / stride + 1, Wo likewise; vpin_net_round_pool gives it the shape.  The tensor
 *                  after the round is C x Ho x Wo, and every later shape follows from it: what input_from and skip_from name, an
 *                  ADD's comparison, an FC's K.  No layer call and no round of its own, and 1 / k^2 of the encryptions */
typedef struct vpin_net_layer {
  int kind;
  size_t fh, fw, pad;            /* CONV */
  size_t stride;                 /* CONV and POOL */
  const uint8_t* filter_le16;    /* CONV: fh x fw u128 weights, row-major, 16 bytes little-endian each */
  size_t k;                      /* POOL: the window */
  uint8_t scale_le16[16];        /* POOL: u128, the reference's 2^10 / k^2 */
  size_t K, N;                   /* FC */
  const int32_t* w;              /* FC: K x N, row-major, non-negative; FCS: signed */
  const int64_t* bias;           /* FC, FCS: N values; CONVMC: NULL or n_out values */
  int has_round, relu, shift_bits, reencrypt;
  uint64_t max_giant;
  size_t n_out;                  /* CONVMC (with fh, fw, pad, stride): the output channels */
  const int32_t* w_mc;           /* CONVMC: n_out x C x fh x fw, row-major, signed */
  const uint8_t* connect;        /* CONVMC: n_out x C bytes, non-zero = connected; NULL: all */
  const uint8_t* sum_table;      /* CONV: NULL, or sum_out x C bytes: the channel sums in front of the layer */
  size_t sum_out;
  size_t repeat;                 /* CONV: 0 or 1: once */
  int plane_order;               /* CONV and POOL: 0, or VPIN_NET_ORDER_INTERLEAVED */
  size_t input_from;             /* any kind: 0, 1 .. i, or VPIN_NET_FROM_INPUT: what the layer reads */
  size_t skip_from;              /* ADD: 1 .. i or VPIN_NET_FROM_INPUT: the second operand; the other kinds: 0 */
  size_t round_pool_k;           /* with has_round: 0, or the window of the max pooling inside the round */
  size_t round_pool_stride;      /* 0 exactly when round_pool_k is */
} vpin_net_layer;
typedef struct vpin_net_cfg {
  size_t C, H, W;                /* the encrypted input */
  int prf_bytes;                 /* per network (cnn_networks: 14) */
  size_t n_layers;
  const vpin_net_layer* layers;
} vpin_net_cfg;
/* what a run consumes; cap >= 8 + 3 n_layers values: out[0] layers, out[1] rounds, out[2] multiplications and out[3] additions
 * of the label, out[4] decryptions, out[5] client encryptions (the input included), out[6] PRF keys, out[7] bias r; then per
 * layer i out[8 + 3 i] its multiplications, out[9 + 3 i] its additions, out[10 + 3 i] the decryptions of the round after it (0:
 * none).  VPIN_EINVAL for a zero dimension, a window that does not fit, an FC whose K is not the incoming C * H * W, an unknown
 * kind, shift_bits outside 0 .. 62, reencrypt = 0 before the last layer, prf_bytes outside 1 .. 16, a CONVMC layer with n_out = 0
 * or a row of connect that selects no channel (the table is read here: the counts depend on it; the weights are not); (ABI 8) a
 * sum_table or a repeat > 1 on a layer that is no CONV, a sum_table with sum_out = 0 or with a row that selects no plane (read
 * here likewise), a plane_order that is neither 0 nor VPIN_NET_ORDER_INTERLEAVED.  A CONV behind sums and repeat counts 2 C'
 * planes, keys and C' planes out, C' = (sum_out, or the incoming C) * repeat.  (ABI 12) The walk follows input_from for the shape
 * that reaches each layer; VPIN_EINVAL, each with a text of its own, for a reference to the layer itself or a later one, a
 * skip_from on a kind other than ADD, an ADD without one, an ADD whose two operands are the same tensor (all doublings), an ADD
 * whose operands differ in C, H or W (the text gives both shapes), an ADD with a plane_order, a sum_table or a repeat.
 * (ABI 13) A round that pools: out[10 + 3 i] stays the C H W decryptions, out[5] counts its C Ho Wo encryptions, and the layers
 * behind it count over C x Ho x Wo; VPIN_EINVAL, each text naming the layer: a round_pool_k without has_round, one of round_pool_k
 * and round_pool_stride zero beside the other, a window that does not fit the layer's output */
int vpin_net_cfg_counts(const vpin_net_cfg* cfg, size_t* out, size_t cap);
/* (ABI 8) the reference's LeNet as a layer list: the seven layers vpin_lenet_infer runs (CONV with repeat = n1; POOL; CONV behind
 * the sums by cfg->connect; POOL; CONV behind the sum of all planes with repeat = n3; FC; FC), the convolutions and poolings
 * interleaved, every layer with its round R1 .. R7 (relu, shift_bits, max_giant, reencrypt = 0 on the last).  `layers` and `ones`
 * (n2 bytes, filled with 1: the table of the third convolution) are the caller's and *out borrows them and cfg's arrays; layer i is
 * label L(i + 1).  What vpin_lenet_infer computes on cfg, vpin_net_infer computes on *out byte for byte, with the same keys and
 * bias r; and so a batch, the wire and several clients take LeNet.  The codes and texts of vpin_lenet_infer for a bad cfg */
int vpin_lenet_as_net(const vpin_lenet_cfg* cfg, vpin_net_layer layers[7], uint8_t* ones, vpin_net_cfg* out);
typedef struct vpin_net_trace vpin_net_trace;
/* The server loop, the same driver as vpin_lenet_infer with one step per layer, the planes blocked (all c1, then all c2): the
 * same callback type per round (round = the round's number), the caller's keys (one per convolution plane and FC row, in call
 * order) and bias r (one per FC output, in layer order) with their counts checked against vpin_net_cfg_counts, baseG / baseH
 * because the server encrypts the bias (may be NULL without an FC layer; round_fn may be NULL without a round).  A failing
 * layer or round frees everything, returns its code and names itself in vpin_last_error(): "vpin_net_infer: layer 2 (fc): .." /
 * "vpin_net_infer: round 1: ..".  VPIN_EINVAL also for a negative weight and for a missing filter, weight or bias array */
int vpin_net_infer(vpin_ctx* ctx, const vpin_net_cfg* cfg, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                   const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH,
                   const uint8_t* keys32, size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn,
                   void* user, vpin_net_trace** out);
void vpin_net_trace_free(vpin_net_trace* t);
/* per layer: the trace of its layer call, borrowed until vpin_net_trace_free */
int vpin_net_trace_layers(const vpin_net_trace* t, size_t* n);
int vpin_net_trace_layer(const vpin_net_trace* t, size_t layer, const vpin_conv_trace** out);
/* as one label, borrowed: a trace whose two lists are those of all layers in layer order -- what the reference holds in its four
 * global lists at the end of inferenceCNN; its output and dims are the last layer's, it has no left sides */
int vpin_net_trace_label(const vpin_net_trace* t, const vpin_conv_trace** out);
/* the label through vpin_gadget_point_mult_dev / _add_dev: one pair of instances per network */
int vpin_net_trace_instances(vpin_ctx* ctx, const vpin_net_trace* t, vpin_dev_instance** mult_out, vpin_dev_instance** add_out);
/* the last layer's ciphertext: 2 x n points, the c1 half and then the c2 half */
int vpin_net_trace_result(const vpin_net_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf, size_t* n);
/* host-clock milliseconds of the last vpin_net_infer on this thread: out[0] the whole, out[1 + 2 i] layer i, out[2 + 2 i] the
 * round after it; slots past 1 + 2 n_layers read 0 */
int vpin_net_last_timings(double* out, size_t cap);
/* ---- a batch of B images through one inference (ABI 6) ---------------------------------------------------------------------
 * vpin_net_infer over B images at once; a batch is byte for byte B single inferences, everything image-major:
 *   c1, c2       B * C * H * W points each, [b][C][H][W]
 *   keys32       B * k keys, k = out[6] of vpin_net_cfg_counts; image b owns keys [b k, (b + 1) k) in the order a single run
 *                consumes them.  bias_r_le32: B * r values (out[7]) likewise: every image has its own bias encryption
 *   a layer      ONE call of its entry point over the planes [b][half][plane], half = c1, then c2: CONV and POOL with P = B * 2 C,
 *                CONVMC with groups = 2 B (g = 2 b + half), FC and FCS with P = 2 B rows (row 2 b: image b's c1 row); the biases
 *                of all images by one vpin_e2_encrypt of B * N values.  Every layer emits its lists plane by plane (row by row,
 *                group by group), so a layer's output, lists and left sides are those of the single runs, image after image
 *   a round      ONE callback with cnt = B * n, the values image-major; round, flags and shift_bits as in a single run.  The
 *                ready-made client consumes its queue of r in order: the input of all images, round 0 of all images, ..
 * B = 1 is vpin_net_infer: both are the same driver.  VPIN_EINVAL before anything runs: B = 0, B > VPIN_NET_MAX_BATCH, n_keys !=
 * B * k, n_bias_r != B * r, and a layer whose planes, groups or rows at this B are more than its kernels' grids take (65535:
 * "vpin_net_infer_batch: layer 2 (convmc): 2 B * C = 73728 planes are more than the 65535 a layer call takes").  A failing layer
 * or round fails the whole batch with the single run's texts; an index in such a text counts over the whole batch: image = index /
 * the per-image count.  A layer says that an input point is not on the curve, not which one; when the first layer refuses the
 * caller's input so, a batch's text goes on with the first such point as vpin_e2_pack names it (found by packing the input, on
 * this path only): ".. a pixel is not on the curve E2; the input's c1: vpin_e2_pack: point 250: the point is not on the curve E2".
 * On a batch's trace the accessors above keep their meaning over the whole batch: vpin_net_trace_layer is the one layer call (P
 * = B x the single P), vpin_net_trace_label holds the images' labels one after the other in image order (its output and dims are
 * the last layer call's), vpin_net_trace_instances builds from that label, vpin_net_trace_result gives B x (2 x n) points
 * image-major with *n = n. */
#define VPIN_NET_MAX_BATCH 1024
int vpin_net_infer_batch(vpin_ctx* ctx, const vpin_net_cfg* cfg, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                         const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH,
                         const uint8_t* keys32, size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn,
                         void* user, vpin_net_trace** out);
/* (ABI 7) vpin_net_infer_batch over the images of several clients, each under its own key: n_pub public keys (hx, hy: canonical
 * little-endian, n_pub x 32 bytes each) and per image the index of its client's, key_of_image[B].  No table of any H: the biases
 * of all images are still ONE encryption, vpin_e2_encrypt_keyed with image b's values under key key_of_image[b].  Everything else
 * is vpin_net_infer_batch: layers, keys, bias r, the trace and all its accessors.  The round callback sees the whole batch,
 * image-major; who decrypts which images is the caller's business.  With n_pub = 1 the run is byte for byte vpin_net_infer_batch
 * under a table of that key.  VPIN_EINVAL in addition: hx, hy or key_of_image NULL, n_pub = 0, a key_of_image[b] >= n_pub (b is
 * named), and, from the first layer with a bias, a public key that vpin_e2_encrypt_keyed refuses */
int vpin_net_infer_multi(vpin_ctx* ctx, const vpin_net_cfg* cfg, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                         const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const uint8_t* hx,
                         const uint8_t* hy, size_t n_pub, const uint32_t* key_of_image, const uint8_t* keys32, size_t n_keys,
                         const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user, vpin_net_trace** out);
/* the images of a trace (1 for vpin_net_infer's) */
int vpin_net_trace_images(const vpin_net_trace* t, size_t* B);
/* image b's label, borrowed until vpin_net_trace_free: byte for byte what vpin_net_trace_label gives for image b run alone
 * (lists, output, dims).  Built when first asked for and kept; one thread reads a trace at a time */
int vpin_net_trace_image_label(const vpin_net_trace* t, size_t b, const vpin_conv_trace** out);
/* (ABI 8) image b's share of ONE layer call, borrowed likewise: its lists, its left sides and its output, byte for byte
 * vpin_net_trace_layer of that image run alone.  For a network whose layers are labels of their own (LeNet: seven) */
int vpin_net_trace_image_layer(const vpin_net_trace* t, size_t b, size_t layer, const vpin_conv_trace** out);
/* image b's label as vpin_net_trace_instances */
int vpin_net_trace_image_instances(vpin_ctx* ctx, const vpin_net_trace* t, size_t b, vpin_dev_instance** mult_out,
                                   vpin_dev_instance** add_out);
/* ---- images that leave a running batch (ABI 9) --------------------------------------------------------------------------------
 * vpin_net_infer_isolated is vpin_net_infer_multi plus status[B]: an image that makes a layer refuse leaves the batch and the
 * others go on.  An image is named by its SLOT b of the batch handed in, for its whole life: keys32, bias_r_le32 and key_of_image
 * stay indexed by slot, so a survivor's bytes depend only on its slot, never on who else is or was in the batch.
 *   a refusal   a layer call that answers VPIN_ESHAPE with units in vpin_enc_last_refusals: the units are mapped to images (plane
 *               / the planes one image hands to the call: 2 C * repeat for CONV behind its sums and repeat, 2 C for POOL; group /
 *               2; row / 2), status[b] = {VPIN_ESHAPE, layer, -1, the text the batch would have failed with}, the images are
 *               removed from the step's input and the call runs again over the survivors, the biases encrypted again with the
 *               same r.  Every repeat removes an image, so a step runs at most B times.  The list names the units of the stage
 *               that refused: an image that breaks a later rule is found by the repeat
 *   a bad point an input or reply point that a layer's load refuses (VPIN_EINVAL, "a coordinate is not below q", ".. is not on
 *               the curve E2"): the images that own such a point are found with vpin_e2_pack per image and leave the same way
 *               with the code VPIN_EINVAL
 *   a drop      inside the round callback (and only there, on its thread) vpin_net_round_images gives the slots of the cnt =
 *               n * per values at hand, position after position, and vpin_net_round_drop_images takes images out of the batch
 *               after the round: status[b] = {code, layer, round, text}, what the callback wrote for them is ignored.
 *               VPIN_EINVAL for a slot that is not at hand, a slot named twice, code = VPIN_OK, a run that is not isolated
 *               (vpin_net_round_images answers in every run of the vpin_net_infer family)
 *   the end     status[b].code = VPIN_OK for the survivors.  Nobody left: VPIN_ESHAPE, "vpin_net_infer_isolated: no image is
 *               left", *out = NULL, every status written
 * NOT isolated, the batch fails as vpin_net_infer_multi's: VPIN_EVERIFY, VPIN_EHIP, VPIN_ENOMEM, a failing round callback, a
 * VPIN_ESHAPE whose list is empty and a VPIN_EINVAL that no image's point explains (the server's keys, weights or bias).
 * The trace: vpin_net_trace_images stays B; vpin_net_trace_layer is the call that succeeded, with P of the images in it, which
 * vpin_net_trace_layer_images names (slots ascending, borrowed); vpin_net_trace_image_layer, _image_label and _image_instances
 * keep taking the slot b and answer VPIN_ESHAPE, "..: image b left the batch at layer L", for an image that is not in that layer
 * (the label: that did not stay to the end; ".. at the last round" for one the last round dropped, which every layer still
 * holds); vpin_net_trace_label, _instances and _result hold the survivors in slot order.
 * With no refusal and no drop the run and the trace are byte for byte vpin_net_infer_multi's. */
typedef struct vpin_net_image_status {
  int code;   /* VPIN_OK: the image stayed to the end */
  int layer;  /* the layer whose call refused it, or whose round dropped it */
  int round;  /* -1: a layer's refusal */
  char text[256];
} vpin_net_image_status;
int vpin_net_infer_isolated(vpin_ctx* ctx, const vpin_net_cfg* cfg, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                            const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const uint8_t* hx,
                            const uint8_t* hy, size_t n_pub, const uint32_t* key_of_image, const uint8_t* keys32, size_t n_keys,
                            const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user,
                            vpin_net_image_status* status, vpin_net_trace** out);
int vpin_net_round_images(const uint32_t** slots, size_t* n);
/* (ABI 13) inside the round callback, on its thread, like vpin_net_round_images: out = {planes = the live images * C, H, W, k,
 * stride} of the round at hand; k = 0 (and stride = 0): the round does not pool.  A callback handed VPIN_LENET_MAXPOOL writes
 * planes * Ho * Wo points.  An image dropped in such a round leaves the batch at its pooled per-image size.  VPIN_EINVAL outside
 * a callback */
int vpin_net_round_pool(size_t out[5]);
int vpin_net_round_drop_images(const uint32_t* slots, size_t n, int code, const char* text);
int vpin_net_trace_layer_images(const vpin_net_trace* t, size_t layer, const uint32_t** slots, size_t* n);
/* what the last vpin_net_infer_isolated on this thread did: images a layer refused, images dropped in a round, layer calls repeated */
void vpin_net_last_isolation(uint64_t out[3]);
/* The ready-made client of both drivers, for n_rounds rounds (LeNet: 7): owns sk, the tables of G and H = sk * G, a
 * discrete-log table of nb baby steps, one range max_giant per round and the queue of n_r encryption randomness values (32 bytes
 * each, one per encrypt call in order).  vpin_net_client_round is a vpin_lenet_round_fn over vpin_e2_client_round with user =
 * the client; it keeps each round's raw decryptions and activated values (vpin_net_client_values, round 0 .. n_rounds - 1,
 * borrowed).  VPIN_EINVAL when the queue of r runs out; a round that fails consumes no randomness, so the client can be used
 * again */
typedef struct vpin_net_client vpin_net_client;
int vpin_net_client_create(vpin_ctx* ctx, const uint8_t sk_le32[32], uint64_t nb, size_t n_rounds, const uint64_t* max_giant,
                           const uint8_t* r_le32, size_t n_r, vpin_net_client** out);
void vpin_net_client_free(vpin_net_client* cl);
int vpin_net_client_bases(const vpin_net_client* cl, const vpin_e2_base** baseG, const vpin_e2_base** baseH);
int vpin_net_client_values(const vpin_net_client* cl, size_t round, const int64_t** v, const int64_t** act, size_t* cnt);
int vpin_net_client_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                          const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* c1ox, uint8_t* c1oy,
                          uint8_t* c1oinf, uint8_t* c2ox, uint8_t* c2oy, uint8_t* c2oinf);
/* (ABI 13) The client's pooling schedule.  Like the rest of the schedule it is the CLIENT's: a client does not pool, or leave it,
 * because a server says so.  vpin_net_client_set_pools gives the client its own per-round {H, W, k, stride} (n_rounds: the rounds
 * it was made for; all zero: the round does not pool, which is what a new client holds for every round).  vpin_net_client_round
 * then answers VPIN_ESHAPE, with a text that gives both sides, before anything is decrypted (vpin_net_client_values is empty for
 * that round and no r is consumed) when the VPIN_LENET_MAXPOOL bit of flags disagrees with its schedule for the round, or cnt is no
 * multiple of H * W; otherwise it calls vpin_e2_client_round_pool with planes = cnt / (H W) and consumes cnt_out values of r.
 * vpin_net_client_values keeps returning v and act with cnt = |v|; vpin_net_client_act_count gives |act|, the pooled count.
 * On the wire the ROUND frame is as it was, flags carrying bit 4, which vpin_net_client_run compares with its schedule like every
 * other flag; the REPLY to a round that pools carries cnt_out points, and vpin_wire_round, which learns cnt_out from
 * vpin_net_round_pool, rejects any other count.  vpin_net_server_create answers VPIN_EINVAL for a configuration with such a round:
 * the multi-client server copies a dropped client's images from a round's input to its output at one per-image size */
typedef struct vpin_net_round_pool_spec {
  size_t H, W, k, stride;
} vpin_net_round_pool_spec;
int vpin_net_client_set_pools(vpin_net_client* cl, const vpin_net_round_pool_spec* pools, size_t n_rounds);
int vpin_net_client_act_count(const vpin_net_client* cl, size_t round, size_t* n);

/* ---- the inference between two processes over a byte stream (ABI 5) ----------------------------------------------------------
 * The reference's Server.py / Client.py are two processes (send_data_in_chunks / receive_data_in_chunks); here the server loop
 * (vpin_net_serve) and the client (vpin_net_client_run) meet over any byte stream the caller has: vpin_wire_round is the round
 * callback of vpin_net_infer on the server's side, vpin_net_client_round is called in a loop on the client's.  The library opens,
 * listens on and connects nothing; there is no authentication.  The frames carry no proofs: those follow DONE
 * on the same stream as records of their own (ABI 10, below: vpin_net_send_proofs, vpin_net_client_verify).
 *
 * A packed point is one 256-bit little-endian integer (E2's group order is prime and the only multiple of itself inside the Hasse
 * interval: every point of the curve is in the group, so x and a sign say it all):
 *   bits 0 .. 252  the canonical x, x < q        bit 254  the identity; all other bits are zero then
 *   bit 253        zero                          bit 255  bit 0 of the canonical y in [0, q)
 * The point (0, sqrt(b)) with even y is 32 zero bytes, a valid point; the identity is 00 .. 00 40.
 * vpin_e2_pack: points as in vpin_e2_msm -> cnt x 32 bytes.  VPIN_EINVAL: a null argument, cnt = 0 or >= 2^31, and, named with the
 * first such index ("vpin_e2_pack: point 3: the point is not on the curve E2"), a coordinate >= q or a point off the curve.
 * vpin_e2_unpack: cnt x 32 bytes -> points as every layer takes them (an identity as zeros with flag 1).  One square root in
 * F_q per point on the device (one fixed exponentiation; the root is checked, never trusted).  VPIN_EINVAL: a null argument,
 * cnt = 0 or >= 2^31, and, named with the first such index and its rule: "x is not below q" (x is never reduced: x = q is not
 * x = 0), "bit 253 is set", "the identity bit is set together with other bits", "x is not on the curve E2" (x^3 + a x + b is
 * not a square), "the parity bit is set over y = 0". */
int vpin_e2_pack(vpin_ctx* ctx, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt, uint8_t* out32);
int vpin_e2_unpack(vpin_ctx* ctx, const uint8_t* in32, size_t cnt, uint8_t* px, uint8_t* py, uint8_t* pinf);

/* A frame is a header of 24 bytes, little-endian, and a payload:
 *   magic "VPW1" | type u8 | flags u8 | shift_bits u8 | reserved u8 = 0 | round u32 | cnt u32 | payload_len u64
 *   HELLO  client -> server  cnt = 1           the packed public key H
 *   INPUT  client -> server  cnt = C H W       cnt packed c1, then cnt packed c2
 *   ROUND  server -> client  the round's cnt   as INPUT, with round, flags (VPIN_LENET_RELU | VPIN_LENET_REENCRYPT), shift_bits
 *   REPLY  client -> server  cnt, or 0         as INPUT; cnt = 0 without a payload acknowledges a round that encrypts nothing
 *   DONE   server -> client  cnt = 0           no payload
 *   ERROR  either way        cnt = 0           an int32 code and at most VPIN_WIRE_MAX_TEXT bytes of text
 * vpin_wire_header_decode answers VPIN_EINVAL and names the rule for a wrong magic, an unknown type, a reserved byte that is
 * not zero, cnt above VPIN_WIRE_MAX_CNT and a payload_len that is not exactly what the type and cnt imply; the cap bounds what
 * a hostile header can make a receiver allocate, and no receiver allocates before decode has accepted the header.
 * vpin_wire_header_encode applies the same rules to what it is given. */
#define VPIN_WIRE_HELLO 1
#define VPIN_WIRE_INPUT 2
#define VPIN_WIRE_ROUND 3
#define VPIN_WIRE_REPLY 4
#define VPIN_WIRE_DONE 5
#define VPIN_WIRE_ERROR 6
#define VPIN_WIRE_HEADER_LEN 24
#define VPIN_WIRE_MAX_CNT ((uint32_t)1 << 24)
#define VPIN_WIRE_MAX_TEXT 1024
typedef struct vpin_wire_header {
  uint8_t type, flags, shift_bits;
  uint32_t round, cnt;
  uint64_t payload_len;
} vpin_wire_header;
int vpin_wire_header_encode(const vpin_wire_header* h, uint8_t out24[VPIN_WIRE_HEADER_LEN]);
int vpin_wire_header_decode(const uint8_t in24[VPIN_WIRE_HEADER_LEN], vpin_wire_header* h);

/* The stream: frames over a transport of the caller's.  send / recv move exactly n bytes and return 0, or fail with a negative
 * code.  The descriptor form serves pipes, socketpairs and connected sockets and closes nothing: every wait is a poll of at most
 * timeout_ms (> 0), EINTR is retried, and end-of-file, a time-out and a write error are VPIN_ECOMM with a text such as
 * "vpin_wire: the peer closed the stream after 17 of 24 bytes"; a closed peer is never SIGPIPE (MSG_NOSIGNAL on sockets, the
 * signal masked around the write elsewhere).  A vpin_wire needs no context and no GPU; one thread drives it.
 * vpin_wire_send / vpin_wire_recv move one frame: recv decodes the header first and answers VPIN_EINVAL, reading no payload,
 * when payload_len is above cap.  vpin_wire_send_error sends ERROR(code, text) best effort and keeps the caller's error text.
 * vpin_wire_stats: bytes sent, bytes received, frames sent, frames received.  vpin_wire_timings: host-clock ms of slot 0 (HELLO
 * and INPUT) or 1 + r (round r) spent by this side in pack, unpack, send and the receive of payloads; VPIN_EINVAL for a slot
 * this wire has not seen. */
typedef struct vpin_wire vpin_wire;
typedef struct vpin_wire_io {
  int (*send)(void* user, const void* p, size_t n);
  int (*recv)(void* user, void* p, size_t n);
  void* user;
} vpin_wire_io;
int vpin_wire_create(const vpin_wire_io* io, vpin_wire** out);
int vpin_wire_fd_create(int rfd, int wfd, int timeout_ms, vpin_wire** out);
void vpin_wire_free(vpin_wire* w);
int vpin_wire_stats(const vpin_wire* w, uint64_t out[4]);
int vpin_wire_timings(const vpin_wire* w, size_t slot, double out[4]);
int vpin_wire_send(vpin_wire* w, const vpin_wire_header* h, const uint8_t* payload);
int vpin_wire_recv(vpin_wire* w, vpin_wire_header* h, uint8_t* payload, size_t cap);
int vpin_wire_send_error(vpin_wire* w, int code, const char* text);

/* The server's endpoint.  vpin_wire_round is a vpin_lenet_round_fn with user = a vpin_wire bound to a context
 * (vpin_wire_bind_ctx; vpin_net_serve binds its own): it packs the round's c1 and c2, sends ROUND, reads REPLY, checks its round
 * and cnt (VPIN_ESHAPE, "vpin_wire_round: round 2: the reply is for round 3"), unpacks (VPIN_EINVAL naming the index, as
 * vpin_e2_unpack) and returns the points in the callback's outputs.  An ERROR frame from the peer is VPIN_ECOMM quoting the
 * peer's code and text.  vpin_lenet_infer takes it as well.
 * vpin_net_serve reads HELLO, unpacks H and builds the tables of G and H, reads INPUT (cnt must be the configuration's C H W:
 * VPIN_ESHAPE), runs vpin_net_infer with vpin_wire_round and sends DONE.  On any failure of its own it sends ERROR(code, text)
 * best effort, frees everything and returns the code with the text; the server never holds a secret key.  VPIN_EINVAL before
 * anything is read for a configuration whose last layer has no round: its result would never reach the client. */
int vpin_wire_bind_ctx(vpin_wire* w, vpin_ctx* ctx);
int vpin_wire_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                    const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* c1ox, uint8_t* c1oy, uint8_t* c1oinf,
                    uint8_t* c2ox, uint8_t* c2oy, uint8_t* c2oinf);
int vpin_net_serve(vpin_ctx* ctx, const vpin_net_cfg* cfg, vpin_wire* w, const uint8_t* keys32, size_t n_keys,
                   const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_trace** out);
/* (ABI 6) vpin_net_serve for a batch of up to max_batch images, run by vpin_net_infer_batch: n_keys = max_batch * k and n_bias_r =
 * max_batch * r (VPIN_EINVAL otherwise, and for max_batch outside 1 .. VPIN_NET_MAX_BATCH, before anything is read).  The server
 * reads B off the INPUT frame, B = cnt / (C H W); a cnt that is no multiple of C H W or a B outside 1 .. max_batch is VPIN_ESHAPE
 * with an ERROR frame to the peer, as for vpin_net_serve's wrong count.  The first B * k keys and B * r values are used.  No
 * frame changes: INPUT and every ROUND and REPLY carry B times the single run's cnt, image-major.  vpin_net_serve itself is as it
 * was: one image, its own texts.  The client's side needs nothing new: vpin_net_client_run takes n_input and the schedule's cnt
 * from its caller */
int vpin_net_serve_batch(vpin_ctx* ctx, const vpin_net_cfg* cfg, vpin_wire* w, size_t max_batch, const uint8_t* keys32, size_t n_keys,
                         const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_trace** out);

/* ---- several clients in one batched inference (ABI 7) -------------------------------------------------------------------------
 * A service has many clients with an image or two each, every one with its own key.  vpin_net_serve_multi runs ONE inference
 * (vpin_net_infer_multi) over the images of all the wires it is given, every round one exchange with all of them, and drops a
 * client that disappears or misbehaves on the wire while the others finish.  No frame changes and the client's side needs nothing
 * new (vpin_net_client_run): each wire sees exactly the frames vpin_net_serve_batch would send it alone.
 * A vpin_net_server holds what outlives a call: the checked configuration (borrowed: it and what it points to live until
 * vpin_net_server_free) and the table of G, built ONCE; no table of any client's H is ever built (vpin_e2_encrypt_keyed).
 * vpin_net_server_create: VPIN_EINVAL as vpin_net_serve_batch for the configuration and max_batch.  vpin_net_server_stats:
 * out = {calls, clients admitted, clients served to DONE, images run, base tables built}.  One thread drives a server.
 *
 * vpin_net_serve_multi, n_keys = max_batch * k and n_bias_r = max_batch * r as for vpin_net_serve_batch:
 *   admission   in wire order: HELLO, then INPUT, B_i = cnt / (C H W).  A wire is answered with ERROR where it can be and is not
 *               admitted when HELLO or INPUT is another type, its key is the identity or does not unpack, its cnt is 0 or no
 *               multiple of C H W, its B_i does not fit into what is left of max_batch (what the wires before it asked for,
 *               whether or not their points then unpack), or one of its input points does not unpack.  The keys and inputs of
 *               all wires are unpacked by ONE launch.  Admitted clients take image slots in wire order: first_image = the sum of
 *               B_j over the clients admitted before; slot s uses the keys [s k, (s + 1) k) and the bias r [s r, (s + 1) r), so
 *               which keys a client is served with depends only on who was admitted before it.  Nobody admitted: VPIN_ESHAPE,
 *               "vpin_net_serve_multi: no client was admitted", *out = NULL, nothing runs
 *   a round     one pack launch over the batch's c1 | c2; every live client gets ROUND with cnt = B_i * n and its slice, c1 part
 *               then c2 part; all ROUNDs are sent first, then the REPLYs are read in wire order (the clients decrypt at the same
 *               time); one unpack launch over all replies
 *   a drop      a client whose stream fails or times out, who sends ERROR, a REPLY for another round or with another cnt, or a
 *               REPLY with a point that does not unpack is dropped from that round on: ERROR to it best effort and nothing more (a
 *               silent client costs its wire's timeout_ms once).  Its images stay in the batch: for that round and every later
 *               one their reply is the ciphertexts the server sent, so the layer calls keep their shape and the other images are
 *               untouched; its part of the trace means nothing.  The last live client gone: VPIN_ECOMM, *out = NULL
 *   the end     DONE to every live client.  VPIN_OK when at least one client got DONE
 *   the server's own failure (a layer's refusal, VPIN_EHIP, VPIN_ENOMEM): ERROR to every live client, the code into their
 *               status, and returned
 * status[i], for wire i: code VPIN_OK and stage VPIN_NET_STAGE_DONE for a client served to DONE; otherwise the code, the text and
 * the stage it left at: VPIN_NET_STAGE_ADMISSION, the round's number, or VPIN_NET_STAGE_SERVER for the server's own failure.
 * first_image and n_images are its slots (0, 0 when it was not admitted).
 * Isolation (ABI 9, vpin_net_server_set_isolation; off by default, and off is everything above, byte for byte): a client whose
 * well-formed ciphertexts drive a layer into a refusal (an identity point the wire format allows, an accumulator that is the
 * identity, an s_k that does not fit) fails the whole batch when it is off.  When it is on the call runs vpin_net_infer_isolated:
 *   a refusal   the image leaves the batch inside the driver and the layer runs again over the others.  The schedule of
 *               vpin_net_client_run fixes cnt = B_i * n per round, so on the wire the unit that leaves is the CLIENT: at the next
 *               round a client that lost an image is dropped with all its images, gets ERROR with the layer's text, and its
 *               status holds the layer's code and text and the stage VPIN_NET_STAGE_LAYER
 *   a drop      a client dropped in a round leaves the batch at that round (vpin_net_round_drop_images): the later layer calls
 *               run over the images of the others alone, and vpin_net_trace_layer_images names them
 *   positions   a client keeps its slots [first_image, first_image + n_images) for its status, its keys and its bias r; where its
 *               images stand in the batch at hand is worked out again before every round.  A surviving client sees exactly the
 *               frames it would see alone in its slots
 *   nobody left VPIN_ECOMM, *out = NULL, every status written
 * vpin_net_server_stats_isolation: out = {images of clients a layer refused, images compacted away after a drop on the wire,
 * layer calls repeated}, summed over the server's calls.  Still NOT isolated: VPIN_EVERIFY, VPIN_EHIP, VPIN_ENOMEM, and a refusal
 * that is the server's own keys' doing (a folded weight that does not fit under a slot's key hits that slot whoever sits in it;
 * one that no image explains fails the batch).
 * VPIN_EINVAL before anything is read: a null argument, n_wires = 0 or > max_batch, the same wire twice, n_keys != max_batch * k,
 * n_bias_r != max_batch * r.  All waits are the wires' own timeout_ms; admission reads the wires one after another. */
typedef struct vpin_net_server vpin_net_server;
int vpin_net_server_create(vpin_ctx* ctx, const vpin_net_cfg* cfg, size_t max_batch, vpin_net_server** out);
void vpin_net_server_free(vpin_net_server* s);
int vpin_net_server_stats(const vpin_net_server* s, uint64_t out[5]);
int vpin_net_server_set_isolation(vpin_net_server* s, int on);
int vpin_net_server_stats_isolation(const vpin_net_server* s, uint64_t out[3]);
#define VPIN_NET_STAGE_DONE (-1)
#define VPIN_NET_STAGE_ADMISSION (-2)
#define VPIN_NET_STAGE_SERVER (-3)
#define VPIN_NET_STAGE_LAYER (-4) /* isolation: a layer refused one of the client's images */
typedef struct vpin_net_peer_status {
  int code;
  int stage;
  uint32_t first_image, n_images;
  char text[256];
} vpin_net_peer_status;
int vpin_net_serve_multi(vpin_net_server* s, vpin_wire* const* wires, size_t n_wires, const uint8_t* keys32, size_t n_keys,
                         const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_peer_status* status, vpin_net_trace** out);

/* The client's endpoint: encrypts the image (n_input ints under n_input r, as vpin_e2_encrypt) under its own tables, sends HELLO
 * and INPUT, then serves frames.  A client that performs whatever round the server asks for is a decryption oracle, so the
 * schedule is the CLIENT's: ROUND must carry the next round number and exactly that round's flags, shift_bits and cnt, else the
 * client sends ERROR and returns VPIN_ESHAPE ("vpin_net_client_run: round 2: the server asks for shift_bits 20, the schedule
 * says 21") before anything is decrypted.  On a match: unpack, vpin_net_client_round, pack, REPLY.  DONE is VPIN_OK only after
 * all n_rounds rounds (VPIN_ESHAPE otherwise); ERROR is VPIN_ECOMM with the peer's text.  n_rounds is at most the rounds the
 * client was created for.  The values are read with vpin_net_client_values. */
typedef struct vpin_wire_round_spec {
  int flags;
  int shift_bits;
  size_t cnt;
} vpin_wire_round_spec;
int vpin_net_client_run(vpin_net_client* cl, vpin_wire* w, const int64_t* image, const uint8_t* image_r_le32, size_t n_input,
                        const vpin_wire_round_spec* schedule, size_t n_rounds);

/* ---- proofs over the wire (ABI 10) ----------------------------------------------------------------------------------------------
 * After DONE the stream is still open (the library closes nothing), and the server can send each client the proofs of its own
 * images: the reference's my_lib_verify on two proofs per label, one saying that the server knows a witness of n_mult point
 * multiplications that satisfies the gadget, one saying the same for n_add point additions, each under the Hyrax commitments
 * comm_para and comm_input it sends.
 * What acceptance means, and what it does not: as in the reference, vars_input holds the server's intermediate values, and
 * NOTHING ties the committed points to this session's ciphertexts.  An accepted record says "a satisfying witness of that many
 * operations exists and the server knows it", not "it is the witness of my inference".  No binding is invented here.
 * The R1CS itself is not left to the server: the instances' A, B, C depend only on the kind and the number of operations
 * (point_mult.rs:61-325 and point_addition.rs:67-153 build inst_1 before any witness value is used, and SNARK::encode takes no
 * randomness), so the client DERIVES the computation commitment and the public inputs from (is_mult, n_ops) on its own GPU and
 * compares the server's comm with its own byte for byte.  There is no mode that takes comm from the server: such a client would
 * accept a proof of a trivial instance.
 *
 * Proofs are no VPW1 frames.  A record has a header of 40 bytes, little-endian, and a payload:
 *   magic "VPP1" | kind u8 | is_mult u8 | reserved u16 = 0 | image u32 | label u32 | n_ops u64 | proof_len u64 | comm_len u64
 *   PROOF  image: the index among the client's own images, in image order; label: 0 for the image's one label, 1 + layer for a
 *          per-layer label; payload proof | comm | comm_para | comm_input, the last two of vpin_gadget_vars_rows(is_mult, n_ops)
 *          rows of 32 bytes each (the rule of vpin_snark_verify_batch); proof_len is at most vpin_gadget_proof_max_bytes and
 *          comm_len exactly vpin_gadget_comm_bytes of the shape
 *   END    image: the number of PROOF records sent; every other field zero; no payload
 *   ERROR  proof_len: the payload's length; the payload an int32 code and at most VPIN_WIRE_MAX_TEXT bytes of text; every other
 *          field zero
 * vpin_proof_header_encode and vpin_proof_header_decode apply the same rules and answer VPIN_EINVAL naming the one broken: a wrong
 * magic, an unknown kind, reserved bytes that are not zero, is_mult > 1, n_ops = 0 or above VPIN_PROOF_MAX_OPS, proof_len above
 * what the shape allows, comm_len other than the shape's, and for END and ERROR a field that must be zero and is not (ERROR: a
 * proof_len outside 4 .. 4 + VPIN_WIRE_MAX_TEXT).  No receiver allocates before decode has accepted the header, and what it then
 * allocates is bounded by the shape.  vpin_proof_payload_len: the payload's bytes under an accepted header.
 * vpin_proof_send / vpin_proof_recv move one record over a vpin_wire and count into its stats as frames; recv decodes the header
 * first and answers VPIN_EINVAL, reading no payload, when the payload is longer than cap. */
#define VPIN_PROOF_RECORD 1
#define VPIN_PROOF_END 2
#define VPIN_PROOF_ERROR 3
#define VPIN_PROOF_HEADER_LEN 40
#define VPIN_PROOF_MAX_OPS ((uint64_t)1 << 24)
typedef struct vpin_proof_header {
  uint8_t kind, is_mult;
  uint32_t image, label;
  uint64_t n_ops, proof_len, comm_len;
} vpin_proof_header;
int vpin_proof_header_encode(const vpin_proof_header* h, uint8_t out40[VPIN_PROOF_HEADER_LEN]);
int vpin_proof_header_decode(const uint8_t in40[VPIN_PROOF_HEADER_LEN], vpin_proof_header* h);
uint64_t vpin_proof_payload_len(const vpin_proof_header* h);
int vpin_proof_send(vpin_wire* w, const vpin_proof_header* h, const uint8_t* payload);
int vpin_proof_recv(vpin_wire* w, vpin_proof_header* h, uint8_t* payload, size_t cap);

/* The server's side.  vpin_net_send_proofs walks the images [first_image, first_image + n_images) of a trace in image order.
 * per_layer = 0: the image's label (the lists of vpin_net_trace_image_label, as vpin_net_trace_image_instances takes them);
 * per_layer = 1: every layer of vpin_net_trace_image_layer in layer order (as vpin_conv_trace_instances), label 1 + layer.  The
 * multiplication instance comes before the addition instance; one that does not exist (a pooling label, a 1 x 1 filter) is
 * skipped.  Per instance: build it, vpin_dev_instance_is_sat (a 0 answers VPIN_EVERIFY, sends an ERROR record, and nothing more
 * is sent), vpin_snark_prove_dev, one PROOF record, free -- the next instance is built after that, so an image never holds two
 * instances at once.  At the end END.  A failure of its own goes to the peer as an ERROR record, best effort.
 * Seeds: the 128 bytes SHAKE256(master_seed64 | "vPIN/wire-proof" | le32(slot) | le32(label) | u8(is_mult)), slot = first_image +
 * image; the first 64 are seed_commit, the last 64 seed_proof.  master_seed64 = NULL: 64 bytes from the operating system.
 * ms_out (may be NULL): host-clock ms of instance build (with is_sat), prove and send. */
int vpin_net_send_proofs(vpin_ctx* ctx, const vpin_net_trace* t, size_t first_image, size_t n_images, vpin_wire* w, int per_layer,
                         const uint8_t master_seed64[64], double ms_out[3]);
/* After vpin_net_serve_multi, with the status it wrote: every wire with code VPIN_OK and stage VPIN_NET_STAGE_DONE gets the proofs
 * of its slots [first_image, first_image + n_images), with isolation on too.  A wire that fails here is reported with its code and
 * text at the stage VPIN_NET_STAGE_PROOFS; the others still get theirs.  VPIN_OK when at least one client received END;
 * VPIN_ESHAPE when no wire was served to DONE, otherwise the last failing wire's code. */
#define VPIN_NET_STAGE_PROOFS (-5)
int vpin_net_server_send_proofs(vpin_net_server* s, const vpin_net_trace* t, vpin_wire* const* wires, size_t n_wires,
                                vpin_net_peer_status* status, int per_layer, const uint8_t master_seed64[64]);

/* The client's side.  A vpin_net_verifier owns, per (is_mult, n_ops), the derived comm bytes and inputs.  vpin_net_verifier_shape
 * derives a shape when first asked: the device gadget over n_ops placeholder operations (points as vpin_synthetic_points makes
 * them, odd weights; for additions operands whose sum is neither a doubling nor the identity), vpin_spark_encode_dev, the
 * commitment and vpin_dev_instance_inputs kept (borrowed until vpin_net_verifier_free), the instance and the decommitment freed.
 * A second request is a lookup: a returning client, or one with many images, derives each shape once.
 * vpin_net_verifier_stats: out = {shapes derived, lookups, proofs accepted, proofs rejected}.  vpin_net_verifier_timings: host-clock
 * ms of the last vpin_net_client_verify: receiving, deriving shapes and comparing commitments, the batch verification.
 * vpin_net_client_verify reads the records behind DONE.  The expectation list is the CLIENT's, as the round schedule is and for the
 * same reason: the same for every image, in the order the server sends, filled from vpin_net_cfg_counts on a configuration of the
 * same architecture.  Each record must be the next expected (image, label, is_mult, n_ops); otherwise the client sends an ERROR
 * record and returns VPIN_ESHAPE naming both sides ("vpin_net_client_verify: image 1, label 0: the server proves 131
 * multiplications, the expectation says 130") before the payload is read or anything is allocated for that record.  After the last
 * record END must follow with the right count.  A peer's ERROR is VPIN_ECOMM quoting it.
 * A record whose comm is not the derived one is rejected without verification (ok_out 0, "not the shape's commitment"); all the
 * others go through ONE vpin_snark_verify_batch with the derived comm and inputs (seed32 as there, may be NULL).  ok_out holds
 * n_images * n_expect verdicts, image-major.  VPIN_OK when every one is 1, VPIN_EVERIFY otherwise. */
typedef struct vpin_net_verifier vpin_net_verifier;
int vpin_net_verifier_create(vpin_ctx* ctx, vpin_net_verifier** out);
void vpin_net_verifier_free(vpin_net_verifier* v);
int vpin_net_verifier_shape(vpin_net_verifier* v, int is_mult, size_t n_ops, const uint8_t** comm, size_t* comm_len,
                            const uint8_t** inputs, size_t* num_inputs);
int vpin_net_verifier_stats(const vpin_net_verifier* v, uint64_t out[4]);
int vpin_net_verifier_timings(const vpin_net_verifier* v, double out[3]);
typedef struct vpin_proof_expect {
  uint32_t label;
  uint8_t is_mult;
  uint64_t n_ops;
} vpin_proof_expect;
int vpin_net_client_verify(vpin_net_verifier* v, vpin_wire* w, size_t n_images, const vpin_proof_expect* expect, size_t n_expect,
                           const uint8_t seed32[32], uint8_t* ok_out /* n_images * n_expect */);

/* BulletReductionProof::prove, Spartan/src/nizk/bullet.rs:32-132, with the round challenges GIVEN (u_mont: log2(R)
 * Montgomery scalars) instead of drawn from a transcript, over the R stream generators of `g` only (the caller's
 * c*Q and blind*H terms are host work: nizk/mod.rs:447-531).  x = the vector being reduced (a in bullet.rs), a = the
 * public vector (b in bullet.rs), R scalars each.  Per round k: cLR_out[64k..] = <a_L,b_R> | <a_R,b_L>,
 * LR_out[64k..] = compressed <a_L,G_R> | <a_R,G_L>; at the end x_hat | a_hat and the compressed g_hat.  The device never
 * folds G (bullet.hip); classic != 0 forces the three-launch rounds that rows longer than 4096 scalars use, classic == 0
 * the fused one-launch rounds (VPIN_ESHAPE where R has none).  Kernel-level parity handle. */
int vpin_bullet_reduce(vpin_ctx* c, const vpin_gens* g, const uint8_t* x_mont, const uint8_t* a_mont, size_t R, const uint8_t* u_mont,
                       int classic, uint8_t* cLR_out, uint8_t* LR_out, uint8_t xhat_ahat_out[64], uint8_t ghat_out[32]);

/* ---- host-only entry points (no GPU needed) -------------------------------------------- */
/* shape of the instance vpin_gadget_point_mult* (is_mult != 0) / vpin_gadget_point_add* will build for n_ops operations:
 * padded num_cons and num_vars and the non-zero entries of A, B, C (point_mult.rs:61-67, point_addition.rs:67-70) -- enough
 * for vpin_sat_prepare / vpin_spark_prepare before the witness has been read */
int vpin_gadget_shape(int is_mult, size_t n_ops, size_t* num_cons, size_t* num_vars, size_t nnz[3]);
/* (ABI 10) what vpin_dev_instance_proof_max_bytes and vpin_dev_instance_comm_bytes answer for the instance of that shape, and
 * the rows of its comm_para / comm_input, from (is_mult, n_ops) alone: what bounds a proof record before anything is allocated */
size_t vpin_gadget_proof_max_bytes(int is_mult, size_t n_ops);
size_t vpin_gadget_comm_bytes(int is_mult, size_t n_ops);
size_t vpin_gadget_vars_rows(int is_mult, size_t n_ops);
/* MultiCommitGens::new (Spartan/src/commitments.rs:20-38): first nb points of the stream */
int vpin_host_gens_derive(const char* label, size_t nb, uint8_t* out_xyzt /* nb*128 */);
/* Merlin: Transcript::new(proto); append_message(label,msg); challenge_bytes(clabel,out) */
int vpin_host_merlin_kat(const char* proto, const char* label, const uint8_t* msg, size_t n, const char* clabel,
                         uint8_t* out, size_t out_n);
/* Commitments::commit (commitments.rs:85-98) under MultiCommitGens::new(n,label), n <= 4 */
int vpin_host_commit(const char* label, const uint8_t* v_mont, size_t n, const uint8_t* blind_mont, uint8_t out[32]);

/* a*P + b*Q on the host (the verifier's variable-base multiplications, host/curve.h: width-5 NAF, shared doublings):
 * scalars in Montgomery form, points compressed; VPIN_EVERIFY when a point does not decode */
int vpin_host_scalar_mul2(const uint8_t a_mont[32], const uint8_t P[32], const uint8_t b_mont[32], const uint8_t Q[32], uint8_t out[32]);

/* self-test of the eq-factored sum-check round the product-circuit prover runs (EqRound, host/prover_common.h), replayed over
 * given sums and challenges; all scalars in Montgomery form.  rand = the layer's k challenges rho_j, claims / coeffs = npc
 * (+ 6 when with_dotp) scalars, res = per round 18 slots of 3 scalars: circuit t at slot t (lead != 0: t(0), the x^2
 * coefficient of t, unused; lead == 0: the sums at x = 0, 2, 3), dot-product half i at slot 12 + i (its sums at x = 0, 2, 3),
 * r = the k round challenges.  polys_out = per round the compressed cubic (coefficients 0, 2, 3), state_out = per round
 * e, s, cn after the challenge.  VPIN_ESHAPE for lead != 0 with a zero rho_j. */
int vpin_host_eq_round(const uint8_t* rand, int k, int npc, int with_dotp, int lead, const uint8_t* claims, const uint8_t* coeffs,
                       const uint8_t* res, const uint8_t* r, uint8_t* polys_out, uint8_t* state_out);

/* self-test of the pinned-memory mailbox framing used between resident kernels and the host (sequence number + checksum per
 * scalar; a torn or mixed publication is rejected and read again): 0 = as expected */
int vpin_host_mailbox_selftest(void);

/* ---- built-in kernel timing (HIP events on the ctx stream) ------------------------ */
/* kernel classes */
#define VPIN_K_SC_CUBIC 0
#define VPIN_K_SC_QUAD 1
#define VPIN_K_SC_BIND 2
#define VPIN_K_SC_CUBIC_FUSED 3
#define VPIN_K_SC_QUAD_FUSED 4
#define VPIN_K_EQ 5
#define VPIN_K_MSM 6
#define VPIN_K_SC_TAIL 7 /* single-workgroup tail rounds (<= 512 pairs), latency bound */
#define VPIN_K_SPARK_ROUND 8 /* batched cubic rounds of the product / dot-product circuits (SPARK) */
#define VPIN_K_SPARK_BUILD 9 /* SPARK gathers, hash layer, product-tree levels, slice evaluations */
#define VPIN_K_SPARK_ROUND_BIG 10 /* the subset of class 8 with >= 2^20 pairs per circuit: the streaming regime (also counted in 8) */
#define VPIN_K_MSM_ROWS 11 /* the subset of class 6 that is a row commitment of >= 128 rows (msm_rows_kernel; also counted in 6) */
#define VPIN_K_SPARK_TAIL 12 /* persistent tail launches (all the small rounds of one layer; time includes the host's turn-arounds) */
#define VPIN_K_COUNT 16
typedef struct {
  uint64_t launches;
  double ms;         /* sum of event-measured durations */
  double alg_bytes;  /* sum of algorithmic bytes moved by those launches */
  double units;      /* classes 8 / 10: pair evaluations (circuits x pairs); class 11 under vpin_prof_enable(ctx, 2): affine
                      * table additions those launches performed */
} vpin_kstat;
/* on = 1: HIP-event bracketing of the kernel classes; on = 2: additionally count the table additions of the row
 * commitments (an extra counting kernel per commitment: for roofline passes, not for timed regions) */
int vpin_prof_enable(vpin_ctx* ctx, int on);
int vpin_prof_reset(vpin_ctx* ctx);
/* resolves outstanding events; stats must have VPIN_K_COUNT entries */
int vpin_prof_read(vpin_ctx* ctx, vpin_kstat* stats);

#ifdef __cplusplus
}
#endif
#endif
