/* kgs.h — C-ABI of the MI355X-native KZG grand-sum / grand-product prover (libkgs.so).
 *
 * Drop-in boundary for the reference's hot path (xavi-pinsach/kzg-grandsums-study, JavaScript):
 * the reference has no native layer of its own; its arithmetic runs in the third-party
 * ffjavascript@0.2.59 / wasmcurves@0.2.1 wasm. Each entry point below names the reference
 * interface it replaces. Host bindings (N-API addon for the JS modules, ctypes for Python) are
 * shown in INTEGRATION.md.
 *
 * Conventions
 *  - Fr / Fq elements: 32 bytes little-endian. "mont" = Montgomery form with R = 2^256 (the
 *    in-memory form of every ffjavascript field element); "std" = standard form.
 *  - G1 affine points: 64 bytes x||y, each 32 B LE Montgomery Fq ("LEM", as in .ptau files and in
 *    ffjavascript `G1.toAffine` output); the point at infinity is 64 zero bytes.
 *  - Every call returns 0 on success or a negative KGS_E_* code; kgs_last_error() returns the
 *    message of the last failure on the calling thread. Semantic failures reproduce the
 *    reference's Error messages verbatim.
 *  - A context owns one HIP device, its HIP streams and work buffers. Every entry point taking a
 *    context holds that context's mutex for the whole call: calls on one context from several
 *    threads are serialised (a busy context blocks, it is never entered twice); independent
 *    contexts run concurrently. The SRS window tables and the NTT domain tables are read-only and
 *    shared by all contexts of a device (one copy per device, refcounted).
 */
#ifndef KGS_H
#define KGS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGS_OK 0
#define KGS_E_ARG (-1)             /* bad argument / shape */
#define KGS_E_HIP (-2)             /* HIP runtime failure */
#define KGS_E_NOT_WELL_CALC (-3)   /* "The grand-sum polynomial S is not well calculated" (grandsum.js:56)
                                      "The grand-product polynomial Z is not well calculated" (grandproduct.js:51) */
#define KGS_E_NOT_DIVISIBLE (-4)   /* "Polynomial is not divisible" (polynomial.js:878) */
#define KGS_E_DOES_NOT_DIVIDE (-5) /* "Polynomial does not divide" (polynomial.js:847) */
#define KGS_E_IO (-6)              /* ptau read/write failure (binfileutils / ptau_utils.js:3-24) */
#define KGS_E_SRS (-7)             /* "The Powers of Tau file is not sufficiently large ..." (prover.js:79-81) */
#define KGS_E_COMM (-8)            /* the shard all-gather callback reported a failure */
#define KGS_E_RANGE (-9)           /* reference-quirks mode only: "offset is out of bounds", the V8 RangeError the
                                      reference's divZh throws for a zero quotient (polynomial.js:857,884) */
#define KGS_E_NOT_IN_TABLE (-10)   /* "Row <i> of F is not in the table." (kgs_lookup_multiplicities: the lowest
                                      selected row of F that equals no row of the table) */

#define KGS_GRANDSUM 0
#define KGS_GRANDPRODUCT 1
/* Lookup (the commented-out cases of test/lookup_kzg_grandsum.test.js:24-44):
 * the selected grand-sum with sel_t carrying MULTIPLICITIES, so that
 *   sum_i selF_i / (f_i + gamma) == sum_i m_i / (t_i + gamma)
 * (f's selected values all occur in t). Identical to KGS_GRANDSUM with selectors in every respect
 * (transcript, proof layout, builder, error strings) except that the quotient and r(X) drop the
 * binary constraint on sel_t (the alpha^3 (selT - selT^2) term of prover.js:241-244 and
 * verifier.js:80-81). sel_f stays binary. Needs both selectors. Not in the reference, so parity is
 * against the oracle's restatement only. */
#define KGS_LOOKUP 2

typedef struct kgs_ctx kgs_ctx_t;

const char* kgs_last_error(void);
const char* kgs_version(void);

/* Number of visible HIP devices (the JS backend spreads its context pool over them). */
int kgs_device_count(int* count);
/* Create / destroy a context on HIP device `device`. kgs_ctx_destroy waits for a call still
 * running on the context. */
int kgs_ctx_create(int device, kgs_ctx_t** out);
void kgs_ctx_destroy(kgs_ctx_t* ctx);

/* ---- multi-GPU: MSM point-range sharding (replaces the [ffjs] worker-pool split
 * of G1.multiExpAffine, polynomial.js:1106-1115, by a split over one process per GPU).
 * With world > 1 every rank runs the whole prover on identical inputs; each commitment MSM over N
 * points is cut into `world` contiguous point ranges (kgs_shard_range), rank r runs Pippenger on
 * its range against the same resident SRS tables and the per-rank partials (c bit-sum points
 * T_k, XYZZ, 128 B each) are exchanged through `fn`, once per prover round. Every rank then
 * holds the same proof. `fn(user, send, recv, bytes)` must all-gather `bytes` from every rank
 * into recv (rank-major, world * bytes) and return 0; it is called in the same order on every
 * rank (the Python binding implements it over torch.distributed, i.e. RCCL on MI355X).
 * world == 1 turns sharding off. */
typedef int (*kgs_allgather_fn)(void* user, const uint8_t* send, uint8_t* recv, uint64_t bytes);
int kgs_ctx_set_shard(kgs_ctx_t* ctx, int rank, int world, kgs_allgather_fn fn, void* user);
/* rank's point range [lo, hi) of an n-point MSM: lo = floor(n*rank/world) */
int kgs_shard_range(uint64_t n, int rank, int world, uint64_t* lo, uint64_t* hi);
/* host-only: commitment from `nparts` rank partials (each c XYZZ points T_0..T_{c-1}, 128 B:
 * X,Y,ZZ,ZZZ LE Montgomery Fq, ZZ == 0 is infinity): sum_k 2^k sum_r T_k^(r) -> affine LEM */
int kgs_msm_combine(const uint8_t* T_all, int nparts, int c, uint8_t out_lem[64]);

/* ---- multi-GPU: the distributed prover (north_star: "the MSM and NTT
 * shard ... by scalar/point range and by butterfly stage across the 8 GPUs of one node").
 * A context attached to a group of W ranks (W = 1, 2, 4, 8 or 16; one context per rank) proves with
 * EVERY vector sharded: NTTs as a local transform + one all-to-all (CYCLIC <-> E layouts), the
 * grand-sum/product builder as a local scan + one all-gather of rank totals, the quotient and the
 * divisibility check on local slices with halo elements, Horner on CYCLIC slices, the synthetic
 * divisions on BLOCK slices with one all-gather of carries, and every MSM over the rank's slice of
 * the SRS. Each rank passes the FULL inputs (as for kgs_prove / kgs_prove_device) and receives the
 * identical, full proof (byte-identical to the single-GPU prover). Needs n >= 2 W^2.
 * All ranks must call the prover with the same arguments, in the same order. Each rank may hold the
 * whole SRS (kgs_srs_load_ptau: the MSMs read it with a point stride) or only its slice
 * (kgs_srs_load_ptau_slice(ctx, path, nbits, rank, world): 1/world of the tables).
 * Transports:
 *   local : several contexts of ONE process (one host thread per rank; devices may differ: attaching a
 *           context, kgs_ctx_set_group, enables peer access between its device and every other attached
 *           rank's device, and fails with KGS_E_COMM for a pair without peer access — the all-to-all
 *           then copies device to device over xGMI; UNVERIFIED on more than one device: every run of
 *           this build had one GPU, so all ranks shared a device)
 *   host  : any host all-gather callback (e.g. torch.distributed gloo); device data via the host
 *   rccl  : one process per GPU, RCCL over xGMI (rank 0 makes the id, the caller broadcasts it)
 * Failures:
 *   - rank-local preconditions (no / too small / wrong-slice SRS, pinned staging) are decided by all
 *     ranks together before the first exchange: every rank fails with the lowest failing rank's
 *     error and the group stays usable;
 *   - semantic prover errors (not well calculated / not divisible / does not divide) are decided
 *     from exchanged values, identically on every rank: the group stays usable;
 *   - anything else (HIP, allocation, transport) aborts the group: local / host peers fail at their
 *     next exchange; RCCL peers fail when their wait for the exchange passes the deadline
 *     KGS_GROUP_TIMEOUT_S (default 120 s; ncclCommAbort alone does not release them). The group is
 *     spent. The RCCL transport has run end to end with a one-rank communicator only (no multi-GPU
 *     box was available to this build); local-group runs of up to 16 ranks cover the data path. */
typedef struct kgs_group kgs_group_t;
int kgs_group_create_local(int world, kgs_group_t** out);
int kgs_group_create_host(int world, kgs_allgather_fn fn, void* user, kgs_group_t** out);
/* host transport with a real all-to-all: `a2a(user, send, recv, chunk)` sends chunk j of send (world
 * chunks of `chunk` bytes) to rank j and receives rank j's chunk for this rank into chunk j of recv
 * (e.g. torch.distributed all_to_all_single over gloo); returns 0. (W - 1) / W of a vector leaves a
 * rank per all-to-all, against W x the vector received through the all-gather-only transport. */
typedef int (*kgs_alltoall_fn)(void* user, const uint8_t* send, uint8_t* recv, uint64_t chunk);
int kgs_group_create_host_a2a(int world, kgs_allgather_fn fn, kgs_alltoall_fn a2a, void* user, kgs_group_t** out);
int kgs_group_rccl_unique_id(uint8_t id[128]);
int kgs_group_create_rccl(int rank, int world, const uint8_t id[128], int device, kgs_group_t** out);
void kgs_group_destroy(kgs_group_t* g);
int kgs_group_world(kgs_group_t* g, int* world);
/* attach (g != NULL) or detach (g == NULL) the distributed prover for this rank; a world-1 group
 * runs the distributed code path on one rank (exercises a transport end to end on one GPU) */
int kgs_ctx_set_group(kgs_ctx_t* ctx, kgs_group_t* g, int rank);
/* exchanges of the context's last proof (zeros after a single-GPU proof): out[0..5] = all-to-all
 * count, their summed span in ms (HIP events on the prover's stream around each exchange: the
 * transfer plus any wait for the peers), bytes that left this rank in them; host all-gather count,
 * their summed wall ms, bytes sent (bytes x (world - 1)). Returns the number of values written. */
int kgs_last_exchange(kgs_ctx_t* ctx, double* out, int max);

/* MSM lanes per context (default 2): with 2, the independent commitments of one prover round
 * (round 1's F_i / T_i, round 5's W_xi / W_xiw) alternate between two HIP streams with separate
 * work buffers, so one MSM's latency-bound tail overlaps the other's bucket accumulation
 * (single-proof latency -3 %, selected-vector 2^22 k=4 -7 %). Use 1 when several contexts already
 * keep the GPU busy with independent proofs (throughput). */
int kgs_ctx_set_msm_lanes(kgs_ctx_t* ctx, int lanes);

/* Reference-quirks mode (default ON since round 5: a new context is on unless the environment variable
 * KGS_REFERENCE_QUIRKS is "0"). On, the prover reproduces what the reference does on the degenerate
 * inputs where the reference does not compute the mathematical quotient (DESIGN.md §4 "Reference
 * quirks"); off (exact-math mode), it returns a valid proof for every valid
 * multiset. Detecting the degenerate inputs costs nothing measurable (93.0 proofs/s either way at
 * n = 2^20, profiles/r05/quirks_cost_ab.txt):
 *   - an operand of degree 1 <= d < n/2 (F, T, S/Z, selF, selT — e.g. F[i] = w^i): the reference's
 *     Polynomial.multiply evaluates it on the wrong points (polynomial.js:352-376 vs
 *     evaluations.js:12-18); the reference's quotient chain is then replayed on the GPU with the
 *     reference's buffer sizes and buffer sharing, and the prover fails where the reference fails
 *     ("Polynomial is not divisible", "Polynomial does not divide") or returns the proof it returns;
 *   - a zero quotient (e.g. F == T element by element): KGS_E_RANGE "offset is out of bounds".
 * Only the two reference arguments are affected (KGS_LOOKUP has no reference behaviour to follow). A
 * rank group (kgs_ctx_set_group) decides the degenerate cases from all-gathered degrees and replays
 * the chain on the gathered operands on every rank: every rank fails with the reference's error, or
 * returns the reference's proof. The replay reproduces transforms of up to 2^26 points (the
 * reference's own need n^2 points for a degree-1 operand); beyond that it fails with KGS_E_ARG.
 * One gap remains in rank groups: a replay that writes into polF's buffer (the unselected grand-sum's
 * polQ1.add(polF) on a shorter polQ1) makes a group fail with KGS_E_ARG where the
 * single-GPU prover follows the reference. No valid multiset of the test families reaches it with a
 * proof: the oracle restatement hits that write only on zero quotients (F == T), where the replay
 * first throws the reference's RangeError (DESIGN.md §13 "Q2 in rank groups"). */
int kgs_ctx_set_reference_quirks(kgs_ctx_t* ctx, int on);

/* Load a .ptau file (binfileutils layout, sections 1-3) and make the first 2^(nbits_max+1) G1
 * points device-resident, together with the MSM window tables and the NTT tables for domains
 * up to 2^nbits_max (nbits_max < 0: the file's power). Replaces readBinFile + readPTauHeader +
 * fd.readToBuffer(section 2) (src/grandsum/mset_eq_kzg_prover.js:15-16,83-85; src/ptau_utils.js:3-24),
 * which reads exactly domainSize*2 points per call: pass the proof's nBits as nbits_max.
 * Device SRS cache, grow-only: a context that already holds tables of the same file (same resolved
 * path, size and mtime) for a domain >= 2^nbits_max keeps them (no-op); tables of that file built
 * for a large enough domain by another context on the device are shared, not rebuilt. */
int kgs_srs_load_ptau(kgs_ctx_t* ctx, const char* path, int nbits_max);
/* A rank's slice of the SRS for the distributed prover (kgs_ctx_set_group, SURVEY.md §8e: "each GPU
 * holds only its SRS slice"): of the first 2^(nbits_max+1) points only rank + world * j are read,
 * made resident and window-expanded — 1/world of the tables of kgs_srs_load_ptau. Every MSM of the
 * distributed prover runs over the rank's CYCLIC slice, whose scalar j multiplies exactly point
 * rank + world * j, so this is all a rank needs. A context holding a slice proves only as that rank
 * of a group of that world (kgs_prove on it alone fails with KGS_E_ARG). Same grow-only cache. */
int kgs_srs_load_ptau_slice(kgs_ctx_t* ctx, const char* path, int nbits_max, int rank, int world);
/* slice of the resident SRS (world 1: the whole prefix) and the bytes of its window tables */
int kgs_srs_slice_info(kgs_ctx_t* ctx, int* rank, int* world, uint64_t* table_bytes);
/* Power of a ptau file from its header only (readPTauHeader, src/ptau_utils.js:3-24). */
int kgs_ptau_power(const char* path, int* power);
/* Same from in-memory LEM points (npts >= 2). `power` is the ceremony power to report. */
int kgs_srs_load_points(kgs_ctx_t* ctx, const uint8_t* g1_lem, uint64_t npts, int power, int nbits_max);
/* power of the loaded ptau, number of resident points, MSM window c */
int kgs_srs_info(kgs_ctx_t* ctx, int* power, uint64_t* npts, int* window_c);
/* *zero_points = 1 if some resident SRS point is the zero point (found when the window tables are
 * built; such a table runs the bucket accumulation with its affine-infinity test), 0 if none is,
 * -1 without an SRS */
int kgs_srs_zero_points(kgs_ctx_t* ctx, int* zero_points);
/* Read [tau]_2 (128 B LEM, section 3 offset 128) from a ptau (verifier input,
 * src/grandsum/mset_eq_kzg_verifier.js:18-19). */
int kgs_ptau_read_tau_g2(const char* path, uint8_t out128[128]);
/* Read [tau^k]_2, point k of section 3 (128 B LEM): a ceremony's ptau holds 2^power of them, the synthetic
 * writer's two ([1]_2 and [tau]_2). KGS_E_IO when the section holds fewer than k + 1 points. k = 1 is
 * kgs_ptau_read_tau_g2. kgs_kzg_verify_coset takes [tau^l]_2. */
int kgs_ptau_read_tau_g2_pow(const char* path, uint64_t k, uint8_t out128[128]);

/* Write a synthetic ptau (sections 1-3 with the hermez layout; section 3 holds [1]_2 and
 * [tau]_2 only) for a known tau (32 B LE standard form). G1 powers are generated on the GPU of
 * `ctx` (or on the CPU if ctx == NULL). */
int kgs_ptau_write_synthetic(kgs_ctx_t* ctx, const char* path, int power, const uint8_t tau_std[32]);

/* Full prover — replaces mset_eq_kzg_{grandsum,grandproduct}_prover
 * (src/grandsum/mset_eq_kzg_prover.js:12, src/grandproduct/mset_eq_kzg_prover.js:12).
 *   kind      KGS_GRANDSUM | KGS_GRANDPRODUCT | KGS_LOOKUP (grand-sum layout; selectors required)
 *   nbits     domain size n = 2^nbits (1 <= nbits <= SRS nbits_max)
 *   npols     k >= 1 (vector argument when k > 1)
 *   evals_f/t k host pointers, n x 32 B STANDARD-form evaluations each (the caller's
 *             Evaluations.eval before prover.js:147-148)
 *   sel_f/t   n x 32 B MONTGOMERY selector evaluations, or both NULL (unselected; the wrapper
 *             passes NULL when both are all Fr.one, prover.js:63-68)
 *   mont_f/t  optional k output pointers (n x 32 B) receiving the Montgomery evaluations that the
 *             reference writes back into the caller's objects (prover.js:147-148); may be NULL
 *   commitments_out  (#commitments x 64 B LEM), order:
 *             grand-sum:     F0,T0,..,F{k-1},T{k-1}, [selF,selT], S, Q, Wxi, Wxiw
 *             grand-product: F0,T0,..,F{k-1},T{k-1}, [selF,selT], Z, Q, Wxi, Wxiw
 *   evaluations_out  (#evaluations x 32 B Montgomery), order:
 *             grand-sum:     f0,t0,..,f{k-1},t{k-1}, [selF,selT], sxiw
 *             grand-product: f0,..,f{k-1}, [selF,selT], zxiw
 */
int kgs_prove(kgs_ctx_t* ctx, int kind, int nbits, int npols, const uint8_t* const* evals_f,
              const uint8_t* const* evals_t, const uint8_t* sel_f, const uint8_t* sel_t, uint8_t* const* mont_f,
              uint8_t* const* mont_t, uint8_t* commitments_out, uint8_t* evaluations_out);
/* Host-buffer boundary: kgs_prove copies pageable inputs into pinned staging (pieces overlapped with
 * their DMA) and the Montgomery outputs back out of it. Buffers the caller has pinned — hipHostMalloc
 * or kgs_host_register, for buffers reused across proofs — are DMA'd in place with no staging copy;
 * kgs_host_unregister before freeing a registered buffer. Registration costs more than one copy
 * (profiles/r03/boundary_ab.txt): register only buffers that outlive several proofs. */
int kgs_host_register(void* ptr, uint64_t bytes);
int kgs_host_unregister(void* ptr);
/* Every kgs_prove / kgs_prove_device call returns with none of its transfers or kernels pending, on
 * its error paths too (a failed call drains the context's streams before it returns), so a caller may
 * unregister or free its buffers as soon as the call returns. A context attached to a rank group
 * (kgs_ctx_set_group) is exempt on its error paths: its main stream may wait in an exchange whose
 * peers failed (the group's abort releases it), so a failed call does not drain it; such a context
 * never reads or writes caller host memory in place. kgs_ctx_idle reports 1 when no stream
 * of the context has work outstanding, 0 otherwise (diagnostic; the tests check the contract). */
int kgs_ctx_idle(kgs_ctx_t* ctx);
/* Same with device-resident inputs (HIP device pointers on ctx's device). */
int kgs_prove_device(kgs_ctx_t* ctx, int kind, int nbits, int npols, const void* const* d_evals_f,
                     const void* const* d_evals_t, const void* d_sel_f, const void* d_sel_t, uint8_t* commitments_out,
                     uint8_t* evaluations_out);
/* number of commitments / evaluations a proof of this shape produces */
int kgs_proof_shape(int kind, int npols, int selected, int* n_commitments, int* n_evaluations);

/* ---- verifiers (host only; no context, no GPU) -------------------------------------------
 * mset_eq_kzg_grandsum_verifier / mset_eq_kzg_grandproduct_verifier
 * (src/grandsum/mset_eq_kzg_verifier.js:9, src/grandproduct/mset_eq_kzg_verifier.js:9): commitment
 * and evaluation buffers in the fixed order kgs_prove writes (kgs_proof_shape; KGS_LOOKUP proofs
 * are checked with kind KGS_LOOKUP and selected = 1); tau_g2 = [tau]_2 as
 * 128 B LEM (the second point of ptau section 3, kgs_ptau_read_tau_g2). Returns 1 (valid), 0
 * (invalid: not on G1, evaluation >= r, or the pairing equation fails) or a negative error.
 * One proof per call, two Miller loops and a final exponentiation each: kgs_verify_batch below shares
 * one pairing check between all proofs checked against the same [tau]_2. */
int kgs_verify(int kind, int nbits, int npols, int selected, const uint8_t* commitments, const uint8_t* evaluations,
               const uint8_t tau_g2[128]);
int kgs_verify_ptau(int kind, const char* ptau_path, int nbits, int npols, int selected, const uint8_t* commitments,
                    const uint8_t* evaluations);
/* curve.pairingEq (src/grandsum/mset_eq_kzg_verifier.js:182, src/grandproduct/mset_eq_kzg_verifier.js:177;
 * [ffjs] bn128 optimal-ate pairing): 1 if prod_k e(P_k, Q_k) == 1, 0 if not. P_k: affine LEM G1
 * (64 B, Montgomery; (0, 0) = infinity), Q_k: affine LEM G2 (128 B: x.c0, x.c1, y.c0, y.c1). Points
 * off their curve: KGS_E_ARG. Host only. */
int kgs_pairing_eq(int npairs, const uint8_t* g1_lem, const uint8_t* g2_lem);

/* ---- batch verifier: many proofs against one [tau]_2, one pairing check (DESIGN.md "Batch verifier").
 * For each proof the verifier's equation is e(-A_i, [tau]_2) * e(B_i, [1]_2) == 1 with A_i, B_i short
 * linear combinations of the proof's own commitments and the generator (Fr scalars from the transcript
 * replay and the evaluations). The batch draws weights rho_i, folds rho_i * A_i and rho_i * B_i for
 * every proof (independent work per proof: on the GPU of `ctx`, kgs_g1_lincomb below), sums them and
 * performs ONE 2-pair pairing check e(-sum rho_i A_i, [tau]_2) * e(sum rho_i B_i, [1]_2) == 1.
 *
 * Weights (deterministic: a batch gives the same bytes on every run; LE32 = 4 bytes little-endian)
 *   seed  = keccak256("kgs-verify-batch-v1" || tau_g2 (128 B) || LE32(count) || for each proof in order:
 *           LE32(kind) || LE32(nbits) || LE32(npols) || LE32(selected) || commitments || evaluations)
 *   rho_i = the first 16 bytes of keccak256(seed || LE32(i)) read as a little-endian integer; 0 -> 1
 * Soundness: the weights are fixed by a hash of everything the check depends on, so (in the random-oracle
 * model) they are independent of the proofs' pairing residues; if some proof of the batch fails its own
 * equation, the weighted product is 1 for at most one value of that proof's weight given the others, so a
 * batch holding an invalid proof passes the aggregate check with probability at most 2^-128.
 *
 * A proof with a commitment off G1 or an evaluation >= r (the structural checks of kgs_verify) is
 * marked invalid first and contributes no term: only points on the curve are folded.
 * If the aggregate check fails and valid_out != NULL, the invalid proofs are located by bisection over
 * the per-proof folded points (host point additions and further pairing checks, never a second fold; a
 * half whose sibling passes under a failing parent is known to fail without a check): with b invalid
 * proofs, pairing_checks <= 1 + 2 b ceil(log2 count) and never more than 2 count - 1. With
 * valid_out == NULL the call stops after the aggregate check. Verdicts equal kgs_verify's.
 *
 * Returns 1 (every proof valid), 0 (some proof invalid) or a negative KGS_E_*: a bad kind / nbits /
 * npols, a KGS_LOOKUP proof without selectors, a NULL buffer or a tau_g2 off its curve give KGS_E_ARG
 * as for kgs_verify; so does a context attached to a rank group. count == 0 returns 1.
 * ctx == NULL folds on the host (no GPU is touched). With a context the call holds its mutex, uses
 * device buffers of its own (sized by the number of terms; the SRS, the domain tables and the prover's
 * work buffers are left as they are) and returns with nothing pending on the context's streams, on
 * its error paths too (kgs_ctx_idle). The environment variable KGS_VERIFY_BATCH_FOLD = "gpu" | "host"
 * forces where a call with a context folds (default: the GPU from 128 terms on, about a dozen proofs,
 * the host below: the measured crossover; diag->on_gpu tells which). */
typedef struct {
  int kind, nbits, npols, selected;
  const uint8_t* commitments; /* kgs_proof_shape order, 64 B affine LEM each */
  const uint8_t* evaluations; /* 32 B Montgomery each */
} kgs_proof_ref_t;
typedef struct {           /* optional; every pointer member optional (NULL: not wanted) */
  uint8_t* weights_out;    /* in: count x 32 B, receives rho_i in standard form LE */
  uint8_t* folded_out;     /* in: count x 128 B, receives rho_i*A_i || rho_i*B_i, affine LEM; zeros for a
                              structurally invalid proof */
  uint32_t pairing_checks; /* out: 2-pair pairing checks performed */
  uint32_t terms;          /* out: (scalar, point) terms folded */
  int on_gpu;              /* out: 1 if the fold ran on the GPU */
  double fold_ms, pairing_ms; /* out: wall clock of the fold and of all pairing checks */
} kgs_batch_diag_t;
int kgs_verify_batch(kgs_ctx_t* ctx, const kgs_proof_ref_t* proofs, int count, const uint8_t tau_g2[128],
                     uint8_t* valid_out /* count bytes (1 valid, 0 invalid) or NULL */, kgs_batch_diag_t* diag);
int kgs_verify_batch_ptau(kgs_ctx_t* ctx, const char* ptau_path, const kgs_proof_ref_t* proofs, int count,
                          uint8_t* valid_out, kgs_batch_diag_t* diag);

/* ---- multi-argument proofs: m arguments over one domain, one quotient, one pair of openings
 * (the reference's TODO "run in the case of multiple arguments (of any kind) at the same
 * time"). Argument j (0 <= j < m, 1 <= m <= KGS_MAX_ARGS) has its own kind (KGS_GRANDSUM,
 * KGS_GRANDPRODUCT or KGS_LOOKUP), number of columns and selectors, in any mix; all share the domain
 * 2^nbits. The arguments share beta (drawn if any of them is a vector argument), gamma, alpha, xi, v and
 * u; a separator delta, drawn after alpha when m > 1, weights argument j's quotient numerator N_j and
 * linearisation r_j by delta^j:
 *   Q     = (sum_j delta^j N_j) / Z_H
 *   W_xi  opens r = sum_j delta^j r_j - Z_H(xi) Q and every round-1 polynomial at xi (v^1, v^2, .. in
 *         proof order: per argument the F's, the T's of a grand-sum / lookup, then selF, selT)
 *   W_xiw opens sum_j v^j S_j at xi w
 * so m arguments cost 3 commitments of n points each plus ONE Q, W_xi and W_xiw (about 3 n m + 5 n MSM
 * points against 8 n m for m single proofs), the proof holds sum_j (2 k_j + 2 sel_j) + m + 3 points
 * and is checked by one pairing equation. With m = 1 no delta is drawn and the proof is byte for byte
 * kgs_prove's in exact-math mode.
 *   commitments_out  every argument's round-1 commitments, argument by argument in kgs_prove's order
 *                    (F0,T0,..,[selF,selT]), then S_0 .. S_{m-1} (Z for a grand-product), Q, Wxi, Wxiw
 *   evaluations_out  every argument's evaluations at xi, argument by argument in kgs_prove's order
 *                    (f0,t0,.. for a grand-sum / lookup, f0,.. for a grand-product, [selF,selT]), then
 *                    S_0(xi w) .. S_{m-1}(xi w)
 * Transcript: all round-1 commitments in that order -> [beta, absorbed] -> gamma; gamma, S_0 .. S_{m-1}
 * -> alpha; [alpha -> delta]; delta (alpha when m = 1), Q -> xi; xi, the evaluations in that order -> v;
 * v, Wxi, Wxiw -> u.
 * The prover is always exact-math (as for KGS_LOOKUP there is no reference behaviour to follow:
 * kgs_ctx_set_reference_quirks has no effect on it). Context contract of the provers: the call holds the
 * context's mutex and returns with nothing pending on its streams, on its error paths too
 * (kgs_ctx_idle). kgs_prove_multi takes host pointers and stages them with plain copies (no pipelined
 * staging, and no Montgomery write-back: that is a side effect of the reference's single provers);
 * kgs_prove_multi_device takes device pointers on ctx's device.
 * Failures: the codes of kgs_prove. An argument's own failure carries the reference's message prefixed
 * with "argument <j>: " for the lowest failing j: KGS_E_NOT_WELL_CALC ("The grand-sum polynomial S is not
 * well calculated" / its grand-product form), KGS_E_NOT_DIVISIBLE ("Polynomial is not divisible"), and
 * the KGS_E_ARG of a bad kind or npols or of a lookup without selectors. KGS_E_DOES_NOT_DIVIDE
 * ("Polynomial does not divide") belongs to the shared openings and names no argument; KGS_E_SRS keeps
 * the reference's SRS message. KGS_E_ARG also for count outside 1 .. KGS_MAX_ARGS, an nbits outside
 * 1 .. 28 or above the nbits_max the SRS was loaded for, a context attached to a rank group
 * (kgs_ctx_set_group) and a context with MSM sharding switched on (kgs_ctx_set_shard). */
#define KGS_MAX_ARGS 16
typedef struct {
  int kind, npols, selected;
} kgs_arg_shape_t;
typedef struct {
  int kind, npols;
  const void* const* evals_f; /* npols pointers, n x 32 B STANDARD form each */
  const void* const* evals_t;
  const void* sel_f; /* n x 32 B MONTGOMERY, or both NULL (unselected) */
  const void* sel_t;
} kgs_arg_t;
/* number of commitments / evaluations of a multi-argument proof of these shapes */
int kgs_multi_proof_shape(const kgs_arg_shape_t* args, int count, int* n_commitments, int* n_evaluations);
int kgs_prove_multi(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* args, int count, uint8_t* commitments_out,
                    uint8_t* evaluations_out);
int kgs_prove_multi_device(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* args, int count, uint8_t* commitments_out,
                           uint8_t* evaluations_out);
/* Verifier of a multi-argument proof (host only, as kgs_verify): 1 (valid), 0 (invalid: a commitment not
 * on G1, an evaluation >= r, or the pairing equation e(-A, [tau]_2) e(B, [1]_2) == 1 fails) or a negative
 * code (KGS_E_ARG: a bad count, kind, npols or nbits, a lookup without selectors, a NULL buffer, a tau_g2
 * off its curve). A = Wxi + u Wxiw; B = the per-argument terms of kgs_verify's equation weighted by
 * delta^j, u v^j on each S_j, xi Wxi + u xi w Wxiw and the evaluations' scalar multiple of the generator.
 * With count = 1 the verdict is kgs_verify's. */
int kgs_verify_multi(int nbits, const kgs_arg_shape_t* args, int count, const uint8_t* commitments,
                     const uint8_t* evaluations, const uint8_t tau_g2[128]);
int kgs_verify_multi_ptau(const char* ptau_path, int nbits, const kgs_arg_shape_t* args, int count,
                          const uint8_t* commitments, const uint8_t* evaluations);

/* Per-proof timing of the last kgs_prove* call (milliseconds, host wall clock): [0..4] prover rounds
 * 1-5, [5] unused, and for kgs_prove (host buffers) [6] input copy into pinned staging, [7] the
 * prover, [8] wait for the Montgomery write-back to the caller. Returns the number written. */
int kgs_last_timing(kgs_ctx_t* ctx, double* rounds_ms, int max_rounds);

/* ---- primitives (host buffers in/out; used by tests and by the bench's roofline legs) ---- */
/* [ffjs] Fr.batchToMontgomery */
int kgs_fr_to_mont(kgs_ctx_t* ctx, const uint8_t* in_std, uint8_t* out_mont, uint64_t n);
/* [ffjs] Fr.batchFromMontgomery (polynomial.js:1112): out = in * 2^-256, canonical */
int kgs_fr_from_mont(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_std, uint64_t n);
/* [ffjs] Fr.batchInverse (grandsum.js:41, grandproduct.js:36): out[i] = in[i]^-1, zero stays zero */
int kgs_fr_batch_inverse(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_mont, uint64_t n);
/* [ffjs] Fr.fft / Fr.ifft: natural order in and out, size 2^logm, ifft includes 1/m */
int kgs_ntt(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_mont, int logm, int inverse);
/* The transforms as the provers launch them (a test primitive: the forward and inverse passes with their
 * fused coset scalings, input length, orders and pass build). m = 2^logm, w = Fr.w[logm], g =
 * KGS_NTT_COSET_GEN, rev = the bit reversal of logm-bit indices, NTT / INTT = kgs_ntt's forward /
 * inverse (INTT with its 1/m). in_mont holds in_len elements (forward) or m elements (inverse), out_mont
 * m elements.
 *   forward (no KGS_NTT_INVERSE): in_len in 0 .. m; a_j = in[j] for j < in_len, 0 for in_len <= j < m
 *     b_j = a_j g^j with KGS_NTT_COSET, else a_j                 A = NTT(b), A_k = sum_j b_j w^(jk)
 *     out[k] = A_rev(k) with KGS_NTT_BITREV (the DIF's own order), else A_k
 *   inverse (KGS_NTT_INVERSE): in_len is ignored
 *     e_j = in[rev(j)] with KGS_NTT_BITREV (input in bit-reversed order), else in[j]
 *     B = m INTT(e) with KGS_NTT_NO_SCALE (B_k = sum_j e_j w^(-jk)), else INTT(e)
 *     out[k] = B_k g^-k with KGS_NTT_COSET, else B_k
 *   KGS_NTT_INPLACE  the transform writes the device buffer it reads (same values)
 *   KGS_NTT_INFLIGHT the pass build of one-lane (in-flight) contexts instead of the default one (same values)
 * KGS_NTT_NO_SCALE means nothing to a forward call. The prover's launches: its coset evaluation of a
 * polynomial is forward COSET | BITREV with in_len <= m; its quotient's return to coefficients inverse
 * COSET | BITREV | NO_SCALE | INPLACE; the distributed prover's last pass inverse COSET; the reference
 * replay forward with in_len < m; kgs_ntt flags 0 and KGS_NTT_INVERSE.
 * KGS_E_ARG: logm outside 0 .. 28, a flag bit not listed here, a forward in_len > m, and inverse INPLACE
 * without BITREV (that pass would gather bit-reversed addresses of the buffer it is writing). */
#define KGS_NTT_COSET_GEN 5 /* the coset of every coset transform is g <w>, g = Fr's first non-residue */
#define KGS_NTT_INVERSE 1
#define KGS_NTT_COSET 2
#define KGS_NTT_BITREV 4
#define KGS_NTT_NO_SCALE 8
#define KGS_NTT_INPLACE 16
#define KGS_NTT_INFLIGHT 32
int kgs_ntt_ex(kgs_ctx_t* ctx, const uint8_t* in_mont, uint64_t in_len, uint8_t* out_mont, int logm, int flags);
/* The batched block transforms as the coset openings and the recovery launch them (a test primitive, like
 * kgs_ntt_ex): B = 2^(logtotal - s) transforms of size m = 2^s over the consecutive blocks of one array of
 * 2^logtotal elements, in place on the device. in_mont and out_mont hold 2^logtotal elements; block b is the
 * elements b m .. b m + m - 1; rev = the bit reversal of s-bit indices; NTT / INTT = kgs_ntt's forward / inverse
 * of size m (INTT with its 1/m). For every block b < B and k < m:
 *   forward (no KGS_NTT_INVERSE): x_j = in[b m + j]          out[b m + k] = NTT(x)_rev(k)   (natural in, bit-reversed out)
 *   inverse (KGS_NTT_INVERSE):    e_j = in[b m + rev(j)]     out[b m + k] = INTT(e)_k       (bit-reversed in, natural out)
 *     with KGS_NTT_NO_SCALE                                  out[b m + k] = m INTT(e)_k = sum_j e_j w^(-jk), w = Fr.w[s]
 *   KGS_NTT_INFLIGHT the pass build of one-lane (in-flight) contexts instead of the default one (same values)
 * That is kgs_ntt_ex(block, m, s, KGS_NTT_BITREV) and kgs_ntt_ex(block, m, s, KGS_NTT_INVERSE | KGS_NTT_BITREV
 * [| KGS_NTT_NO_SCALE]) block by block; s == 0 returns the input. The domain tables grow to 2^s only, never to
 * 2^logtotal, as in the calls that launch these transforms (kgs_kzg_open_cosets_many, kgs_kzg_recover_cosets,
 * kgs_kzg_recover_cosets_many): the passes read the stage tables by stage, not by transform size.
 * KGS_E_ARG: logtotal outside 0 .. 28, s outside 0 .. logtotal, a flag bit other than the three above, NULL. */
int kgs_ntt_blocks(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_mont, int logtotal, int s, int flags);
/* [ffjs] G1.multiExpAffine(SRS[0..n), fromMont(scalars)) + toAffine (polynomial.js:1106-1115).
 * The scalars are canonical Montgomery forms (below r; any representative below 2^254 is taken). */
int kgs_msm(kgs_ctx_t* ctx, const uint8_t* scalars_mont, uint64_t n, uint8_t out_lem[64]);
/* ComputeSGrandSumPolynomial / ComputeZGrandProductPolynomial evaluations before the ifft
 * (grandsum.js:6-57, grandproduct.js:6-52): out = S (or Z) evaluations, natural order */
int kgs_grand_build(kgs_ctx_t* ctx, int kind, const uint8_t* f_mont, const uint8_t* t_mont, const uint8_t* sel_f,
                    const uint8_t* sel_t, const uint8_t gamma_mont[32], uint64_t n, uint8_t* out_mont);
/* ---- round 3 as the provers launch it (test primitives, like kgs_ntt_ex: the entry points below and the
 * round engine call the same host functions, so the scalar set-up and the launch choice under test are
 * the provers' own). Per point, with s = S(x), sw = S(w x), f, t, and sf, st the selector values
 * (unselected: absent), every product in Fr:
 *   core  = [selected: ((st - st^2) a_t + (sf - sf^2)) alpha, a_t = 0 for KGS_LOOKUP, alpha otherwise] +
 *           grand-sum / lookup:  (sw - s)(f + gamma)(t + gamma) + (selected: st (f + gamma) - sf (t + gamma);
 *                                                                 unselected: f - t)
 *           grand-product:       sw dT - s dF,  dT = t + gamma, dF = f + gamma (unselected),
 *                                dT = st (t + gamma - 1) + 1, dF = sf (f + gamma - 1) + 1 (selected)
 *   l1op  = s (grand-sum / lookup), s - 1 (grand-product)
 * The quotient numerator of an argument is N(x) = alpha core(x) + L1(x) l1op(x) (prover.js:233-286).
 *
 * kgs_quotient_ex: the quotient of `count` arguments on a coset, (sum_j delta^j N_j) / Z_H times 1/cs (the
 * scaling of the inverse transform that follows it in the prover, KGS_NTT_NO_SCALE). n = 2^nbits,
 * cs = 2^lcs, rot = cs / n, g = KGS_NTT_COSET_GEN, w_cs = Fr.w[lcs], rev = the bit reversal of lcs-bit
 * indices. Every array holds cs elements indexed by p as the kernels read them (the order of a forward
 * KGS_NTT_COSET | KGS_NTT_BITREV transform): i = rev(p), x_i = g w_cs^i, and S_j(w x_i) is S_j[p'] with
 * p' = rev((i + rot) mod cs). The values are arbitrary field elements (no degree is assumed).
 *   q_out[p] = (1/cs) [ alpha / (x_i^n - 1) * sum_j delta^j core_j(p)  +  1 / (n (x_i - 1)) * sum_j delta^j l1op_j(p) ]
 * count == 1 runs the single proof's kernel (delta_mont is ignored, and may be NULL), or with
 * KGS_QUOT_FUSED the multi-argument kernel on one argument (the same values); count > 1 runs the
 * multi-argument kernel in groups of eight arguments, the later groups adding to q_out. The 1/(n (x - 1))
 * table is the context's own, cached per (nbits, lcs). The domain tables grow on demand as for kgs_ntt_ex;
 * no SRS is needed.
 * KGS_E_ARG: nbits outside 1 .. 27, lcs other than nbits or nbits + 1, count outside 1 .. KGS_MAX_ARGS, a
 * flag bit other than KGS_QUOT_FUSED, an unknown kind, a NULL array or scalar (sel_f and sel_t must be both
 * NULL or both set, and KGS_LOOKUP needs them). */
typedef struct {
  int kind;                                 /* KGS_GRANDSUM | KGS_GRANDPRODUCT | KGS_LOOKUP */
  const uint8_t *S, *F, *T, *sel_f, *sel_t; /* cs x 32 B Montgomery each */
} kgs_quot_arg_t;
#define KGS_QUOT_FUSED 1
int kgs_quotient_ex(kgs_ctx_t* ctx, int nbits, int lcs, const kgs_quot_arg_t* args, int count,
                    const uint8_t alpha_mont[32], const uint8_t gamma_mont[32], const uint8_t delta_mont[32], int flags,
                    uint8_t* q_out);
/* The divisibility check of round 3 (the test behind "Polynomial is not divisible"): *nonzero = 1 iff
 * N(w^(gbase + i)) != 0 for some i < n, else 0, with
 *   N(w^(gbase + i)) = alpha core(i) + (gbase + i == 0 ? l1op(i) : 0)        (L1 is 1 at w^0, 0 elsewhere on H)
 * over n x 32 B Montgomery arrays in natural order, core(i) taking sw = S[i + 1] for i + 1 < n and
 * sw = *s_next for i = n - 1 (s_next == NULL: S[0], the wrap of a whole domain). n is any value >= 1 (up
 * to 2^28), not only a power of two: with s_next and gbase this is the check of one block of a larger
 * domain, as the distributed prover runs it on a rank's block, here without a rank group.
 * KGS_E_ARG: n outside 1 .. 2^28, an unknown kind, a NULL array, scalar or result, one selector without the
 * other, KGS_LOOKUP without selectors. */
int kgs_divcheck(kgs_ctx_t* ctx, int kind, uint64_t n, const uint8_t* S, const uint8_t* f, const uint8_t* t,
                 const uint8_t* sel_f, const uint8_t* sel_t, const uint8_t alpha_mont[32], const uint8_t gamma_mont[32],
                 const uint8_t* s_next, uint64_t gbase, int* nonzero);
/* The provers' linear combination of vectors (round 2's beta combinations, round 5's opening numerators):
 *   out[i] = sum over the k with i < lens[k] of coef_k srcs[k][i]  +  (i == 0 ? c0 : 0),   i < out_len
 * srcs[k] holds lens[k] x 32 B Montgomery elements (lens[k] may exceed out_len, and may be 0 with
 * srcs[k] == NULL); coefs_mont holds count x 32 B. Terms are taken 32 to a launch, the later launches
 * re-reading out as their first source. Source pointers that are equal are one device buffer, as in the
 * prover, where a polynomial can enter a combination more than once.
 * KGS_E_ARG: count outside 0 .. 256, out_len outside 1 .. 2^28, a lens[k] above 2^28, a NULL pointer
 * (srcs, lens and coefs_mont may be NULL when count == 0). */
int kgs_lincomb(kgs_ctx_t* ctx, const uint8_t* const* srcs, const uint64_t* lens, const uint8_t* coefs_mont, int count,
                const uint8_t c0_mont[32], uint64_t out_len, uint8_t* out_mont);
/* Polynomial.evaluate (polynomial.js:228-238) */
int kgs_poly_eval(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t x_mont[32],
                  uint8_t out_mont[32]);
/* Polynomial.divByXSubValue (polynomial.js:814-851); out has `len` coefficients */
int kgs_poly_div_x_sub(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t z_mont[32],
                       uint8_t* out_mont);
/* Multiplicities of a lookup (the sel_t of a KGS_LOOKUP proof) from the witness and the table: a hash
 * join on the GPU. mul_t[j] = number of rows i of F with sel_f[i] == one that equal row j of T,
 * as a 32 B Montgomery element. No SRS is needed.
 *   npols     k in 1 .. 32; a row is the k-tuple (col_0[i], .., col_{k-1}[i])
 *   n         rows of F and of T, any value in 1 .. 2^28 (not only powers of two)
 *   evals_f/t k host pointers, n x 32 B STANDARD-form evaluations each, as kgs_prove takes them (read
 *             only). Rows are equal when all k components are equal as elements of Fr: a stored value
 *             v >= r counts as v mod r.
 *   sel_f     n x 32 B MONTGOMERY selector (zero or one per row), or NULL: every row is selected
 * A table row that occurs several times receives ALL of its multiplicity at its FIRST occurrence (the
 * lowest index); its later occurrences get zero. Any split over the occurrences proves; this one is
 * fixed so that the output is the same bytes on every run.
 * Failures (the output's contents are then unspecified):
 *   KGS_E_ARG           "selF is not binary at row <i>." — the lowest row whose selector is neither
 *                       zero nor one (reported before a missing row); bad npols / n / NULL; a context
 *                       attached to a rank group (kgs_ctx_set_group: not supported)
 *   KGS_E_NOT_IN_TABLE  "Row <i> of F is not in the table." — the lowest selected row without a match
 * Like the provers, the call returns with nothing pending on the context's streams, on its error
 * paths too (kgs_ctx_idle). */
int kgs_lookup_multiplicities(kgs_ctx_t* ctx, int npols, uint64_t n, const uint8_t* const* evals_f,
                              const uint8_t* const* evals_t, const uint8_t* sel_f, uint8_t* mul_t_mont);
/* Same with device pointers in and out (on ctx's device): the n x 32 B output is what
 * kgs_prove_device(KGS_LOOKUP, ..) takes as d_sel_t, so a device-resident witness and table never
 * leave the GPU between the two calls. */
int kgs_lookup_multiplicities_device(kgs_ctx_t* ctx, int npols, uint64_t n, const void* const* d_evals_f,
                                     const void* const* d_evals_t, const void* d_sel_f, void* d_mul_t_mont);
/* Segmented G1 linear combination (the fold of kgs_verify_batch): out_lem[s] = sum over the terms t in
 * [seg_off[s], seg_off[s + 1]) of scalar_t * P_t, for s < nseg. points_lem: affine LEM points on the
 * curve, the zero point allowed (a point off the curve or with a coordinate >= q: KGS_E_ARG);
 * scalars_std: 32 B little-endian STANDARD form each, any 256-bit integer; seg_off: nseg + 1
 * non-decreasing term offsets starting at 0 (at most 2^26 terms and segments). An empty segment or a
 * sum equal to the identity gives 64 zero bytes. ctx == NULL computes on the host; with a context, one
 * thread per term does double-and-add on the GPU, one per segment sums, and the results are made
 * affine by a batched inversion. No SRS is needed, none is touched. Same context contract as
 * kgs_lookup_multiplicities (mutex, no rank group, idle on return). */
int kgs_g1_lincomb(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, const uint64_t* seg_off,
                   uint64_t nseg, uint8_t* out_lem);
/* Variable-base MSM ([ffjs] G1.multiExpAffine over arbitrary bases): out_lem = sum_i s_i * P_i for
 * i < n. No window tables are built: the points are read as given (one 64 B row, O(n) device memory),
 * where kgs_msm runs over the resident SRS tables that kgs_srs_load_* expands once.
 *   points_lem   n affine LEM points, 64 B each; 64 zero bytes is the identity, allowed anywhere.
 *                Points are NOT validated (as for kgs_srs_load_points and [ffjs]): a point off the
 *                curve or a coordinate >= q gives an unspecified result, never a fault.
 *   scalars_std  n x 32 B little-endian STANDARD form; any 256-bit integer, taken mod r (which is the
 *                integer multiple for every point of G1: the cofactor is 1)
 *   n            0 .. 2^26; n == 0 gives the identity
 *   window_c     0: the library chooses (clamp(ceil(log2 n) - 4, 7, 16)); 7 .. 16: that window, used as
 *                given (for tests and tuning; with window_c == 7, n <= 2^31 / 37)
 *   out_lem      affine LEM, the identity as 64 zero bytes
 * ctx == NULL computes on the host (no GPU is touched; window_c is only range-checked).
 * Failures: KGS_E_ARG for a window_c outside {0, 7 .. 16}, a NULL buffer with n > 0, n above the limit,
 * a context attached to a rank group (kgs_ctx_set_group) or with MSM sharding on (kgs_ctx_set_shard).
 * Same context contract as kgs_lookup_multiplicities and kgs_g1_lincomb: the call holds the context's
 * mutex, uses device buffers of its own (sized from n and the window), needs no SRS and leaves the
 * resident SRS, the domain tables and the prover's MSM work buffers as they are, and returns with nothing
 * pending on the context's streams, on its error paths too (kgs_ctx_idle). */
int kgs_msm_points(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t n, int window_c,
                   uint8_t out_lem[64]);
/* Same with device pointers (on ctx's device; ctx must not be NULL). Both buffers are read only: the
 * points are copied into a buffer of the library's own before they are converted. */
int kgs_msm_points_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t n,
                          int window_c, uint8_t out_lem[64]);
/* [ffjs] G1.fft / G1.ifft: the radix-2 number-theoretic transform over G1 with the conventions of Fr.fft /
 * Fr.ifft (kgs_ntt), natural order in and out:
 *   forward  out_j = sum_i w^(i j) P_i            inverse  out_j = (1 / m) sum_i w^(-i j) P_i
 * with m = 2^logm and w = Fr.w[logm], the root the Fr transform uses.
 *   points_lem  m affine LEM points, 64 B each; 64 zero bytes is the identity, allowed anywhere. Points
 *               are NOT validated (as for kgs_msm_points): a point off the curve or a coordinate >= q
 *               gives an unspecified result, never a fault.
 *   out_lem     m canonical affine LEM points (results compare byte for byte); may alias points_lem
 *   logm        0 .. 24; logm == 0 copies the point
 * ctx == NULL computes on the host (no GPU is touched). Failures: KGS_E_ARG for a logm out of range, a NULL
 * buffer, a context attached to a rank group (kgs_ctx_set_group) or with MSM sharding on
 * (kgs_ctx_set_shard). Same context contract as kgs_msm_points: the call holds the context's mutex, uses
 * device buffers of its own (sized from m), needs no SRS and leaves the resident SRS, the domain tables
 * and the prover's MSM work buffers as they are, and returns with nothing pending on the context's
 * streams, on its error paths too (kgs_ctx_idle). */
int kgs_g1_ntt(kgs_ctx_t* ctx, const uint8_t* points_lem, uint8_t* out_lem, int logm, int inverse);
/* Same with device pointers (on ctx's device; ctx must not be NULL). The input is only read, unless the
 * output aliases it, which is allowed. */
int kgs_g1_ntt_device(kgs_ctx_t* ctx, const void* d_points_lem, void* d_out_lem, int logm, int inverse);
/* The Lagrange-basis SRS [L_i(tau)]_1, i < 2^nbits, of the context's resident SRS: the inverse G1
 * transform of its first 2^nbits points (what snarkjs' "prepare phase 2" computes), so that
 * sum_i e_i [L_i(tau)]_1 commits to the polynomial with the evaluations e_i on the domain. The points are
 * read from the resident window table's first row, which holds 2^-256 P_i: the factor 2^256 is folded into
 * the inverse transform's final scaling (2^256 / n instead of 1 / n), so there is no extra pass over the
 * points and no second read of the ptau file. The result is cached on the device per (SRS, nbits), shared
 * by the contexts of that device, published once complete and released with the SRS tables; a second call
 * returns the cached points without running the transform.
 *   nbits    0 .. min(24, the nbits_max the SRS was loaded for)
 *   out_lem  2^nbits affine LEM points, or NULL: build and cache only
 * Failures: KGS_E_SRS "no SRS loaded"; KGS_E_ARG for an nbits out of range, a context attached to a rank
 * group or with MSM sharding on, an SRS loaded as a slice (kgs_srs_load_ptau_slice). Context contract as
 * for kgs_g1_ntt. */
int kgs_srs_lagrange(kgs_ctx_t* ctx, int nbits, uint8_t* out_lem);
/* Commitment from evaluations: out_lem = sum_i e_i [L_i(tau)]_1, i < 2^nbits, which is the point kgs_msm
 * gives for the coefficient form of e (kgs_fr_to_mont, inverse kgs_ntt, kgs_msm), byte for byte, without
 * computing the coefficients: the variable-base Pippenger of kgs_msm_points over the cached Lagrange
 * bases (built on first use, kgs_srs_lagrange), which drops zero digits, so small evaluations stay cheap.
 *   evals_std  2^nbits x 32 B little-endian STANDARD form; any 256-bit integer, taken mod r
 *   out_lem    affine LEM; all-zero evaluations give 64 zero bytes
 * Failures and context contract as for kgs_srs_lagrange; a NULL buffer is KGS_E_ARG. */
int kgs_commit_evals(kgs_ctx_t* ctx, const uint8_t* evals_std, int nbits, uint8_t out_lem[64]);
/* Same with a device pointer (on ctx's device), read only. */
int kgs_commit_evals_device(kgs_ctx_t* ctx, const void* d_evals_std, int nbits, uint8_t out_lem[64]);
/* One scalar per point: out_lem[i] = s_i * P_i for i < n (the pointwise step of kgs_kzg_open_all as a
 * primitive): per lane a signed-digit double-and-add, then one batched affine conversion.
 *   points_lem   n affine LEM points as kgs_msm_points takes them: 64 zero bytes is the identity, points are
 *                NOT validated (an unspecified result for a point off the curve, never a fault)
 *   scalars_std  n x 32 B little-endian STANDARD form; any 256-bit integer, taken mod r
 *   n            0 .. 2^26
 *   out_lem      n canonical affine LEM points; an identity in or a scalar that is 0 mod r gives 64 zero
 *                bytes. May alias points_lem.
 * ctx == NULL computes on the host (no GPU is touched). Failures: KGS_E_ARG for an n above the limit, a NULL
 * buffer with n > 0, a context attached to a rank group or with MSM sharding on. Context contract as for
 * kgs_g1_ntt: own device buffers, no SRS, nothing of the prover's touched, idle on return. */
int kgs_g1_mul_each(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t n, uint8_t* out_lem);
/* Same with device pointers (on ctx's device; ctx must not be NULL). The inputs are only read, unless the
 * output aliases the points, which is allowed. */
int kgs_g1_mul_each_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t n,
                           void* d_out_lem);
/* One KZG opening over the resident SRS: y = p(z) and proof = [(p(X) - y) / (X - z)](tau) for the polynomial
 * with the `len` coefficients coef_mont (32 B Montgomery each, as kgs_poly_eval takes them; len == 0: the
 * zero polynomial), z any element of Fr. It composes what the rounds launch: the Horner tiles of
 * kgs_poly_eval, the synthetic division of kgs_poly_div_x_sub (whose quotient does not depend on p's
 * constant term) and kgs_msm over the len - 1 quotient coefficients; it adds no kernel. proof_lem: affine
 * LEM, 64 zero bytes for a constant polynomial.
 * Failures: KGS_E_SRS "no SRS loaded", or len - 1 above the resident points; KGS_E_ARG for a NULL argument, a
 * context attached to a rank group or with MSM sharding on, an SRS loaded as a slice. The call holds the
 * context's mutex and returns with nothing pending on its streams, on its error paths too. */
int kgs_kzg_open(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t z_mont[32], uint8_t y_mont[32],
                 uint8_t proof_lem[64]);
/* All n = 2^nbits openings of one polynomial on its domain in O(n log n) group operations (Feist-Khovratovich;
 * DESIGN.md §19): proofs_lem[i] is the proof kgs_kzg_open gives at z = Fr.w[nbits]^i, byte for byte. The
 * quotient commitments are a Toeplitz product of the coefficients with the SRS, computed as one cyclic
 * convolution of size 2n over G1: a forward Fr transform of the zero-padded coefficients, one scalar
 * multiplication per point against the transform of the SRS side, an unscaled inverse G1 transform of size 2n
 * and a forward one of size n. The SRS side is read off the resident window table's first row (as
 * kgs_srs_lagrange does, no second read of the ptau file), transformed once per (SRS, nbits) and cached on
 * the device under the rules of the Lagrange row: shared by the contexts of the device, published once
 * complete, released with the SRS tables (128 B x 2^nbits).
 *   coef_mont   len <= 2^nbits coefficients, 32 B Montgomery each (the rest are zero; len == 0 gives n
 *               identities and zero evaluations)
 *   nbits       0 .. min(23, the nbits_max the SRS was loaded for)
 *   proofs_lem  2^nbits canonical affine LEM points, the identity as 64 zero bytes
 *   evals_mont  NULL, or 2^nbits x 32 B that receive p(w^i): one more Fr transform of size n
 * Failures: KGS_E_SRS "no SRS loaded"; KGS_E_ARG for an nbits out of range, len > 2^nbits, a NULL buffer with
 * work to do, a context attached to a rank group or with MSM sharding on, an SRS loaded as a slice. Unlike
 * kgs_g1_ntt this call, like kgs_ntt, may grow the device's shared domain tables (to 2^(nbits + 1)); the
 * window tables, the Lagrange cache and the prover's MSM work buffers stay as they are. The call holds the
 * context's mutex, uses device buffers of its own and returns with nothing pending on the context's
 * streams, on its error paths too (kgs_ctx_idle). */
int kgs_kzg_open_all(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, int nbits, uint8_t* proofs_lem,
                     uint8_t* evals_mont);
/* Same with device pointers (on ctx's device); d_coef_mont is only read. */
int kgs_kzg_open_all_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, void* d_proofs_lem,
                            void* d_evals_mont);
/* Host only (no GPU, no context): the check of one opening, e(proof, [tau]_2) == e(C - y G + z proof, [1]_2).
 * Returns 1 valid, 0 invalid (which includes a commitment or proof that is no canonical point of the curve
 * and a z or y that is not below r), KGS_E_ARG for a NULL argument or a tau_g2 off its curve. */
int kgs_kzg_verify(const uint8_t commit_lem[64], const uint8_t z_mont[32], const uint8_t y_mont[32],
                   const uint8_t proof_lem[64], const uint8_t tau_g2[128]);
/* Column sums of per-point products: out_lem[i] = sum_{r < rows} s_{r cols + i} * P_{r cols + i} for i < cols
 * (the pointwise step of kgs_kzg_open_cosets as a primitive): signed-digit double-and-add, from
 * 2^17 terms on with two rows of a column per lane sharing their doublings, the rows summed in extended coordinates
 * (equal, opposite and identity terms are summed correctly), one batched affine conversion of cols points.
 *   points_lem   rows * cols affine LEM points, row after row; 64 zero bytes is the identity; NOT validated
 *   scalars_std  rows * cols x 32 B little-endian STANDARD form; any 256-bit integer, taken mod r
 *   rows, cols   rows >= 1 (any integer), rows * cols <= 2^26; cols == 0 does nothing
 *   out_lem      cols canonical affine LEM points (64 zero bytes for the identity); must not overlap the inputs
 * ctx == NULL computes on the host (no GPU is touched). Failures: KGS_E_ARG for rows == 0, more than 2^26
 * terms, a NULL buffer with cols > 0, a context attached to a rank group or with MSM sharding on. Context
 * contract as for kgs_g1_mul_each: own device buffers (128 B per term), no SRS, nothing of the prover's
 * touched, idle on return, on error paths too. */
int kgs_g1_mul_sum(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t rows, uint64_t cols,
                   uint8_t* out_lem);
/* Same with device pointers (on ctx's device; ctx must not be NULL). The inputs are only read. */
int kgs_g1_mul_sum_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t rows,
                          uint64_t cols, void* d_out_lem);
/* Every coset opening of one polynomial at once. With n = 2^nbits, l = 2^lbits, m = n / l and
 * w = Fr.w[nbits], coset i < m is H_i = { w^(i + m j) : j < l }, the zeros of X^l - a_i with a_i = w^(i l), and
 * proofs_lem[i] = [q_i(tau)]_1 for p = q_i (X^l - a_i) + I_i, deg I_i < l: one 64 B proof for the l values
 * p(w^(i + m j)) = evals[i + m j]. lbits = 0 is kgs_kzg_open_all (same bytes); lbits = nbits gives one
 * identity. The Toeplitz product of kgs_kzg_open_all splits into l products of size m over the stride-l
 * subsequences of the coefficients and of the SRS: l zero-padded Fr transforms of size 2m, one multiply-sum
 * pass of 2n terms into 2m points (kgs_g1_mul_sum), ONE unscaled inverse G1 transform of size 2m and a
 * forward one of size m. The SRS side (the l G1 transforms of size 2m, scaled by 1 / 2m, 128 B x 2^nbits) is
 * built as one partial transform of size 2n on first use and cached per (SRS, nbits, lbits) under the rules
 * of kgs_kzg_open_all's row.
 *   coef_mont   len <= 2^nbits coefficients, 32 B Montgomery each (len == 0: identities and zero evaluations)
 *   nbits       0 .. min(23, the nbits_max the SRS was loaded for);  lbits  0 .. nbits
 *   proofs_lem  2^(nbits - lbits) canonical affine LEM points, the identity as 64 zero bytes
 *   evals_mont  NULL, or 2^nbits x 32 B that receive p(w^k) in natural order, as kgs_kzg_open_all gives them
 * Failures, context contract and what the call may grow: as for kgs_kzg_open_all (KGS_E_SRS "no SRS loaded";
 * KGS_E_ARG for nbits or lbits out of range, len > 2^nbits, a NULL buffer with work to do, a rank group, MSM
 * sharding, an SRS slice). It leaves kgs_kzg_open_all's rows and the Lagrange cache as they are. */
int kgs_kzg_open_cosets(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, int nbits, int lbits, uint8_t* proofs_lem,
                        uint8_t* evals_mont);
/* Same with device pointers (on ctx's device); d_coef_mont is only read. */
int kgs_kzg_open_cosets_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int lbits,
                               void* d_proofs_lem, void* d_evals_mont);
/* 1 when the SRS side of kgs_kzg_open_cosets for (nbits, lbits) is cached on the device for ctx's SRS (lbits
 * = 0: kgs_kzg_open_all's row), else 0: such a call builds nothing. No GPU work. */
int kgs_kzg_open_cosets_cached(kgs_ctx_t* ctx, int nbits, int lbits);
/* kgs_kzg_open_cosets for `polys` polynomials over one (nbits, lbits) and one SRS, every stage launched once for
 * the whole set: one layout kernel and one batched Fr transform for the polys * l coefficient rows,
 * one multiply-sum pass of polys * 2n terms against the l cached rows, and the two G1 transforms as batched
 * stages that give a wave one twiddle across polynomials and groups. A transform of 128 points costs a single
 * call as much time as one of thousands; here the polynomials share those stages.
 *   coef_mont   polynomial b has its len <= 2^nbits Montgomery coefficients at coef_mont + 32 * stride * b;
 *               stride >= len, and what lies between len and stride is not read
 *   polys       polys * 2^nbits <= 2^24; polys == 0 does nothing and returns KGS_OK
 *   nbits, lbits  as for kgs_kzg_open_cosets
 *   proofs_lem  polys * 2^(nbits - lbits) canonical affine LEM points, polynomial after polynomial
 *   evals_mont  NULL, or polys * 2^nbits x 32 B, polynomial after polynomial, each in natural order
 * Results: the bytes kgs_kzg_open_cosets gives for polynomial b alone, at every lbits 0 .. nbits, for len == 0 and
 * for one coset (lbits == nbits). lbits == 0 runs kgs_kzg_open_all's path polynomial after polynomial: it has no
 * rows to share a multiply-sum pass over. The SRS side is kgs_kzg_open_cosets' cached row of (SRS, nbits, lbits):
 * either call builds it for the other, and kgs_kzg_open_cosets_cached reports it.
 * Failures: KGS_E_SRS "no SRS loaded"; KGS_E_ARG (the message names the offender) for a NULL ctx, a NULL buffer
 * with work to do, stride < len, len > 2^nbits, polys * 2^nbits > 2^24, nbits or lbits out of range, a rank group,
 * MSM sharding, an SRS slice. Context contract as for kgs_kzg_open_cosets: device buffers of the call's own
 * ("km_*", about 450 B per coefficient slot polys * 2^nbits), nothing of the prover's, of the window tables or of
 * the other caches touched, idle on return, on error paths too. */
int kgs_kzg_open_cosets_many(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t polys, uint64_t stride, uint64_t len,
                             int nbits, int lbits, uint8_t* proofs_lem, uint8_t* evals_mont);
/* Same with device pointers (on ctx's device); d_coef_mont is only read. */
int kgs_kzg_open_cosets_many_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t polys, uint64_t stride,
                                    uint64_t len, int nbits, int lbits, void* d_proofs_lem, void* d_evals_mont);
/* Host only (no GPU, no context): the check of one coset opening of kgs_kzg_open_cosets,
 * e(-proof, [tau^l]_2) e(C - [I(tau)]_1 + a_i proof, [1]_2) == 1, where I interpolates the l values
 * ys_mont[j] = p(w^(index + m j)): I = sum_k d_k X^k with d_k = w^(-index k) J_k and J the inverse transform
 * of size l of the values (kgs_ntt's convention); [I(tau)]_1 is the host sum of kgs_msm_points over
 * srs_g1_lem, the first l points [tau^k]_1 of the SRS (affine LEM). nbits 0 .. 28, lbits 0 .. nbits,
 * index < 2^(nbits - lbits). Returns 1 valid, 0 invalid (which includes a commitment, proof or SRS point
 * that is no canonical point of the curve and a value that is not below r), KGS_E_ARG for a NULL argument,
 * a range error or a tau_l_g2 off its curve. */
int kgs_kzg_verify_coset(const uint8_t commit_lem[64], int nbits, int lbits, uint64_t index, const uint8_t* ys_mont,
                         const uint8_t proof_lem[64], const uint8_t* srs_g1_lem, const uint8_t tau_l_g2[128]);

/* ---- batch verifier for coset openings: many (commitment, coset, values, proof) tuples against one SRS, one
 * pairing check. Notation as for kgs_kzg_open_cosets: n = 2^nbits, l = 2^lbits, m = n / l,
 * w = Fr.w[nbits], a_i = w^(i l). Opening k < count is (commitment c(k) = commit_of[k], coset i_k = index[k], the
 * l values y_k = ys_mont[k l .. k l + l), proof pi_k). Every opening's equation is linear in G1, so under weights
 * w_k = rho^k the batch is accepted iff
 *   e(-A, [tau^l]_2) * e(B, [1]_2) == 1
 *   A = sum_k w_k pi_k
 *   B = sum_k w_k C_c(k) + sum_k (w_k a_{i_k}) pi_k - [D(tau)]_1
 *   D = sum_k w_k I_k, that is D_j = sum_k w_k w^(-i_k j) J_{k,j} for j < l, J_k the inverse transform of size l of
 *       y_k in kgs_ntt's convention: the interpolant kgs_kzg_verify_coset builds (kgs_coset_interp_fold below)
 * With count == 1 (rho^0 = 1) this is kgs_kzg_verify_coset's equation, and the verdict is the same.
 *
 * Weights (deterministic; LE32 / LE64 = 4 / 8 bytes little-endian)
 *   seed = seed32 if it is given, else keccak256("kgs-verify-cosets-batch-v1" || tau_l_g2 (128 B) || LE32(nbits) ||
 *          LE32(lbits) || LE64(ncommits) || commits || LE64(count) || commit_of (LE32 each) || index (LE64 each) ||
 *          ys || proofs)
 *   rho  = keccak256("kgs-verify-cosets-batch-v1/rho" || seed) read as a little-endian integer mod r; 0 -> 1
 *   w_k  = rho^k
 * A caller's seed32 saves hashing count * l * 32 bytes on one host thread; it MUST be unpredictable to whoever
 * made the proofs (fresh randomness drawn after the batch is fixed, or a hash that covers all of it).
 * Soundness: the pairing residues of the openings are fixed before rho is (the seed hashes everything the check
 * depends on, or is drawn afterwards). If some opening fails its own equation, the batch equation is a nonzero
 * polynomial of degree < count in rho, so in the random-oracle model a batch holding an invalid opening passes
 * the aggregate check with probability at most count / r < 2^-227 for count <= 2^26.
 *
 * Structural checks, as in the single check: an opening whose proof or commitment is no canonical point of the
 * curve, with a value >= r, an index >= m or a commit_of >= ncommits is marked invalid before the aggregate
 * check and enters it with weight 0. An SRS point off the curve makes every opening invalid (returns 0).
 *
 * Returns 1 if every opening is valid, 0 if some opening is invalid, a negative KGS_E_* for an error. With
 * valid_out == NULL only that verdict is computed. With valid_out (count bytes, 1 valid / 0 invalid) a failing
 * batch is bisected over contiguous index ranges: under a failing parent the left half is checked; if it passes
 * the right half is known to fail and is not checked. With b invalid openings that is at most
 * 1 + 2 b ceil(log2 count) checks. A sub-range is folded again, with the same weights; on the GPU path the inputs
 * stay on the device between the checks.
 *   nbits, lbits  with a context nbits 0 .. 23 (what the shared domain tables cover), on the host 0 .. 28;
 *                 lbits 0 .. nbits; with a context count * l <= 2^26. On the GPU the fold covers lbits <= 10:
 *                 a batch of larger cosets folds on the host (the _device twin answers KGS_E_ARG)
 *   commits_lem   ncommits affine LEM commitments (64 B); one commitment may serve many openings
 *   commit_of     count indices into commits_lem;   index  count coset indices
 *   ys_mont       count * l values, 32 B Montgomery, the rows contiguous;   proofs_lem  count x 64 B affine LEM
 *   srs_g1_lem    the first l points [tau^k]_1 (affine LEM);   tau_l_g2  [tau^l]_2 (kgs_ptau_read_tau_g2_pow)
 *   seed32        NULL, or 32 bytes (see above)
 * KGS_E_ARG: a NULL buffer with work to do, nbits / lbits / count out of range, a tau_l_g2 off its curve, a
 * context attached to a rank group or with MSM sharding on. count == 0 returns 1 and touches nothing.
 * ctx == NULL computes everything on the host (no GPU is touched). With a context a batch of fewer than 24 terms
 * (3 count + l; the measured crossover) folds on the host as well, and diag->on_gpu tells which
 * path ran; the environment variable KGS_VERIFY_COSETS_FOLD = "gpu" | "host" forces either. On the GPU path the
 * on-curve checks (k_g1_on_curve), the range checks (inside the interpolation kernel), the weights, D and the
 * terms of A and B are computed on the device, and A and B are summed there by kgs_msm_points' buckets
 * (KGS_VERIFY_COSETS_MSM = "fold" runs kgs_g1_lincomb's fold instead: slower at every size, kept for the A/B);
 * the host does the hash, the pairing checks and the bisection. Context contract as for kgs_g1_mul_sum and kgs_kzg_open_cosets: device
 * buffers of the call's own; the window tables, the Lagrange cache, the fk rows and the prover's work buffers
 * are untouched; the domain tables may grow to 2^nbits; the context is idle on return, on error paths too. */
typedef struct {            /* optional; every pointer member optional (NULL: not wanted) */
  uint8_t* rho_out;         /* in: 32 B, receives rho in standard form LE */
  uint8_t* folded_out;      /* in: 128 B, receives A || B (affine LEM) of the first (whole-batch) check */
  uint8_t* interp_out;      /* in: l x 32 B, receives D (Montgomery) of the first check */
  uint32_t pairing_checks;  /* out: 2-pair pairing checks performed */
  int on_gpu;               /* out: 1 if the folds ran on the GPU */
  double hash_ms, fold_ms, pairing_ms; /* out: wall clock of the seed and rho, of all folds (structural checks
                                          and transfers included), of all pairing checks */
} kgs_coset_batch_diag_t;
int kgs_kzg_verify_cosets_batch(kgs_ctx_t* ctx, int nbits, int lbits, const uint8_t* commits_lem, uint64_t ncommits,
                                const uint32_t* commit_of, const uint64_t* index, const uint8_t* ys_mont,
                                const uint8_t* proofs_lem, uint64_t count, const uint8_t* srs_g1_lem,
                                const uint8_t tau_l_g2[128], const uint8_t* seed32, uint8_t* valid_out,
                                kgs_coset_batch_diag_t* diag);
/* Same with d_commit_of, d_index, d_ys_mont and d_proofs_lem device pointers (on ctx's device, only read; e.g.
 * kgs_kzg_open_cosets_device's outputs). commits_lem, srs_g1_lem, tau_l_g2, valid_out and diag stay host
 * pointers. ctx and seed32 must not be NULL (the seed is not derived from device memory); the folds always run
 * on the GPU. */
int kgs_kzg_verify_cosets_batch_device(kgs_ctx_t* ctx, int nbits, int lbits, const uint8_t* commits_lem,
                                       uint64_t ncommits, const void* d_commit_of, const void* d_index,
                                       const void* d_ys_mont, const void* d_proofs_lem, uint64_t count,
                                       const uint8_t* srs_g1_lem, const uint8_t tau_l_g2[128], const uint8_t* seed32,
                                       uint8_t* valid_out, kgs_coset_batch_diag_t* diag);
/* The weighted sum of interpolants on its own: out_mont[j] = sum_{k < count} weights[k] * w^(-index[k] j) * J_{k,j},
 * j < l, with J_k the inverse transform of size l of row k of ys_mont (kgs_ntt's convention, 1 / l included); with
 * count == 1 and weight one this is the coefficient vector of kgs_kzg_verify_coset's I. A row of weight zero is not
 * read. weights_mont: count x 32 B Montgomery. nbits / lbits / count ranges as above; with a context lbits <= 10
 * (one fused kernel, coset_fold.hip k_coset_interp_fold; larger l: KGS_E_ARG), ctx == NULL computes on the host.
 * KGS_E_ARG also for a NULL buffer with work to do, an index >= m, a weight or (in a row of nonzero weight) a value
 * >= r, a rank group, MSM sharding. count == 0 gives zeros. Context contract as above. */
int kgs_coset_interp_fold(kgs_ctx_t* ctx, int nbits, int lbits, const uint64_t* index, const uint8_t* ys_mont,
                          const uint8_t* weights_mont, uint64_t count, uint8_t* out_mont /* l x 32 B */);
/* Same with device pointers (on ctx's device; ctx must not be NULL). The inputs are only read. */
int kgs_coset_interp_fold_device(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                 const void* d_weights_mont, uint64_t count, void* d_out_mont);
/* ---- recovery: a polynomial of known length back from a subset of its cosets. Notation as for
 * kgs_kzg_open_cosets: n = 2^nbits, l = 2^lbits, m = n / l, w = Fr.w[nbits], coset i < m is { w^(i + m j) : j < l }.
 * Row k < count of ys_mont holds the l values y_{k,j} = p(w^(index[k] + m j)) (kgs_kzg_verify_cosets_batch's rows);
 * the indices are distinct, in any order. With count l >= len there is at most one p of degree < len through
 * those values:
 *   returns 1  it exists: coef_mont receives its len coefficients, and evals_mont (if not NULL) all n values p(w^k)
 *              in natural order, as kgs_kzg_open_cosets' evals_mont holds them
 *   returns 0  the values lie on no polynomial of degree < len; the outputs are unspecified
 * Fr only: no SRS, no G1, no pairing; a context with no SRS loaded serves. With Z the vanishing polynomial of the
 * missing cosets (a polynomial in X^l, built as a product tree on the device): three transforms of size n (E Z to
 * coefficients, onto the coset g <w>, back after the division by Z there), two of size m and m inversions.
 *   nbits  0 .. 23;  lbits  0 .. nbits;  len  1 .. n;  count  ceil(len / l) .. m
 *   index  count coset indices < m;  ys_mont  count x l x 32 B Montgomery, canonical;  both only read
 * KGS_E_ARG (kgs_last_error names the first offender where there is one): ctx == NULL (there is no host path; no
 * GPU is touched), a NULL index, ys_mont or coef_mont, nbits / lbits / len / count out of range, an index >= m, an
 * index given twice, a value >= r, a rank group, MSM sharding. Context contract as for kgs_kzg_open_cosets: device
 * work buffers of the call's own ("rc_*"), the shared domain tables may grow to 2^nbits; the window tables, the
 * Lagrange, kgs_kzg_open_all and kgs_kzg_open_cosets caches and the prover's buffers are not touched; the context
 * is idle on return, on error paths too. */
int kgs_kzg_recover_cosets(kgs_ctx_t* ctx, int nbits, int lbits, const uint64_t* index, const uint8_t* ys_mont,
                           uint64_t count, uint64_t len, uint8_t* coef_mont /* len x 32 B */,
                           uint8_t* evals_mont /* NULL or 2^nbits x 32 B */);
/* Same with device pointers (on ctx's device) for index, ys, coef and evals. */
int kgs_kzg_recover_cosets_device(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                  uint64_t count, uint64_t len, void* d_coef_mont, void* d_evals_mont);
/* ---- recovery of many polynomials in one call. `polys` polynomials of `len` coefficients each, over
 * one domain (notation above). The cells arrive as kgs_kzg_verify_cosets_batch takes them: cell k < count belongs to
 * polynomial poly_of[k] < polys (commit_of's type and role), names coset index[k] < m, and row k of ys_mont holds its
 * l values. Cells come in any order and every polynomial has its own set of cosets. The outputs are laid out as
 * kgs_kzg_open_cosets_many's input: coef_mont + 32 stride b receives the len coefficients of polynomial b (stride >=
 * len; the gap between len and stride is not written), evals_mont (if not NULL) its n values p_b(w^k) at
 * 32 n b, and status_out (if not NULL) one byte per polynomial:
 *   1  recovered
 *   0  its cells lie on no polynomial of degree < len
 *   2  it has fewer than ceil(len / l) cells, possibly none: nothing can be said
 * For status 0 and 2 that polynomial's outputs are unspecified; every other polynomial's are unaffected. For status 0
 * and 1 the verdict and every byte equal what kgs_kzg_recover_cosets gives for that polynomial's cells alone.
 * Returns 1 when every status is 1, else 0 (the same with status_out == NULL). polys == 0 does nothing and returns 1
 * (after the NULL-ctx refusal no other argument is looked at then, the context's state included);
 * count == 0 gives status 2 everywhere. Every stage is launched once for all the polynomials, over arrays of polys
 * rounded up to a power of two blocks (at most twice the memory): the product trees are the levels of one array
 * stopped at degree m, the transforms run block by block in one launch sequence.
 *   nbits  0 .. 23;  lbits  0 .. nbits;  len  1 .. n;  polys n <= 2^24;  count <= polys m;  stride >= len
 *   poly_of  count x uint32;  index  count x uint64;  ys_mont  count x l x 32 B Montgomery, canonical;  all only read
 * KGS_E_ARG (kgs_last_error names the first offender where there is one): ctx == NULL (there is no host path; no GPU
 * is touched), a NULL coef_mont, a NULL poly_of, index or ys_mont with count > 0, nbits / lbits / len / polys / count
 * out of range, stride < len, a rank group, MSM sharding; and, found on the device, the lowest cell with poly_of >=
 * polys or index >= m, the lowest cell that names a (polynomial, coset) pair a second time, the lowest value (cell, j)
 * that is not below r. Context contract as for kgs_kzg_recover_cosets, with work buffers of the call's own ("rcm_*"):
 * the single call's "rc_*" buffers are not touched either. */
int kgs_kzg_recover_cosets_many(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const uint32_t* poly_of,
                                const uint64_t* index, const uint8_t* ys_mont, uint64_t count, uint64_t len,
                                uint64_t stride, uint8_t* coef_mont /* polys x stride x 32 B */,
                                uint8_t* evals_mont /* NULL or polys x 2^nbits x 32 B */,
                                uint8_t* status_out /* NULL or polys B */);
/* Same with device pointers (on ctx's device) for poly_of, index, ys, coef and evals; status_out stays a host
 * pointer. */
int kgs_kzg_recover_cosets_many_device(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const void* d_poly_of,
                                       const void* d_index, const void* d_ys_mont, uint64_t count, uint64_t len,
                                       uint64_t stride, void* d_coef_mont, void* d_evals_mont, uint8_t* status_out);
/* Keccak-256 (js-sha3 keccak256) */
int kgs_keccak256(const uint8_t* data, uint64_t len, uint8_t out[32]);

/* ---- device timing helpers for bench.py (events recorded on ctx's stream) ---- */
/* Run `reps` MSMs of n scalars (device pointer) back to back; returns total ms on the stream. */
int kgs_bench_msm(kgs_ctx_t* ctx, const void* d_scalars_mont, uint64_t n, int reps, double* ms);
/* Run `reps` MSMs of n scalars, accumulating per-phase device time (ms) into phase_ms[4]:
 * [0] digit recoding + counting sort, [1] bucket accumulation (the k_accumulate launch alone),
 * [2] bucket combine, [3] bit-sum reduction. *entries = nonzero (bucket, point) entries of the last run. */
int kgs_bench_msm_phases(kgs_ctx_t* ctx, const void* d_scalars_mont, uint64_t n, int reps, double* phase_ms,
                         uint64_t* entries);
/* Run `reps` forward+inverse NTT pairs of size 2^logm on a device buffer; returns ms. */
int kgs_bench_ntt(kgs_ctx_t* ctx, void* d_buf, int logm, int reps, double* ms);
/* `reps` runs (after one warm-up) of a G1 transform leg of size 2^logm (1 .. 24) on device buffers, each
 * between two events on ctx's stream: ms[r] = run r. what: 0 the forward transform, 1 the inverse, 2 the
 * scaling pass alone (2^logm multiplications by one launch-uniform 254-bit constant and their affine
 * conversion: the rate of a wave-uniform double-and-add, as k_tab_scale's). mapping: 0 the library's
 * thread mapping, 1 one twiddle per lane, 2 one per wave wherever a stage has 64 groups. */
int kgs_bench_g1_ntt(kgs_ctx_t* ctx, const void* d_in, void* d_out, int logm, int what, int mapping, int reps,
                     double* ms);
/* `reps` runs of a leg of kgs_kzg_open_all_device for the 1 <= len <= 2^nbits device-resident coefficients,
 * each between two events on ctx's stream, after one whole call (which builds and caches the SRS side):
 * ms[r] = run r. what: 0 the call with the cache warm, 1 the build of the cached SRS side (not published),
 * 2 the pointwise pass alone (2^(nbits + 1) per-lane multiplications and their affine conversion). */
int kgs_bench_kzg_open_all(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int what, int reps,
                           double* ms);
/* `reps` runs of a leg of kgs_kzg_open_cosets_device (1 <= lbits < nbits, 1 <= len <= 2^nbits), as
 * kgs_bench_kzg_open_all times its own. what: 0 the call with the cache warm, 1 the build of the cached rows
 * (the partial transform and its scaling, not published), 2 the multiply-sum pass alone (2^(nbits + 1) terms
 * into 2m points and their affine conversion), 3 the two G1 transforms alone (the inverse of size 2m and the
 * forward of size m, over the call's own u and h), 4 kgs_g1_mul_each's kernel over the same 2^(nbits + 1)
 * terms, no sum and no conversion; 5 the multiply-sum pass with one row per lane (that kernel, then the column
 * sums: the other arm of the A/B of DESIGN.md §20; what 2 runs the pass as it ships, two rows per lane). */
int kgs_bench_kzg_open_cosets(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int lbits, int what,
                              int reps, double* ms);
/* `reps` runs of a leg of kgs_kzg_open_cosets_many_device (1 <= lbits < nbits, 1 <= len <= stride, polys >= 1), as
 * kgs_bench_kzg_open_cosets times its own: after one whole call, each between two events on ctx's stream. what:
 * 0 the call with the cache warm, 1 the Fr side (layout, batched transform, bit reversal), 2 the multiply-sum pass
 * and its affine conversion, 3 the two batched G1 transforms and the slice between them, 4 the same with the
 * per-lane mapping forced in every stage (the other arm of the A/B of DESIGN.md §23), 5 the yardstick: polys runs
 * of kgs_kzg_open_cosets_device's work, one polynomial after the other, enqueued back to back. */
int kgs_bench_kzg_open_cosets_many(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t polys, uint64_t stride, uint64_t len,
                                   int nbits, int lbits, int what, int reps, double* ms);
/* The route kgs_commit_evals_device replaces, with the same device-resident input: to Montgomery form,
 * inverse NTT, kgs_msm over the resident window tables (profiles/g1_ntt_time.py times both by the wall
 * clock; each ends synchronised). */
int kgs_bench_coeff_commit(kgs_ctx_t* ctx, const void* d_evals_std, int nbits, uint8_t out_lem[64]);
/* `reps` runs (after one warm-up) of kgs_coset_interp_fold_device's two launches (k_coset_interp_fold and the
 * reduction of its partial sums) over device-resident inputs, each between two events on ctx's stream: ms[r] =
 * run r. count >= 1, lbits <= 10; the sum itself is discarded. */
int kgs_bench_coset_interp_fold(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                const void* d_weights_mont, uint64_t count, int reps, double* ms);
/* `reps` runs of a leg of kgs_kzg_recover_cosets_device over device-resident inputs (arguments and ranges as that
 * call's; d_coef_mont receives the coefficients), after one whole call, each between two events on ctx's stream:
 * ms[r] = run r. what: 0 the whole call without evaluations, 1 the marks and the product tree, 2 the m-sized side
 * (z's coefficients, its two transforms of size m, the batch inversion), 3 the three transforms of size n alone.
 * leaf_log: the tree's leaves cover 2^leaf_log cosets, 6 .. 9, or 0 for the library's choice. */
int kgs_bench_kzg_recover_cosets(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                 uint64_t count, uint64_t len, void* d_coef_mont, int what, int leaf_log, int reps,
                                 double* ms);
/* `reps` runs of a leg of kgs_kzg_recover_cosets_many_device over device-resident inputs (arguments and ranges as that
 * call's, polys >= 1; d_coef_mont receives the coefficients), after one whole call, each between two events on ctx's
 * stream: ms[r] = run r. what: 0 the whole call without evaluations, 1 the marks and the trees, 2 the m-sized side,
 * 3 the three block transforms of size n and the twist between them alone, 4 the yardstick: polys runs of
 * kgs_kzg_recover_cosets_device's work, one polynomial after the other, enqueued back to back without the per-call
 * drain. what 4 takes the cells grouped by ascending polynomial, ceil(len / l) .. m of them for each, and uses the
 * single call's "rc_*" buffers. */
int kgs_bench_kzg_recover_cosets_many(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const void* d_poly_of,
                                      const void* d_index, const void* d_ys_mont, uint64_t count, uint64_t len,
                                      uint64_t stride, void* d_coef_mont, int what, int reps, double* ms);
/* Host-only test hook of kgs_prove's staging copy (no GPU): copies len bytes src -> dst the way a
 * host input vector is staged (256 KiB pieces over the copy pool, spans of `span` bytes reported in
 * order once copied). spans_out[i] receives the byte offset of the i-th reported span (up to max);
 * fail_at >= 0 makes the report of span fail_at fail, the way a failed DMA enqueue does: the copy
 * then still completes and the call returns KGS_E_HIP. *nspans = spans reported. */
int kgs_test_stream_copy(uint8_t* dst, const uint8_t* src, uint64_t len, uint64_t span, int fail_at,
                         uint64_t* spans_out, int max, int* nspans);

#ifdef __cplusplus
}
#endif
#endif /* KGS_H */
