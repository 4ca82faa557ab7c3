// Launch wrappers for the gfx950 kernels (ntt.hip, poly.hip, msm.hip, lookup.hip, fold.hip, g1ntt.hip, coset_fold.hip, recover.hip). All pointers are device
// pointers to 32 B Montgomery Fr elements (uint32_t[8]) or 64 B affine / 128 B XYZZ G1 points,
// unless stated otherwise. Launches are asynchronous on `st`.
#pragma once

// Wave priority: every kernel except k_accumulate raises its waves to priority 3 (1 until round 5), so the
// short latency-bound kernels of the other in-flight proofs (NTT, sort, MSM tail, poly) win VALU arbitration
// against the long accumulate waves they share SIMDs with (arbitration is by priority, then age); the
// accumulate waves stay at 0, or step 2 -> 1 -> 0 with their progress (msm.hip, k_accumulate). A/B on
// MI355X, same box: 77.9 -> 80.5 proofs/s at n = 2^20 (4 in flight); single-proof latency 14.6 -> 14.9 ms.
// -DKGS_NO_PRIO_AUX disables.
#ifndef KGS_NO_PRIO_AUX
#define KGS_AUX_PRIO() __builtin_amdgcn_s_setprio(3)
#else
#define KGS_AUX_PRIO() ((void)0)
#endif

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "field.hpp"
#include "msm_sizes.hpp"

namespace kgs {

constexpr int LC_MAX = 32;
constexpr int LC_W29 = 10;  // words of a coefficient's 29-bit product record (fr29.hpp)
struct LinComb {  // out[i] = sum_k coef_k * src_k[i] (zero beyond len_k) + (i == 0 ? c0 : 0)
  int nterms;
  const uint32_t* src[LC_MAX];
  uint64_t len[LC_MAX];
  uint32_t coef[LC_MAX][8];
  uint32_t coef29[LC_MAX][LC_W29];  // coef_k as 29-bit records (prover.cpp fr29_record)
  uint32_t c0[8];
};

constexpr int EB_MAX = 32;
struct EvalBatch {
  int npolys;
  const uint32_t* src[EB_MAX];
  uint64_t len[EB_MAX];
};

struct MsmTables {
  uint32_t* table = nullptr;  // W x npts affine points (64 B)
  uint64_t npts = 0;
  int c = 0, W = 0;
  // Row 0 holds 2^-256 * P_i (mod r), so that the digits are read off the scalars' Montgomery words
  // (msm.hip scalar_digits). zero_points: some P_i is the zero point (found when the table is built);
  // a table without one runs the bucket accumulation without the affine-infinity test.
  bool zero_points = true;
};

// Work buffers of one MSM in flight, sized by msm_work_sizes (msm_sizes.hpp, with the bucket sort's
// msm_lob / msm_nh and the kernels' constants)
struct MsmWork {
  int32_t* digit = nullptr;  // reused as the partition-pass value array
  uint8_t* lo = nullptr;
  uint32_t* blockhist = nullptr;  // NH x ceil(N / (256 * SORT_SPT)) per-block partition counts
  uint32_t *counts = nullptr, *offsets = nullptr, *cursor = nullptr, *sorted = nullptr;
  uint32_t* part = nullptr;      // bucket row + column sums (2^h + 2^l run records, msm.hip k_rowcol)
  uint32_t* segowner = nullptr;  // bucket of each segment's first run
  uint32_t* locnt = nullptr;     // lo pass: NH partitions x 2^LOB lo x SL_G chunks counts / bases
  uint32_t* chunklist = nullptr; // combine levels: 3 lists of chunk-start segments
  uint32_t* chunkcnt = nullptr;  // their lengths
  uint32_t* raw29 = nullptr;     // accumulate output in the fq29 form (B + 1 + nseg entries x 160 B)
};

// ntt.hip
// NTT LDS passes built for three waves per SIMD (co-resident with two accumulate waves: proofs in
// flight) or two (fastest alone) for the calling thread's later launches; returns the previous setting
bool ntt_set_coresident(bool on);
constexpr int TW29_WORDS = 10;  // words per 29-bit twiddle record (fr29.hpp W29_WORDS)
// the 29-bit twin (fr29.hpp, k_tw29 records; record i <-> element i) of `count` 8 x 32 elements at
// `base`: the LDS passes of ntt_dif / ntt_dit multiply by the twin records of the twiddle table and
// the pre / post scalings they were given when every one of them lies in a registered table
void ntt_register_tw29(const uint32_t* base, uint64_t count, const uint32_t* twin);
void ntt_unregister_tw29(const uint32_t* base);
// out[i] = the k_tw29 record of in[i] (8 x 32 Montgomery words), i < count
void launch_tw29(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t count);
void ntt_dif(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t in_len, int logm, const uint32_t* pre,
             const uint32_t* tw, int logM);
void ntt_dit(hipStream_t st, uint32_t* out, const uint32_t* in, int in_bitrev, int logm, const uint32_t* tw, int logM,
             const uint32_t* post, const uint32_t* post_s);
// The 2^(logtotal - s) transforms of size 2^s (1 <= s <= logtotal) over the consecutive blocks of 2^s elements of
// `data` (2^logtotal elements), in place: the last s stages of ntt_dif / the first s stages of ntt_dit over the
// whole array, by the same passes. dif: natural in, bit-reversed out within each block; dit: bit-reversed in,
// natural out, every output times *post_s if given. tw: a stage table covering 2^s.
void ntt_dif_blocks(hipStream_t st, uint32_t* data, int logtotal, int s, const uint32_t* tw);
void ntt_dit_blocks(hipStream_t st, uint32_t* data, int logtotal, int s, const uint32_t* tw, const uint32_t* post_s);
void launch_powers(hipStream_t st, uint32_t* out, uint64_t count, const uint32_t* w_dev, const uint32_t* scale_dev);
void launch_scale_copy(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t n, const uint32_t* tab,
                       const uint32_t* sc);
void launch_bitrev_copy(hipStream_t st, uint32_t* out, const uint32_t* in, int logm);

// poly.hip
void launch_to_mont(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t n);
// device -> mapped pinned host memory by a small store kernel (bytes a multiple of 16)
void launch_host_store(hipStream_t st, void* dst_host_mapped, const void* src, uint64_t bytes, unsigned blocks);
void launch_lincomb(hipStream_t st, uint32_t* out, uint64_t n, const LinComb& lc);
void launch_builder(hipStream_t st, bool prod, bool sel, uint32_t* out, const uint32_t* f, const uint32_t* t,
                    const uint32_t* sf, const uint32_t* stt, const uint32_t* gamma, uint64_t n, uint32_t* scratch_tp,
                    uint32_t* scratch_ti, uint32_t* flag);
void launch_quotient(hipStream_t st, bool prod, bool sel, uint32_t* q, const uint32_t* S, const uint32_t* F,
                     const uint32_t* T, const uint32_t* SF, const uint32_t* ST, const uint32_t* inv_nxm1,
                     const uint32_t* scalars, int lcs, uint32_t rot);
// The quotient of a multi-argument proof (prover_rounds.cpp): up to QM_MAX arguments per launch share the
// coset point, the Z_H and L1 factors and the store. Argument j contributes delta^j times its numerator.
constexpr int QM_MAX = 8;
struct QuotArg {
  const uint32_t *S, *F, *T, *SF, *ST;  // coset evaluations, bit-reversed (SF / ST: selected only)
  int prod, sel, lookup;                // grand-product / selected / no selT-binary term
  uint32_t delta[8];                    // delta^j
  uint32_t delta29[LC_W29];             // delta^j as a 29-bit record (prover.cpp fr29_record)
};
struct QuotMulti {
  int nargs;
  int accumulate;  // add to q instead of overwriting it (the launches after the first of m > QM_MAX)
  QuotArg a[QM_MAX];
};
// q[p] (+)= (alpha / Z_H)(x_p) * sum_j delta^j core_j(x_p) + inv_nxm1[p] * sum_j delta^j l1op_j(x_p), with core_j /
// l1op_j what launch_quotient computes for argument j alone; scalars, lcs, rot as for launch_quotient
void launch_quotient_multi(hipStream_t st, uint32_t* q, const QuotMulti& qm, const uint32_t* inv_nxm1,
                           const uint32_t* scalars, int lcs, uint32_t rot);
void launch_divcheck(hipStream_t st, bool prod, bool sel, uint32_t* flag, const uint32_t* S, const uint32_t* f,
                     const uint32_t* t, const uint32_t* sf, const uint32_t* stt, const uint32_t* scalars, uint64_t n,
                     const uint32_t* S_next = nullptr, uint64_t gbase = 0);
void launch_eval_tiles(hipStream_t st, uint32_t* part, const EvalBatch& eb, const uint32_t* xp, uint32_t ntiles_max);
void launch_divide(hipStream_t st, uint32_t* q, uint32_t* flag, const uint32_t* a, uint64_t L, const uint32_t* xp,
                   uint32_t* part, uint32_t* carry);
void launch_fr_batch_inv(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t n);
void launch_from_mont(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t n);
void launch_nxm1(hipStream_t st, uint32_t* out, const uint32_t* tw, uint64_t halfM, const uint32_t* gp,
                 const uint32_t* np, int lcs, uint64_t wstride);
constexpr uint64_t EVAL_TILE = 2048;
// reference-quirks mode (prover.cpp ref_quirks_*): degree, the reference's multiply/shiftOmega
// pointwise step on its own evaluation domains, divZh in place
void launch_degree(hipStream_t st, uint32_t* out, const uint32_t* a, uint64_t len);
void launch_ref_gather_mul(hipStream_t st, uint32_t* out, const uint32_t* a, int loga, const uint32_t* b, int logb,
                           uint64_t N, uint64_t rot);
void launch_ref_divzh(hipStream_t st, uint32_t* c, uint64_t n, uint32_t ext, uint32_t* flag);

// dist.hip (the distributed prover's rank-local kernels; layouts in prover_dist.cpp)
void launch_gather_e(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t N, int W, int r, bool to_mont);
void launch_dfwd_pack(hipStream_t st, uint32_t* send, const uint32_t* Z, int logMl, int W, int r, const uint32_t* tw,
                      int logN);
void launch_dfwd_wdft(hipStream_t st, uint32_t* out, const uint32_t* recv, int logMl, int W, const uint32_t* tw, int logN);
void launch_dinv_wdft_pack(hipStream_t st, uint32_t* send, const uint32_t* loc, int logMl, int W, int r,
                           const uint32_t* tw_inv, int logN);
void launch_unpack_c2b(hipStream_t st, uint32_t* out, const uint32_t* recv, uint64_t Lb, int W);
void launch_pack_b2c(hipStream_t st, uint32_t* send, const uint32_t* blk, uint64_t Lb, int W);
void launch_scan_fix(hipStream_t st, bool prod, uint32_t* out, const uint32_t* off, uint64_t n);
void launch_e_heads(hipStream_t st, uint32_t* heads, const uint32_t* S, uint64_t Ml, int W, int rot);
void launch_quotient_e(hipStream_t st, bool prod, bool sel, uint32_t* q, const uint32_t* S, const uint32_t* F,
                       const uint32_t* T, const uint32_t* SF, const uint32_t* ST, const uint32_t* nxm1,
                       const uint32_t* scalars, const uint32_t* halo, uint64_t Ml, int W, int r, int rot);
void launch_nxm1_e(hipStream_t st, uint32_t* out, const uint32_t* tw, int lcs, const uint32_t* gp, const uint32_t* np,
                   int W, int r);
void launch_div_fix(hipStream_t st, uint32_t* q, const uint32_t* pz, const uint32_t* c, uint64_t Lb);

// lookup.hip
// k columns of 32 B STANDARD-form elements (any 256-bit value; rows compare as elements of Fr)
struct LookupCols {
  int k;
  const uint32_t* col[EB_MAX];
};
// out[j] (Montgomery) = number of rows i < n of F with sel_f[i] == one (nullptr: every row) that equal
// row j of T, a repeated table row's whole count on its lowest index. table: `capacity` (a power of two
// >= 2n) words preset to 0xFFFFFFFF; count: n words preset to 0; flags: two words preset to
// 0xFFFFFFFF that receive the lowest row of F missing from T and the lowest row whose selector is
// neither zero nor Montgomery one.
void launch_lookup_multiplicities(hipStream_t st, uint32_t* out, uint32_t* table, uint64_t capacity, uint32_t* count,
                                  uint32_t* flags, const LookupCols& F, const LookupCols& T, const uint32_t* sel_f,
                                  uint64_t n);

// fold.hip
// out_aff[s] (64 B affine LEM, zeros for the identity) = sum_{t in [seg_off[s], seg_off[s + 1])} scalars[t] * points[t]
// for s < nseg. points: nterms affine LEM points on the curve (zero allowed); scalars: nterms x 8 words,
// STANDARD form, any 256-bit integer; seg_off: nseg + 1 non-decreasing term offsets, seg_off[nseg] == nterms.
// Work buffers: term_xyzz 128 B x nterms, seg_xyzz 128 B x nseg, scratch 32 B x nseg.
void launch_g1_fold(hipStream_t st, uint32_t* out_aff, const uint32_t* points, const uint32_t* scalars,
                    const uint32_t* seg_off, uint64_t nterms, uint64_t nseg, uint32_t* term_xyzz, uint32_t* seg_xyzz,
                    uint32_t* scratch);

// msm.hip
// table row 0: the points as loaded, replaced by rho * P_i (rho: standard form of 2^-256 mod r) before
// the window rows are expanded; *zero_flag (a device word) ends as 1 if some P_i is the zero point
void msm_build_table(hipStream_t st, uint32_t* table, uint64_t npts, int c, int W, uint32_t* tmp_xyzz,
                     uint32_t* scratch, const uint32_t rho[8], uint32_t* zero_flag);
// scalars[i] multiplies SRS point pbase + pstride * i (pbase + pstride * (N - 1) < tb.npts).
// exclusive_acc: the bucket accumulation takes a SIMD's whole register file at its two waves (for a
// context whose two MSM lanes would otherwise co-run their accumulations and delay each other's
// tails); default: a 168-VGPR build that leaves room for other proofs' kernels (msm.hip). w sized by
// msm_work_sizes(tb.npts, tb.c, tb.c, 2^(tb.c - 1), 1). Returns false, with nothing launched, for a window
// the sort has no instantiation for (outside 7 .. 20).
bool msm_run(hipStream_t st, const MsmTables& tb, MsmWork& w, const uint32_t* scalars, uint64_t N, uint32_t* T_out,
             hipEvent_t* ev = nullptr, uint64_t pbase = 0, uint64_t pstride = 1, bool exclusive_acc = false);
// Variable-base MSM over one row of points, no window tables (msm.hip). Window c in
// MSM_POINTS_C_MIN .. MSM_POINTS_C_MAX: W = ceil(255 / c) windows of B = 2^(c-1) buckets each, and
// W * B <= 2^19 is the largest key space the sort partitions (c = 16 reaches it exactly). The partition
// pass stages 256 * 2 * W * 7 B + 12 B per partition in LDS: 133.0 KB at c = 7, of a workgroup's 160 KB.
constexpr int MSM_POINTS_C_MIN = 7, MSM_POINTS_C_MAX = 16;
// bytes of the MsmWork buffers (same roles as in msm_run) and of the T output
inline MsmSizes msm_points_work_sizes(uint64_t N, int c) {
  const int W = msm_windows(c);
  return msm_work_sizes(N, c, msm_points_c_sort(c), (uint64_t)W << (c - 1), W);
}
// row (N affine points, 256-bit Montgomery, zeros = identity) -> the accumulation's 29-bit form, in place
void msm_points_row29(hipStream_t st, uint32_t* row, uint64_t N);
// T_out[j * c + k] (XYZZ, 128 B) = sum of window j's buckets with bit k set, so that
// sum_i s_i P_i = sum_m 2^m T_out[m] over m < W * c. scalars_std: N x 8 words, any 256-bit integers (taken
// mod r). N >= 1, N * W <= 2^31; w sized by msm_points_work_sizes(N, c). Returns false, with nothing
// launched, for a window outside MSM_POINTS_C_MIN .. MSM_POINTS_C_MAX.
bool msm_points_run(hipStream_t st, MsmWork& w, const uint32_t* row29, const uint32_t* scalars_std, uint64_t N, int c,
                    uint32_t* T_out);
void launch_fixed_base(hipStream_t st, uint32_t* out_xyzz, const uint32_t* sc, uint64_t count, const uint32_t* tbl);
void launch_batch_affine(hipStream_t st, uint32_t* out_aff, const uint32_t* in_xyzz, uint32_t* scratch, uint64_t npts);

// g1ntt.hip
// Radix-2 NTT over G1, natural order in and out, n = 2^logn affine LEM points (zeros =
// identity): out_j = scale * sum_i root^(i j) P_i. root_mont: a primitive n-th root of unity (Montgomery
// words; its inverse for the inverse transform); scale_std: a standard-form factor < r applied to every
// output (nullptr or 1: none). in_aff is only read, unless out_aff aliases it, which is allowed.
constexpr int G1NTT_TW_WORDS = 16;  // a twiddle's signed-digit record: the masks of its +1 and of its -1 digits
// which lanes of a wave share a twiddle: AUTO takes the per-wave mapping in every stage that has at
// least 64 butterfly groups and a twiddle other than 1; LANE / WAVE force one for A/B timing
// (kgs_bench_g1_ntt; WAVE still needs the 64 groups)
constexpr int G1NTT_MAP_AUTO = 0, G1NTT_MAP_LANE = 1, G1NTT_MAP_WAVE = 2;
struct G1NttSizes {  // bytes of the work buffers
  uint64_t xyzz, aff, scratch, tw;
};
G1NttSizes g1_ntt_sizes(int logn);
struct G1NttWork {
  uint32_t *xyzz = nullptr, *aff = nullptr, *scratch = nullptr, *tw = nullptr;
};
// stages: -1 runs all logn stages. 1 <= stages < logn stops after the stages of half-width 1 .. 2^(stages-1)
// (DESIGN.md §20): the 2^(logn-stages) blocks of 2^stages consecutive outputs are then the transforms of size
// 2^stages (root root^(2^(logn-stages))) of the input's subsequences of stride 2^(logn-stages), block b
// holding the subsequence of residue bitrev(b); scale_std applies to them as to a whole transform.
void g1_ntt_run(hipStream_t st, const G1NttWork& w, uint32_t* out_aff, const uint32_t* in_aff, int logn,
                const uint32_t root_mont[8], const uint32_t* scale_std, int mapping, int stages = -1);
// out_aff[i] = scale_std * in_aff[i], i < n: the transform's scaling pass on its own (w sized for n points)
void launch_g1_scale(hipStream_t st, const G1NttWork& w, uint32_t* out_aff, const uint32_t* in_aff, uint64_t n,
                     const uint32_t scale_std[8]);
// out_xyzz[i] = k_i * in_aff[i], i < n, a scalar of its own per point (follow with
// launch_batch_affine). scalars: n x 8 words read as integers; reduce: any 256-bit integers, taken mod r,
// else every k_i < r already (an Fr kernel's output words). in_aff: zeros = identity.
void launch_g1_mul_each(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars, uint64_t n,
                        bool reduce);
// out_xyzz[i] = sum_{r < rows} k[r cols + i] * in_aff[r cols + i], i < cols (follow with
// launch_batch_affine over cols points). out_xyzz holds rows * cols XYZZ points: the products land there
// (scalars and `reduce` as launch_g1_mul_each takes them) and are summed in place, by eights, into row 0. The
// sum takes the identity, equal and opposite branches of g1_xyzz::add, the grouped kernel those of add_aff.
// group: 2, two rows of a column per lane sharing their doublings (k_g1_mul_group; the products then fill
// the first ceil(rows / 2) rows of out_xyzz), or 1, launch_g1_mul_each over all the terms (what rows == 1 takes,
// and the other arm of the A/B).
// Below G1_MUL_GROUP_MIN_TERMS terms (the smallest size at which the grouped kernel measured faster) group 2
// takes the one-row route as well.
constexpr int G1_MUL_SUM_GROUP = 2;
constexpr uint64_t G1_MUL_GROUP_MIN_TERMS = 1ull << 17;
void launch_g1_mul_sum(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars, uint64_t rows,
                       uint64_t cols, bool reduce, int group = G1_MUL_SUM_GROUP);
// The Fr side of kgs_kzg_open_cosets, l = 2^lbits >= 2 rows of m = 2^logm elements of 8 words:
// out[b m + u] = in[u l + bitrev_l(b)], zero from index len on (the rows in the cached G1 rows' order)
void launch_coset_rows(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t len, int logm, int lbits);
// out[b 2^logm + j] = in[b 2^logm + bitrev(j)], b < nblocks, out of place: launch_bitrev_copy per block
void launch_bitrev_blocks(hipStream_t st, uint32_t* out, const uint32_t* in, int logm, uint64_t nblocks);
// npts affine points of a table row (coordinates x * 2^261, msm_points_row29) -> the 2^256 form, out of
// place; reversed: out_aff[npts - 1 - i] = point i, or with block_log > 0 the blocks of 2^block_log points
// in reverse order, each block in its own order (npts a multiple of the block)
void launch_g1_from29(hipStream_t st, uint32_t* out_aff, const uint32_t* in29, uint64_t npts, bool reversed = false,
                      int block_log = 0);
// The stages of kgs_kzg_open_cosets_many, each one launch for all the polynomials.
// `polys` transforms of size 2^logn side by side, transform p over the points [p n, (p + 1) n) of in_aff and
// out_aff (which may alias): g1_ntt_run without a scaling, one twiddle table of size n, the thread mapping of
// g1ntt_map.hpp (mapping: G1NTT_MAP_AUTO, or G1NTT_MAP_LANE for the A/B). w sized for polys * n points, w.tw
// for one transform of size n.
void g1_ntt_many_run(hipStream_t st, const G1NttWork& w, uint32_t* out_aff, const uint32_t* in_aff, uint64_t polys,
                     int logn, const uint32_t root_mont[8], int mapping);
// launch_g1_mul_sum over rows x (polys pcols) scalars below r (an Fr kernel's output words) against rows x pcols points,
// pcols a power of two: out_xyzz[p pcols + i] = sum_r k[r][p pcols + i] * in_aff[r pcols + i]. out_xyzz as
// launch_g1_mul_sum's for rows x (polys pcols) terms.
void launch_g1_mul_sum_many(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars,
                            uint64_t rows, uint64_t polys, uint64_t pcols, int group = G1_MUL_SUM_GROUP);
// launch_coset_rows for polys polynomials (len coefficients each, `stride` elements apart) into nblocks >= l polys
// blocks of 2^logblk >= m elements, block b polys + p = the row of residue bitrev_l(b) of polynomial p, zero behind
// its m elements; the blocks from l polys on are zero. lbits = 0, logblk = logm: the zero-padded coefficients.
void launch_coset_rows_many(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t polys, uint64_t stride, uint64_t len,
                            int logm, int lbits, int logblk, uint64_t nblocks);
// h[p m + k] = u[p 2m + m - 1 + k], k < m - 1, and h[p m + m - 1] = the identity: m = 2^logm points of 64 B
void launch_coset_slice_many(hipStream_t st, uint32_t* h, const uint32_t* u, int logm, uint64_t polys);


// coset_fold.hip (the batch verifier for coset openings)
// The fused interpolation fold covers l = 2^lbits up to 2^COSET_FOLD_LBITS_MAX values per row (32 KiB of LDS).
constexpr int COSET_FOLD_LBITS_MAX = 10;
// blocks of the fold over `count` rows: one per tile of max(1, 512 / l) rows, at most 1024
inline unsigned coset_fold_blocks(uint64_t count, int lbits) {
  const uint64_t rt = lbits < 9 ? 512u >> lbits : 1, tiles = (count + rt - 1) / rt;
  return (unsigned)(tiles < 1 ? 1 : tiles > 1024 ? 1024 : tiles);
}
// bytes of launch_coset_interp_fold's `part`
inline uint64_t coset_fold_part_bytes(uint64_t count, int lbits) {
  return 32ull * coset_fold_blocks(count, lbits) * ((1ull << lbits) > 256 ? (1ull << lbits) : 256);
}
// out[j] (Montgomery) = sum_{k < count} weights[k] * w^(-index[k] j) * J_{k,j}, j < l = 2^lbits, with w = Fr.w[nbits]
// and J_k the inverse transform of size l (kgs_ntt's convention, 1 / l included) of the l values of row k of ys
// (count x l Montgomery elements, rows contiguous). A row with weight 0 is not read. valid: NULL, or count bytes:
// a row with 0 there is skipped. A row with a value or a weight >= r or an index >= 2^(nbits - lbits) is skipped too, gets 0
// in `valid` and sets *bad (a device word the caller has zeroed) to 1. tw_inv / invm: the domain's tables,
// covering 2^nbits. Returns false, with nothing launched, for lbits outside 0 .. min(COSET_FOLD_LBITS_MAX, nbits).
bool launch_coset_interp_fold(hipStream_t st, uint32_t* out, uint32_t* part, uint8_t* valid, uint32_t* bad,
                              const uint32_t* ys, const uint64_t* index, const uint32_t* weights, uint64_t count,
                              const uint32_t* tw_inv, const uint32_t* invm, int nbits, int lbits);
// ok[i] = 1 if point i (64 B affine LEM) is the identity or has canonical coordinates on y^2 = x^3 + 3, else 0
void launch_g1_on_curve(hipStream_t st, uint8_t* ok, const uint32_t* points, uint64_t n);
// valid[k] = proof_ok[k] && commit_of[k] < ncommits && commit_ok[commit_of[k]] && index[k] < m, k < count
void launch_coset_screen(hipStream_t st, uint8_t* valid, const uint8_t* proof_ok, const uint8_t* commit_ok,
                         const uint32_t* commit_of, const uint64_t* index, uint64_t count, uint64_t ncommits,
                         uint64_t m);
// The 3 cnt + l terms of the openings lo <= k < lo + cnt (standard-form scalars, 64 B points): w_k pi_k (the cnt
// terms of A), then B's: w_k C_c(k), w_k a_{i_k} pi_k, and -D_j srs_j for j < l (two launches: k_coset_terms,
// k_coset_terms_srs). Openings with valid[k] == 0 give zero scalars and identities. tw_fwd covers 2^(nbits - lbits).
void launch_coset_terms(hipStream_t st, uint32_t* scal, uint32_t* pts, const uint8_t* valid, const uint32_t* weights,
                        const uint64_t* index, const uint32_t* commit_of, const uint32_t* commits,
                        const uint32_t* proofs, const uint32_t* D, const uint32_t* srs, const uint32_t* tw_fwd,
                        uint64_t lo, uint64_t cnt, int nbits, int lbits);

// recover.hip (kgs_kzg_recover_cosets). m = 2^logm cosets of l = 2^lbits points, n = m l.
constexpr uint32_t RC_NONE = 0xFFFFFFFFu;  // row_of: the coset is missing
// the call's four flag words: the lowest row with an index >= m, the lowest row that names a coset again, the
// lowest value (row * l + j) >= r (each preset to RC_NONE), and 1 for a nonzero coefficient from len on (preset 0)
constexpr int RC_FLAG_INDEX = 0, RC_FLAG_DUP = 1, RC_FLAG_VALUE = 2, RC_FLAG_HIGH = 3;
// A leaf of the product tree covers 2^leaf_log coset slots (one thread each). A leaf costs B / 4 products per slot
// at half the cosets missing, a tree level a constant; 64, 128 and 256 measured within a few per cent of each other
// at every size, and 64 is the least arithmetic. The kernel is built for up to 512 (its LDS, below,
// stays under the 64 KiB of a plain launch).
constexpr int RC_LEAF_LOG = 6, RC_LEAF_LOG_MIN = 6, RC_LEAF_LOG_MAX = 9, RC_LEAF_MAX = 1 << RC_LEAF_LOG_MAX;
inline unsigned rc_leaf_lds_bytes(int leaf_log) { return (6u * 16u + 4u) << leaf_log; }
// row_of (m words preset to RC_NONE) and flags from the `count` coset indices
void launch_rc_mark(hipStream_t st, uint32_t* row_of, uint32_t* flags, const uint64_t* index, uint64_t count, uint64_t m);
// T (m elements): block b of 2^leaf_log elements = the low coefficients of Y^(B - d) prod (Y - a_i) over the d missing
// slots of [b B, (b + 1) B), monic of degree B. leaf_log <= min(logm, RC_LEAF_LOG_MAX); tw_fwd covers m.
void launch_rc_leaves(hipStream_t st, uint32_t* T, const uint32_t* row_of, const uint32_t* tw_fwd, int logm, int leaf_log);
// One level: T's m / d monic polynomials of degree d = 2^logd (d low coefficients each) -> the m / 2d products of
// neighbours, in place. W: 2m elements of work space. tw_fwd / tw_inv / invm cover 2d.
void launch_rc_level(hipStream_t st, uint32_t* T, uint32_t* W, int logm, int logd, const uint32_t* tw_fwd,
                     const uint32_t* tw_inv, const uint32_t* invm);
// the root T = Y^count z(Y) -> zc[t] = z_t and zs[t] = z_t g^(l t), t < m (coset_pow covers n)
void launch_rc_zcoef(hipStream_t st, uint32_t* zc, uint32_t* zs, const uint32_t* T, uint64_t count, uint64_t m,
                     const uint32_t* coset_pow, int lbits);
// out[i + m j] = ys[row_of[i] l + j] * zev[bitrev_m(i)], zero where row_of[i] == RC_NONE; a value >= r counts as
// zero and lowers flags[RC_FLAG_VALUE] to its position
void launch_rc_scatter(hipStream_t st, uint32_t* out, const uint32_t* ys, const uint32_t* row_of, const uint32_t* zev,
                       uint32_t* flags, int logm, int lbits);
// out[i] = 1 / in[i], i < n, zero for zero; out != in
void launch_rc_batch_inv(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t n);
// data[x] *= inv[x >> lbits], x < n
void launch_rc_divide(hipStream_t st, uint32_t* data, const uint32_t* inv, int lbits, uint64_t n);
// coef[j] = q[j] for j < len; flags[RC_FLAG_HIGH] = 1 if q[j] != 0 for some len <= j < n
void launch_rc_check_copy(hipStream_t st, uint32_t* coef, const uint32_t* q, uint64_t len, uint64_t n, uint32_t* flags);
// kgs_kzg_recover_cosets_many: P = 2^logP >= polys polynomials side by side, the arrays of P m slots
// (2^logtotal with logtotal = logP + logm) or of P n elements (logtotal = logP + nbits). launch_rc_level,
// launch_rc_batch_inv and launch_rc_divide serve these arrays as they are.
// row_of (P m words preset to RC_NONE): the lowest cell naming (poly_of[k], index[k]); cnt (P words preset to 0): the
// distinct cosets of each polynomial; flags[RC_FLAG_INDEX]: the lowest cell with poly_of >= polys or index >= m;
// flags[RC_FLAG_DUP]: the lowest cell naming a pair again
void launch_rcm_mark(hipStream_t st, uint32_t* row_of, uint32_t* flags, uint32_t* cnt, const uint32_t* poly_of,
                     const uint64_t* index, uint64_t count, uint64_t polys, uint64_t m);
// launch_rc_leaves over the 2^logtotal slots, a_i from the slot's index mod m; leaf_log <= min(logm, RC_LEAF_LOG_MAX)
void launch_rcm_leaves(hipStream_t st, uint32_t* T, const uint32_t* row_of, const uint32_t* tw_fwd, int logtotal, int logm,
                       int leaf_log);
// launch_rc_zcoef per block of m: block b's root is Y^cnt[b] z_b(Y)
void launch_rcm_zcoef(hipStream_t st, uint32_t* zc, uint32_t* zs, const uint32_t* T, const uint32_t* cnt, int logtotal,
                      int logm, const uint32_t* coset_pow, int lbits);
// out[b n + bitrev_n(i + m j)] = ys[row_of[b m + i] l + j] * zev[b m + bitrev_m(i)], zero on a missing coset; a value
// >= r as launch_rc_scatter takes it
void launch_rcm_scatter(hipStream_t st, uint32_t* out, const uint32_t* ys, const uint32_t* row_of, const uint32_t* zev,
                        uint32_t* flags, int logtotal, int logm, int lbits);
// data[x] *= tab[x mod n], x < 2^logtotal
void launch_rcm_twist(hipStream_t st, uint32_t* data, const uint32_t* tab, int logtotal, int nbits);
// coef[b stride + j] = q[b n + j] ipow[j] for j < len, b < polys; high[b] = 1 if q[b n + j] != 0 for some len <= j < n
void launch_rcm_check_copy(hipStream_t st, uint32_t* coef, const uint32_t* q, const uint32_t* ipow, uint64_t len,
                           uint64_t stride, int nbits, uint64_t polys, uint32_t* high);

}  // namespace kgs
