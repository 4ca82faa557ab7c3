// The KZG openings over the whole resident SRS (include/kgs.h), a protocol layer on the G1 transform (g1_ntt.cpp;
// kernels and device drivers in g1ntt.hip): kgs_kzg_open (one point, as the rounds compose it), kgs_kzg_open_all
// (DESIGN.md §19), kgs_kzg_open_cosets (§20) and kgs_kzg_open_cosets_many (§23: §20's pipeline with a polynomial
// dimension in every stage), with their timing helpers.
//
// Host: argument checks (check_cosets_many), one entry for the three calls that open everything at once
// (open_entry: the staging between the caller's buffers and the device), each call's own device pipeline
// (kzg_open_all_run, kzg_open_cosets_run, kzg_open_cosets_many_run), and the SRS side of the Toeplitz product,
// cached per (SRS, nbits, lbits) under the one rule of context.hpp (srs_row_cached).
#include <mutex>

#include "context.hpp"

namespace {

constexpr int KZG_OPEN_ALL_LOG_MAX = G1_NTT_LOG_MAX - 1;  // the Toeplitz product transforms 2n points
constexpr uint64_t KZG_MANY_MAX_SLOTS = 1ull << 24;       // polys * n

// the refusals of the calls over the whole resident SRS, in kgs_srs_lagrange's words
void check_open_all(const kgs_ctx& c, int nbits, const char* fn) {
  check_plain_ctx(c, fn);
  if (nbits < 0 || nbits > KZG_OPEN_ALL_LOG_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " + std::to_string(KZG_OPEN_ALL_LOG_MAX));
  check_lagrange(c, nbits, fn);
}

// The refusals of the three calls beyond a NULL context and NULL buffers (the caller holds the context). A single
// call is polys = 1, stride = len, which passes the last two: nbits <= 23, so 2^24 >> nbits >= 2.
void check_cosets_many(const kgs_ctx& c, uint64_t polys, uint64_t stride, uint64_t len, int nbits, int lbits, const char* fn) {
  check_open_all(c, nbits, fn);
  if (lbits < 0 || lbits > nbits)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": lbits must be in 0 .. nbits = " + std::to_string(nbits));
  const uint64_t n = 1ull << nbits;
  if (len > n)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": len = " + std::to_string(len) + " coefficients do not fit the domain of 2^" +
                                  std::to_string(nbits) + " points.");
  if (stride < len)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": stride = " + std::to_string(stride) + " is below len = " + std::to_string(len));
  if (polys > KZG_MANY_MAX_SLOTS >> nbits)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": polys = " + std::to_string(polys) + " times 2^nbits is above 2^24.");
}

// ------------------------------------------------------------------ the cached SRS side
// The rows of (the context's SRS, nbits, lbits, m = n / l), enqueued on the main stream and not yet published.
// X_{j l + r} = x^(r)_j = s_{(m-2-j) l + r} for j <= m - 2 and the identity above: the first n - l points of
// table row 0 with their blocks of l reversed. The l transforms of size 2m of the stride-l subsequences of X are
// the first log2(2m) stages of the transform of size 2n (g1_ntt_run, `stages`), then one uniform scaling by
// 1 / 2m. Block b of the result holds the row of residue bitrev_l(b): kzg_open_cosets_run lays the Fr side out in
// the same order (launch_coset_rows). lbits = 0 is kgs_kzg_open_all's row: x = (s_{n-2}, .., s_0, identity x
// (n + 1)), every stage, 1 / 2n. Row 0's rho = 2^-256 stays on the points: the pointwise pass multiplies by
// Montgomery words, which carry 2^256.
std::shared_ptr<SrsRow> coset_build(kgs_ctx& c, int nbits, int lbits) {
  const uint64_t n = 1ull << nbits, l = 1ull << lbits;
  auto row = SrsRow::make(c.device, n, 128 * n);
  uint32_t* x = c.buf("gn_io", 128 * n);
  HC(hipMemsetAsync(x, 0, 128 * n, c.st));
  launch_g1_from29(c.st, x, c.tb.table, n - l, true, lbits);
  const int logm2 = nbits - lbits + 1;
  const G1NttWork w = ntt_work(c, nbits + 1);
  uint32_t root[8], sc[8];
  fr_words(ntt_root(nbits + 1, false), root);
  fr_words(ninv_std(logm2), sc);
  g1_ntt_run(c.st, w, row->p, x, nbits + 1, root, sc, G1NTT_MAP_AUTO, logm2);
  check_launch();
  return row;
}

// the cached rows, built on first use (srs_row_cached)
std::shared_ptr<SrsRow> coset_row(kgs_ctx& c, int nbits, int lbits) {
  return srs_row_cached(c, c.srs->fk, {nbits, lbits}, [&] { return coset_build(c, nbits, lbits); });
}

// u = (the Fr transform's output words) x (the cached points), pointwise, affine, into w.aff
void fk_pointwise(kgs_ctx& c, const G1NttWork& w, const SrsRow& row, const uint32_t* chat_words) {
  launch_g1_mul_each(c.st, w.xyzz, row.p, chat_words, 2 * row.n, false);
  launch_batch_affine(c.st, w.aff, w.xyzz, w.scratch, 2 * row.n);
}

// u^_i = sum_r (the Fr transforms' output words)_{r, i} x (the cached points)_{r, i}, i < 2m, affine, into w.aff
void coset_pointwise(kgs_ctx& c, const G1NttWork& w, const SrsRow& row, const uint32_t* chat_words, int lbits,
                     int group = G1_MUL_SUM_GROUP) {
  const uint64_t cols = (2 * row.n) >> lbits;
  launch_g1_mul_sum(c.st, w.xyzz, row.p, chat_words, 1ull << lbits, cols, false, group);
  launch_batch_affine(c.st, w.aff, w.xyzz, w.scratch, cols);
}

// the two G1 transforms of an opening: u = the unscaled inverse of size 2m in place in w.aff (the cached row has
// its 1 / 2m), h = u_{m-1 .. 2m-3} and one identity, the forward transform of size m of h into d_proofs
void coset_transforms(kgs_ctx& c, const G1NttWork& w, int logm, uint32_t* h, uint32_t* d_proofs) {
  const uint64_t m = 1ull << logm;
  uint32_t root[8];
  fr_words(ntt_root(logm + 1, true), root);
  g1_ntt_run(c.st, w, w.aff, w.aff, logm + 1, root, nullptr, G1NTT_MAP_AUTO);
  if (m > 1) HC(hipMemcpyAsync(h, w.aff + 16 * (m - 1), 64 * (m - 1), hipMemcpyDeviceToDevice, c.st));
  HC(hipMemsetAsync(h + 16 * (m - 1), 0, 64, c.st));
  fr_words(ntt_root(logm, false), root);
  g1_ntt_run(c.st, w, d_proofs, h, logm, root, nullptr, G1NTT_MAP_AUTO);
}

// ------------------------------------------------------------------ every domain point
// All n = 2^nbits openings of the polynomial with the `len` <= n Montgomery coefficients at d_coef (device),
// enqueued on the main stream (not synchronised): n affine LEM proofs into d_proofs, p(w^i) into d_evals
// (or nullptr). The caller holds the context, has checked it (check_open_all) and reset its staging.
void kzg_open_all_run(kgs_ctx& c, const uint32_t* d_coef, uint64_t len, int nbits, uint32_t* d_proofs,
                      uint32_t* d_evals) {
  const uint64_t n = 1ull << nbits;
  const int logm = nbits + 1;
  if (!len) {  // the zero polynomial
    HC(hipMemsetAsync(d_proofs, 0, 64 * n, c.st));
    if (d_evals) HC(hipMemsetAsync(d_evals, 0, 32 * n, c.st));
    return;
  }
  const std::shared_ptr<SrsRow> row = coset_row(c, nbits, 0);
  if (logm > c.logM) ensure_domain(c, logm);
  uint32_t* sa = c.buf("fk_fr", 64 * n);
  uint32_t* sb = c.buf("fk_chat", 64 * n);
  uint32_t* h = c.buf("fk_h", 64 * n);
  const G1NttWork w = ntt_work(c, logm);  // serves the transform of size n too
  // c^ = the Fr transform of size 2n of the zero-padded coefficients, natural order
  ntt_dif(c.st, sa, d_coef, len, logm, nullptr, c.tw_fwd, c.logM);
  launch_bitrev_copy(c.st, sb, sa, logm);
  fk_pointwise(c, w, *row, sb);
  coset_transforms(c, w, nbits, h, d_proofs);  // h_k = u_{n-1+k}
  if (d_evals) {
    ntt_dif(c.st, sa, d_coef, len, nbits, nullptr, c.tw_fwd, c.logM);
    launch_bitrev_copy(c.st, d_evals, sa, nbits);
  }
  check_launch();
}

// ------------------------------------------------------------------ coset openings
// All m = 2^(nbits - lbits) coset openings (kgs.h kgs_kzg_open_cosets) of the polynomial with the `len` <= n
// Montgomery coefficients at d_coef (device), enqueued on the main stream (not synchronised). lbits = 0 is
// kzg_open_all_run. The caller holds the context, has checked it and reset its staging.
void kzg_open_cosets_run(kgs_ctx& c, const uint32_t* d_coef, uint64_t len, int nbits, int lbits, uint32_t* d_proofs,
                         uint32_t* d_evals) {
  if (!lbits) return kzg_open_all_run(c, d_coef, len, nbits, d_proofs, d_evals);
  const uint64_t n = 1ull << nbits, l = 1ull << lbits, m = n >> lbits;
  const int logm = nbits - lbits;
  if (!len) {  // the zero polynomial
    HC(hipMemsetAsync(d_proofs, 0, 64 * m, c.st));
    if (d_evals) HC(hipMemsetAsync(d_evals, 0, 32 * n, c.st));
    return;
  }
  uint32_t* sa = c.buf("fk_fr", 64 * n);
  if (m == 1) {  // one coset, the whole domain: p = I, the quotient is zero
    HC(hipMemsetAsync(d_proofs, 0, 64, c.st));
  } else {
    const std::shared_ptr<SrsRow> row = coset_row(c, nbits, lbits);
    if (logm + 1 > c.logM) ensure_domain(c, logm + 1);
    uint32_t* rows = c.buf("fk_rows", 32 * n);
    uint32_t* sb = c.buf("fk_chat", 64 * n);
    uint32_t* h = c.buf("fk_h", 64 * m);
    const G1NttWork w = ntt_work(c, nbits + 1);  // xyzz holds the 2n products; serves both transforms too
    // row b of the Fr side = the coefficients of residue bitrev_l(b), the order of the cached rows' blocks
    launch_coset_rows(c.st, rows, d_coef, len, logm, lbits);
    for (uint64_t b = 0; b < l; b++)  // c^ = the l zero-padded Fr transforms of size 2m
      ntt_dif(c.st, sa + 16 * m * b, rows + 8 * m * b, m, logm + 1, nullptr, c.tw_fwd, c.logM);
    launch_bitrev_blocks(c.st, sb, sa, logm + 1, l);
    coset_pointwise(c, w, *row, sb, lbits);
    coset_transforms(c, w, logm, h, d_proofs);
  }
  if (d_evals) {
    if (nbits > c.logM) ensure_domain(c, nbits);
    ntt_dif(c.st, sa, d_coef, len, nbits, nullptr, c.tw_fwd, c.logM);
    launch_bitrev_copy(c.st, d_evals, sa, nbits);
  }
  check_launch();
}

// ------------------------------------------------------------------ coset openings of many polynomials
int log2_ceil(uint64_t x) {
  int lg = 0;
  while ((1ull << lg) < x) lg++;
  return lg;
}

// The sizes and the device buffers of one call ("km_*": the call's own, beside the single call's "fk_*" / "gn_*").
// lbits >= 1 here; lbits = 0 goes polynomial by polynomial through kzg_open_all_run.
struct CosetsMany {
  uint64_t polys, stride, len, n, l, m;
  int nbits, lbits, logm;
  int log_fr_blocks;  // the l polys blocks of 2m of the Fr side, rounded up to the power of two ntt_dif_blocks takes
  int log_ev_blocks;  // the polys blocks of n of the evaluations, likewise
  uint32_t *fr = nullptr, *chat = nullptr, *h = nullptr;
  G1NttWork w;  // xyzz: the products of the multiply-sum pass, then the stages' outputs; aff: u, in place
};

CosetsMany cosets_many_plan(kgs_ctx& c, uint64_t polys, uint64_t stride, uint64_t len, int nbits, int lbits) {
  CosetsMany q;
  q.polys = polys, q.stride = stride, q.len = len, q.nbits = nbits, q.lbits = lbits, q.logm = nbits - lbits;
  q.n = 1ull << nbits, q.l = 1ull << lbits, q.m = q.n >> lbits;
  q.log_fr_blocks = log2_ceil(q.l * polys);
  q.log_ev_blocks = log2_ceil(polys);
  const uint64_t fr_elems = std::max((2 * q.m) << q.log_fr_blocks, q.n << q.log_ev_blocks);
  const uint64_t terms = 2 * q.n * polys, upts = 2 * q.m * polys;
  q.fr = c.buf("km_fr", 32 * fr_elems);
  q.chat = c.buf("km_chat", 32 * terms);
  q.h = c.buf("km_h", 64 * q.m * polys);
  // two rows per lane leave l / 2 rows of products (launch_g1_mul_sum), one row per lane all l; l >= 2
  q.w.xyzz = c.buf("km_xyzz", 128 * (terms >= G1_MUL_GROUP_MIN_TERMS ? terms / 2 : terms));
  q.w.aff = c.buf("km_aff", 64 * upts);
  q.w.scratch = c.buf("km_scratch", 32 * upts);
  q.w.tw = c.buf("km_tw", 4 * (uint64_t)G1NTT_TW_WORDS * (q.m + 1));
  return q;
}

// c^: the l polys zero-padded Fr transforms of size 2m, natural order, rows over polynomials, into q.chat
void cosets_many_fr(kgs_ctx& c, const CosetsMany& q, const uint32_t* d_coef) {
  launch_coset_rows_many(c.st, q.fr, d_coef, q.polys, q.stride, q.len, q.logm, q.lbits, q.logm + 1, 1ull << q.log_fr_blocks);
  ntt_dif_blocks(c.st, q.fr, q.log_fr_blocks + q.logm + 1, q.logm + 1, c.tw_fwd);
  launch_bitrev_blocks(c.st, q.chat, q.fr, q.logm + 1, q.l * q.polys);
}

// u^[p][i] = sum_r c^[r][p][i] x (the cached points)[r][i], affine, into q.w.aff
void cosets_many_pointwise(kgs_ctx& c, const CosetsMany& q, const SrsRow& row) {
  launch_g1_mul_sum_many(c.st, q.w.xyzz, row.p, q.chat, q.l, q.polys, 2 * q.m);
  launch_batch_affine(c.st, q.w.aff, q.w.xyzz, q.w.scratch, 2 * q.m * q.polys);
}

// coset_transforms for all the polynomials, each stage one launch: the unscaled inverses of size 2m in place in
// q.w.aff, the slices, the forward transforms of size m into d_proofs
void cosets_many_transforms(kgs_ctx& c, const CosetsMany& q, uint32_t* d_proofs, int mapping) {
  uint32_t root[8];
  fr_words(ntt_root(q.logm + 1, true), root);
  g1_ntt_many_run(c.st, q.w, q.w.aff, q.w.aff, q.polys, q.logm + 1, root, mapping);
  launch_coset_slice_many(c.st, q.h, q.w.aff, q.logm, q.polys);
  fr_words(ntt_root(q.logm, false), root);
  g1_ntt_many_run(c.st, q.w, d_proofs, q.h, q.polys, q.logm, root, mapping);
}

// kgs_kzg_open_cosets_many on the main stream (not synchronised): the coset openings of the `polys` polynomials
// at d_coef (device; polynomial p at d_coef + 8 stride p words) into d_proofs (polys x m points) and d_evals
// (polys x n elements, or nullptr). The caller holds the context, has checked it and reset its staging.
void kzg_open_cosets_many_run(kgs_ctx& c, const uint32_t* d_coef, uint64_t polys, uint64_t stride, uint64_t len, int nbits,
                              int lbits, uint32_t* d_proofs, uint32_t* d_evals) {
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  if (!lbits) {  // one coset per point: no rows to sum over, kgs_kzg_open_all's path polynomial after polynomial
    for (uint64_t p = 0; p < polys; p++)
      kzg_open_all_run(c, d_coef + 8 * stride * p, len, nbits, d_proofs + 16 * n * p, d_evals ? d_evals + 8 * n * p : nullptr);
    return;
  }
  if (!len) {  // zero polynomials
    HC(hipMemsetAsync(d_proofs, 0, 64 * m * polys, c.st));
    if (d_evals) HC(hipMemsetAsync(d_evals, 0, 32 * n * polys, c.st));
    return;
  }
  std::shared_ptr<SrsRow> row;
  if (m > 1) row = coset_row(c, nbits, lbits);
  if (c.logM < (d_evals ? nbits : nbits - lbits + 1)) ensure_domain(c, d_evals ? nbits : nbits - lbits + 1);
  const CosetsMany q = cosets_many_plan(c, polys, stride, len, nbits, lbits);
  if (m == 1) {  // one coset, the whole domain: p = I, the quotient is zero
    HC(hipMemsetAsync(d_proofs, 0, 64 * polys, c.st));
  } else {
    cosets_many_fr(c, q, d_coef);
    cosets_many_pointwise(c, q, *row);
    cosets_many_transforms(c, q, d_proofs, G1NTT_MAP_AUTO);
  }
  if (d_evals) {  // the polys transforms of size n of the zero-padded coefficients, natural order
    launch_coset_rows_many(c.st, q.fr, d_coef, polys, stride, len, nbits, 0, nbits, 1ull << q.log_ev_blocks);
    ntt_dif_blocks(c.st, q.fr, q.log_ev_blocks + nbits, nbits, c.tw_fwd);
    launch_bitrev_blocks(c.st, d_evals, q.fr, nbits, polys);
  }
  check_launch();
}

// ------------------------------------------------------------------ the entry of the three calls
// what distinguishes the public calls at their entry
struct OpenCall {
  const char* fn;      // the public name, in every refusal
  const char* prefix;  // of the staged call's pool buffers (kgs.h): "fk_" for a single polynomial, "km_" for many
  const char *no_proofs, *no_coef;  // the words of the two NULL refusals
};
constexpr OpenCall OPEN_ALL{"kgs_kzg_open_all", "fk_", "NULL argument", "NULL argument"};
constexpr OpenCall OPEN_COSETS{"kgs_kzg_open_cosets", "fk_", "NULL argument", "NULL argument"};
constexpr OpenCall OPEN_MANY{"kgs_kzg_open_cosets_many", "km_", "NULL proofs buffer", "NULL coefficient buffer"};

// One call: the refusals, then `run` (the call's device pipeline: d_coef, stride, d_proofs, d_evals) between two
// resets of the staging, over the caller's device pointers or over the call's own buffers with the copies in and
// out. A single polynomial is polys = 1, stride = len. The staged coefficients are packed: the gaps of a stride
// above len stay on the host.
template <class Run>
int open_entry(kgs_ctx_t* ctx, const OpenCall& call, const void* coef, uint64_t polys, uint64_t stride, uint64_t len,
               int nbits, int lbits, void* proofs, void* evals, bool device, Run run) {
  API_BEGIN
  const std::string fn = call.fn, pre = call.prefix;
  if (!ctx) throw KgsError(KGS_E_ARG, fn + ": NULL ctx");
  if (!polys) return KGS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_cosets_many(*ctx, polys, stride, len, nbits, lbits, call.fn);
  if (!proofs) throw KgsError(KGS_E_ARG, fn + ": " + call.no_proofs);
  if (len && !coef) throw KgsError(KGS_E_ARG, fn + ": " + call.no_coef);
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  if (device) {
    run(c, (const uint32_t*)coef, stride, (uint32_t*)proofs, (uint32_t*)evals);
  } else {
    uint32_t* dc = c.buf(pre + "coef", 32 * (len ? len * polys : 1));
    uint32_t* dp = c.buf(pre + "out", 64 * m * polys);
    uint32_t* de = evals ? c.buf(pre + "ev", 32 * n * polys) : nullptr;
    if (len && stride == len)
      HC(hipMemcpyAsync(dc, coef, 32 * len * polys, hipMemcpyHostToDevice, c.st));
    else if (len)
      HC(hipMemcpy2DAsync(dc, 32 * len, coef, 32 * stride, 32 * len, polys, hipMemcpyHostToDevice, c.st));
    run(c, dc, len, dp, de);
    HC(hipMemcpyAsync(proofs, dp, 64 * m * polys, hipMemcpyDeviceToHost, c.st));
    if (evals) HC(hipMemcpyAsync(evals, de, 32 * n * polys, hipMemcpyDeviceToHost, c.st));
  }
  c.reset_staging();
  API_END
}

int open_all_entry(kgs_ctx_t* ctx, const void* coef, uint64_t len, int nbits, void* proofs, void* evals, bool device) {
  return open_entry(ctx, OPEN_ALL, coef, 1, len, len, nbits, 0, proofs, evals, device,
                    [&](kgs_ctx& c, const uint32_t* dc, uint64_t, uint32_t* dp, uint32_t* de) {
                      kzg_open_all_run(c, dc, len, nbits, dp, de);
                    });
}

int open_cosets_entry(kgs_ctx_t* ctx, const void* coef, uint64_t len, int nbits, int lbits, void* proofs, void* evals,
                      bool device) {
  return open_entry(ctx, OPEN_COSETS, coef, 1, len, len, nbits, lbits, proofs, evals, device,
                    [&](kgs_ctx& c, const uint32_t* dc, uint64_t, uint32_t* dp, uint32_t* de) {
                      kzg_open_cosets_run(c, dc, len, nbits, lbits, dp, de);
                    });
}

int open_many_entry(kgs_ctx_t* ctx, const void* coef, uint64_t polys, uint64_t stride, uint64_t len, int nbits, int lbits,
                    void* proofs, void* evals, bool device) {
  return open_entry(ctx, OPEN_MANY, coef, polys, stride, len, nbits, lbits, proofs, evals, device,
                    [&](kgs_ctx& c, const uint32_t* dc, uint64_t dstride, uint32_t* dp, uint32_t* de) {
                      kzg_open_cosets_many_run(c, dc, polys, dstride, len, nbits, lbits, dp, de);
                    });
}

// ------------------------------------------------------------------ one point
// One opening over the resident SRS as the rounds compose it: the Horner tiles for y, the synthetic
// division (whose quotient does not depend on the constant term, so p is divided as it is and the
// remainder flag is not read), the fixed-base MSM of the quotient.
void kzg_open_run(kgs_ctx& c, const uint8_t* coef_mont, uint64_t len, const Fr& z, uint8_t y_mont[32],
                  uint8_t proof_lem[64]) {
  c.reset_staging();
  if (!len) {
    memset(y_mont, 0, 32);
    memset(proof_lem, 0, 64);
    return;
  }
  uint32_t* a = c.buf("prim_a", 32 * len);
  HC(hipMemcpyAsync(a, coef_mont, 32 * len, hipMemcpyHostToDevice, c.st));
  EvalJob j = eval_launch(c, {a}, {len}, z, 0);
  Commit cm;
  if (len > 1) {
    uint32_t* q = c.buf("prim_b", 32 * len);
    const uint32_t dt = (uint32_t)((len + EVAL_TILE - 1) / EVAL_TILE);
    uint32_t* flag = c.buf("flags", 64);
    HC(hipMemsetAsync(flag, 0, 64, c.st));
    launch_divide(c.st, q, flag, a, len, xpowers(c, z), c.buf("div_part", 32 * (dt + 1)),
                  c.buf("div_carry", 32 * (dt + 1)));
    check_launch();
    cm = commit_launch(c, q, len - 1, 0);
  }
  c.sync();
  eval_finish(j)[0].to_bytes(y_mont);
  if (len > 1) commit_finish(c, cm, proof_lem);
  else memset(proof_lem, 0, 64);
  c.reset_staging();
}

}  // namespace

extern "C" {

int kgs_kzg_open(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t z_mont[32], uint8_t y_mont[32],
                 uint8_t proof_lem[64]) {
  API_BEGIN
  const char* fn = "kgs_kzg_open";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  if (!z_mont || !y_mont || !proof_lem || (len && !coef_mont)) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn);
  check_whole_srs(*ctx, fn);
  if (len > ctx->tb.npts + 1) throw KgsError(KGS_E_SRS, "MSM larger than the resident SRS");
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  kzg_open_run(*ctx, coef_mont, len, Fr::from_bytes(z_mont), y_mont, proof_lem);
  API_END
}

int kgs_kzg_open_all(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, int nbits, uint8_t* proofs_lem,
                     uint8_t* evals_mont) {
  return open_all_entry(ctx, coef_mont, len, nbits, proofs_lem, evals_mont, false);
}

int kgs_kzg_open_all_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, void* d_proofs_lem,
                            void* d_evals_mont) {
  return open_all_entry(ctx, d_coef_mont, len, nbits, d_proofs_lem, d_evals_mont, true);
}

int kgs_kzg_open_cosets(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, int nbits, int lbits, uint8_t* proofs_lem,
                        uint8_t* evals_mont) {
  return open_cosets_entry(ctx, coef_mont, len, nbits, lbits, proofs_lem, evals_mont, false);
}

int kgs_kzg_open_cosets_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int lbits,
                               void* d_proofs_lem, void* d_evals_mont) {
  return open_cosets_entry(ctx, d_coef_mont, len, nbits, lbits, d_proofs_lem, d_evals_mont, true);
}

int kgs_kzg_open_cosets_many(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t polys, uint64_t stride, uint64_t len,
                             int nbits, int lbits, uint8_t* proofs_lem, uint8_t* evals_mont) {
  return open_many_entry(ctx, coef_mont, polys, stride, len, nbits, lbits, proofs_lem, evals_mont, false);
}

int kgs_kzg_open_cosets_many_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t polys, uint64_t stride,
                                    uint64_t len, int nbits, int lbits, void* d_proofs_lem, void* d_evals_mont) {
  return open_many_entry(ctx, d_coef_mont, polys, stride, len, nbits, lbits, d_proofs_lem, d_evals_mont, true);
}

int kgs_kzg_open_cosets_cached(kgs_ctx_t* ctx, int nbits, int lbits) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "kgs_kzg_open_cosets_cached: NULL ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->srs) return 0;
  std::lock_guard<std::mutex> reg(g_reg_mu);
  return (int)ctx->srs->fk.count({nbits, lbits});
  API_END
}

// ---- timing helper of profiles/kzg_open_all_time.py
int kgs_bench_kzg_open_all(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int what, int reps,
                           double* ms) {
  API_BEGIN
  const char* fn = "kgs_bench_kzg_open_all";
  if (!ctx || !d_coef_mont || !ms) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (what < 0 || what > 2 || reps < 1) throw KgsError(KGS_E_ARG, std::string(fn) + ": bad what / reps");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_open_all(*ctx, nbits, fn);
  const uint64_t n = 1ull << nbits;
  if (len < 1 || len > n) throw KgsError(KGS_E_ARG, std::string(fn) + ": len must be in 1 .. 2^nbits");
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  const uint32_t* coef = (const uint32_t*)d_coef_mont;
  uint32_t* out = c.buf("fk_out", 64 * n);
  // every leg after one whole call: the row cached, the buffers grown, c^ in "fk_chat"
  kzg_open_all_run(c, coef, len, nbits, out, nullptr);
  HC(hipStreamSynchronize(c.st));
  const std::shared_ptr<SrsRow> row = coset_row(c, nbits, 0);
  const G1NttWork w = ntt_work(c, nbits + 1);
  const uint32_t* chat = c.buf("fk_chat", 64 * n);
  EventTimer timer;
  for (int r = 0; r < reps; r++) {
    std::shared_ptr<SrsRow> built;
    ms[r] = timer.ms(c.st, [&] {
      if (what == 0)
        kzg_open_all_run(c, coef, len, nbits, out, nullptr);
      else if (what == 1)
        built = coset_build(c, nbits, 0);
      else
        fk_pointwise(c, w, *row, chat);
    });
  }
  c.reset_staging();
  API_END
}

// ---- timing helper of profiles/kzg_open_cosets_time.py
int kgs_bench_kzg_open_cosets(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int lbits, int what,
                              int reps, double* ms) {
  API_BEGIN
  const char* fn = "kgs_bench_kzg_open_cosets";
  if (!ctx || !d_coef_mont || !ms) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (what < 0 || what > 5 || reps < 1) throw KgsError(KGS_E_ARG, std::string(fn) + ": bad what / reps");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_open_all(*ctx, nbits, fn);
  if (lbits < 1 || lbits >= nbits) throw KgsError(KGS_E_ARG, std::string(fn) + ": lbits must be in 1 .. nbits - 1");
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  if (len < 1 || len > n) throw KgsError(KGS_E_ARG, std::string(fn) + ": len must be in 1 .. 2^nbits");
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  const uint32_t* coef = (const uint32_t*)d_coef_mont;
  uint32_t* out = c.buf("fk_out", 64 * m);
  // every leg after one whole call: the rows cached, the buffers grown, c^ in "fk_chat", u in "gn_aff" and h
  // in "fk_h" (the operands the transform legs run over: points of this polynomial, no periodic vector)
  kzg_open_cosets_run(c, coef, len, nbits, lbits, out, nullptr);
  HC(hipStreamSynchronize(c.st));
  const std::shared_ptr<SrsRow> row = coset_row(c, nbits, lbits);
  const G1NttWork w = ntt_work(c, nbits + 1);
  const uint32_t* chat = c.buf("fk_chat", 64 * n);
  uint32_t* h = c.buf("fk_h", 64 * m);
  EventTimer timer;
  for (int r = 0; r < reps; r++) {
    std::shared_ptr<SrsRow> built;
    ms[r] = timer.ms(c.st, [&] {
      if (what == 0)
        kzg_open_cosets_run(c, coef, len, nbits, lbits, out, nullptr);
      else if (what == 1)
        built = coset_build(c, nbits, lbits);
      else if (what == 2)
        coset_pointwise(c, w, *row, chat, lbits);
      else if (what == 3)
        coset_transforms(c, w, nbits - lbits, h, out);
      else if (what == 4)
        launch_g1_mul_each(c.st, w.xyzz, row->p, chat, 2 * n, false);
      else
        coset_pointwise(c, w, *row, chat, lbits, 1);
    });
  }
  c.reset_staging();
  API_END
}

// ---- timing helper of profiles/kzg_open_cosets_many_time.py
int kgs_bench_kzg_open_cosets_many(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t polys, uint64_t stride, uint64_t len,
                                   int nbits, int lbits, int what, int reps, double* ms) {
  API_BEGIN
  const char* fn = "kgs_bench_kzg_open_cosets_many";
  if (!ctx || !d_coef_mont || !ms) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (what < 0 || what > 5 || reps < 1 || !polys) throw KgsError(KGS_E_ARG, std::string(fn) + ": bad what / reps / polys");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_cosets_many(*ctx, polys, stride, len, nbits, lbits, fn);
  if (lbits < 1 || lbits >= nbits) throw KgsError(KGS_E_ARG, std::string(fn) + ": lbits must be in 1 .. nbits - 1");
  if (len < 1) throw KgsError(KGS_E_ARG, std::string(fn) + ": len must be in 1 .. 2^nbits");
  const uint64_t m = 1ull << (nbits - lbits);
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  const uint32_t* coef = (const uint32_t*)d_coef_mont;
  uint32_t* out = c.buf("km_out", 64 * m * polys);
  uint32_t* one = c.buf("fk_out", 64 * m);
  // every leg after one whole call of each kind: the rows cached, the buffers grown, c^ in "km_chat", u in "km_aff"
  kzg_open_cosets_run(c, coef, len, nbits, lbits, one, nullptr);
  kzg_open_cosets_many_run(c, coef, polys, stride, len, nbits, lbits, out, nullptr);
  HC(hipStreamSynchronize(c.st));
  const std::shared_ptr<SrsRow> row = coset_row(c, nbits, lbits);
  const CosetsMany q = cosets_many_plan(c, polys, stride, len, nbits, lbits);
  EventTimer timer;
  for (int r = 0; r < reps; r++)
    ms[r] = timer.ms(c.st, [&] {
      if (what == 0)
        kzg_open_cosets_many_run(c, coef, polys, stride, len, nbits, lbits, out, nullptr);
      else if (what == 1)
        cosets_many_fr(c, q, coef);
      else if (what == 2)
        cosets_many_pointwise(c, q, *row);
      else if (what == 3 || what == 4)
        cosets_many_transforms(c, q, out, what == 3 ? G1NTT_MAP_AUTO : G1NTT_MAP_LANE);
      else
        for (uint64_t p = 0; p < polys; p++) kzg_open_cosets_run(c, coef + 8 * stride * p, len, nbits, lbits, one, nullptr);
    });
  c.reset_staging();
  API_END
}

}  // extern "C"
