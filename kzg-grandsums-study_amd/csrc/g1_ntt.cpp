// The G1 transform and what it is for (include/kgs.h; kernels and the device driver in
// g1ntt.hip, g1_ntt_run): kgs_g1_ntt / kgs_g1_ntt_device ([ffjs] G1.fft / G1.ifft), kgs_srs_lagrange (the
// Lagrange-basis SRS of the resident SRS) and kgs_commit_evals / kgs_commit_evals_device (a commitment
// straight from evaluations, over those bases).
//
// Further down: the openings over the whole resident SRS, kgs_kzg_open_all (§19), kgs_kzg_open_cosets (§20) and
// kgs_kzg_open_cosets_many (§23: §20's pipeline with a polynomial dimension in every stage), with their caches
// and timing helpers.
//
// Host: argument checks, the root and the scaling constant, the call's own device buffers ("gn_*" in the
// context's pool, grown on demand, g1_ntt_sizes), the per-device cache of Lagrange rows on the SrsTables
// entry, and for ctx == NULL the transform itself with the host curve code. Nothing of the prover's
// state is touched: the window tables are read, never written.
//
// kgs_srs_lagrange reads table row 0, which holds rho * P_i (rho = 2^-256 mod r, msm.hip) with
// coordinates as x * 2^261. The coordinates go back to the 2^256 form in one pass (launch_g1_from29);
// rho^-1 = 2^256 is folded into the inverse transform's final scaling, 2^256 / n instead of 1 / n, whose
// standard form is the Montgomery form of 1 / n word for word: no extra pass over the points and no second
// read of the ptau file.
#include <mutex>

#include "context.hpp"
#include "verify_linear.hpp"

namespace {

constexpr int G1_NTT_LOG_MAX = 24;

void fr_words(const Fr& x, uint32_t w[8]) { memcpy(w, x.v, 32); }

Fr ntt_root(int logm, bool inverse) {
  const Fr w = host::fr_w_cached(logm);
  return inverse ? w.inverse() : w;
}

// the transform with the host curve code: bit reversal, then the stages of g1ntt.hip
void g1_ntt_host(const uint8_t* in, uint8_t* out, int logm, bool inverse) {
  const size_t n = (size_t)1 << logm;
  std::vector<host::G1> a(n);
  for (size_t i = 0; i < n; i++) {
    size_t j = 0;
    for (int b = 0; b < logm; b++) j |= ((i >> b) & 1) << (logm - 1 - b);
    a[j] = host::G1::from_affine_lem(in + 64 * i);
  }
  const Fr w = ntt_root(logm, inverse);
  for (size_t h = 1; h < n; h *= 2) {
    Fr wh = w;  // omega_{2h} = omega_n^(n / 2h)
    for (size_t k = 2 * h; k < n; k *= 2) wh = wh.sqr();
    Fr tw = Fr::one();
    for (size_t t = 0; t < h; t++) {
      for (size_t g = 0; g < n; g += 2 * h) {
        const host::G1 T = t ? a[g + t + h].mul(tw) : a[g + t + h];
        const host::G1 A = a[g + t];
        a[g + t] = A.add(T);
        a[g + t + h] = A.add(T.neg());
      }
      tw = tw * wh;
    }
  }
  if (inverse && n > 1) {
    const Fr ninv = Fr::from_u64(n).inverse();
    for (size_t i = 0; i < n; i++) a[i] = a[i].mul(ninv);
  }
  for (size_t i = 0; i < n; i++) a[i].to_affine_lem(out + 64 * i);
}

G1NttWork ntt_work(kgs_ctx& c, int logm) {
  const G1NttSizes z = g1_ntt_sizes(logm);
  G1NttWork w;
  w.xyzz = c.buf("gn_xyzz", z.xyzz);
  w.aff = c.buf("gn_aff", z.aff);
  w.scratch = c.buf("gn_scratch", z.scratch);
  w.tw = c.buf("gn_tw", z.tw);
  return w;
}

// the transform on the main stream (not synchronised); scale: nullptr, or the standard-form factor
void ntt_enqueue(kgs_ctx& c, uint32_t* out, const uint32_t* in, int logm, bool inverse, const Fr* scale_words) {
  const G1NttWork w = ntt_work(c, logm);
  uint32_t root[8], sc[8];
  fr_words(ntt_root(logm, inverse), root);
  if (scale_words) fr_words(*scale_words, sc);
  g1_ntt_run(c.st, w, out, in, logm, root, scale_words ? sc : nullptr, G1NTT_MAP_AUTO);
  check_launch();
}

// 1 / n as the standard-form words the kernels take
Fr ninv_std(int logm) {
  uint64_t s[4];
  Fr::from_u64(1ull << logm).inverse().to_std(s);
  Fr r;
  memcpy(r.v, s, 32);
  return r;
}

void g1_ntt_gpu(kgs_ctx& c, const void* in, void* out, bool device, int logm, bool inverse) {
  DrainOnError drain(&c);
  const uint64_t n = 1ull << logm;
  const Fr ninv = ninv_std(logm);
  const Fr* scale = inverse && logm ? &ninv : nullptr;
  if (device) {
    ntt_enqueue(c, (uint32_t*)out, (const uint32_t*)in, logm, inverse, scale);
    HC(hipStreamSynchronize(c.st));
    return;
  }
  uint32_t* io = c.buf("gn_io", 64 * n);
  HC(hipMemcpyAsync(io, in, 64 * n, hipMemcpyHostToDevice, c.st));
  ntt_enqueue(c, io, io, logm, inverse, scale);
  HC(hipMemcpyAsync(out, io, 64 * n, hipMemcpyDeviceToHost, c.st));
  HC(hipStreamSynchronize(c.st));
}

// the common refusals of the calls that take a context (after the mutex is held)
void check_ctx(const kgs_ctx& c, const char* fn) {
  if (c.group) throw KgsError(KGS_E_ARG, std::string(fn) + " does not run on a context attached to a rank group.");
  if (c.shard_world > 1)
    throw KgsError(KGS_E_ARG, std::string(fn) + " does not run on a context with MSM sharding (kgs_ctx_set_shard).");
}

int g1_ntt_entry(kgs_ctx_t* ctx, const void* in, void* out, bool device, int logm, int inverse) {
  API_BEGIN
  if (logm < 0 || logm > G1_NTT_LOG_MAX)
    throw KgsError(KGS_E_ARG, "kgs_g1_ntt: logm must be in 0 .. " + std::to_string(G1_NTT_LOG_MAX));
  if (!in || !out) throw KgsError(KGS_E_ARG, "kgs_g1_ntt: NULL argument");
  if (!ctx) {
    if (device) throw KgsError(KGS_E_ARG, "kgs_g1_ntt_device: NULL ctx");
    g1_ntt_host((const uint8_t*)in, (uint8_t*)out, logm, inverse != 0);
    return KGS_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_ctx(*ctx, "kgs_g1_ntt");
  HC(hipSetDevice(ctx->device));
  g1_ntt_gpu(*ctx, in, out, device, logm, inverse != 0);
  API_END
}

// The context's SRS can serve 2^nbits Lagrange bases, or the refusal of kgs.h.
void check_lagrange(const kgs_ctx& c, int nbits, const char* fn) {
  check_ctx(c, fn);
  if (nbits < 0 || nbits > G1_NTT_LOG_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " + std::to_string(G1_NTT_LOG_MAX));
  if (c.srs_power < 0 || !c.srs) throw KgsError(KGS_E_SRS, "no SRS loaded");
  if (c.srs_slice_world > 1)
    throw KgsError(KGS_E_ARG, std::string(fn) + " needs the whole SRS: this context holds a rank's slice of it.");
  if (nbits > c.nbits_max || (1ull << nbits) > c.tb.npts)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits = " + std::to_string(nbits) + " is above the nbits_max = " +
                                  std::to_string(c.nbits_max) + " the SRS was loaded for.");
}

std::shared_ptr<LagrangeRow> lagrange_find(const kgs_ctx& c, int nbits) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = c.srs->lagrange.find(nbits);
  return it == c.srs->lagrange.end() ? nullptr : it->second;
}

// The cached row of (the context's SRS, nbits), built on first use: the inverse transform of the first
// 2^nbits points of table row 0, scaled by 2^256 / n, in msm_points_run's form. The caller holds the
// context and has checked it (check_lagrange). Ends with the main stream drained when it built.
std::shared_ptr<LagrangeRow> lagrange_row(kgs_ctx& c, int nbits) {
  if (auto hit = lagrange_find(c, nbits)) return hit;
  DrainOnError drain(&c);
  const uint64_t n = 1ull << nbits;
  auto row = std::make_shared<LagrangeRow>();
  row->device = c.device;
  row->n = n;
  HC(dev_malloc((void**)&row->row29, 64 * n));
  uint32_t* in = c.buf("gn_io", 64 * n);
  launch_g1_from29(c.st, in, c.tb.table, n);
  const Fr scale = Fr::from_u64(n).inverse();  // its Montgomery words: the standard form of 2^256 / n
  ntt_enqueue(c, row->row29, in, nbits, true, &scale);
  msm_points_row29(c.st, row->row29, n);
  check_launch();
  HC(hipStreamSynchronize(c.st));
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto& slot = c.srs->lagrange[nbits];
  if (!slot) slot = row;  // else: built concurrently by another context and published first; ours is released
  return slot;
}

void commit_evals_gpu(kgs_ctx& c, const void* evals, bool device, int nbits, uint8_t out[64]) {
  DrainOnError drain(&c);
  const uint64_t n = 1ull << nbits;
  const std::shared_ptr<LagrangeRow> row = lagrange_row(c, nbits);
  const uint32_t* sc = (const uint32_t*)evals;
  if (!device) {
    uint32_t* d = c.buf("mp_scal", 32 * n);
    HC(hipMemcpyAsync(d, evals, 32 * n, hipMemcpyHostToDevice, c.st));
    sc = d;
  }
  msm_points_over_row(c, row->row29, sc, n, 0, out);
}

int commit_evals_entry(kgs_ctx_t* ctx, const void* evals, bool device, int nbits, uint8_t out[64]) {
  API_BEGIN
  const char* fn = "kgs_commit_evals";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  if (!evals || !out) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_lagrange(*ctx, nbits, fn);
  HC(hipSetDevice(ctx->device));
  commit_evals_gpu(*ctx, evals, device, nbits, out);
  API_END
}

// ------------------------------------------------------------------ openings
constexpr int KZG_OPEN_ALL_LOG_MAX = G1_NTT_LOG_MAX - 1;  // the Toeplitz product transforms 2n points
constexpr uint64_t G1_MUL_EACH_MAX = 1ull << 26;

// the refusals of the calls over the whole resident SRS, in kgs_srs_lagrange's words
void check_open_all(const kgs_ctx& c, int nbits, const char* fn) {
  check_ctx(c, fn);
  if (nbits < 0 || nbits > KZG_OPEN_ALL_LOG_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " + std::to_string(KZG_OPEN_ALL_LOG_MAX));
  check_lagrange(c, nbits, fn);
}

// The row of (the context's SRS, nbits), enqueued on the main stream and not yet published: the forward
// transform of size 2n of x = (s_{n-2}, .., s_0, identity x (n + 1)) read off table row 0, scaled by 1 / 2n.
// Row 0's rho = 2^-256 stays on the points: the pointwise pass multiplies by Montgomery words, which
// carry 2^256.
std::shared_ptr<FkRow> fk_build(kgs_ctx& c, int nbits) {
  const uint64_t n = 1ull << nbits;
  auto row = std::make_shared<FkRow>();
  row->device = c.device;
  row->n = n;
  HC(dev_malloc((void**)&row->xhat, 128 * n));
  uint32_t* x = c.buf("gn_io", 128 * n);
  HC(hipMemsetAsync(x, 0, 128 * n, c.st));
  launch_g1_from29(c.st, x, c.tb.table, n - 1, true);
  const Fr scale = ninv_std(nbits + 1);
  ntt_enqueue(c, row->xhat, x, nbits + 1, false, &scale);
  return row;
}

// The cached row, built on first use under the Lagrange row's rules (lagrange_row)
std::shared_ptr<FkRow> fk_row(kgs_ctx& c, int nbits) {
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = c.srs->fk.find(nbits);
    if (it != c.srs->fk.end()) return it->second;
  }
  DrainOnError drain(&c);
  const std::shared_ptr<FkRow> row = fk_build(c, nbits);
  HC(hipStreamSynchronize(c.st));
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto& slot = c.srs->fk[nbits];
  if (!slot) slot = row;  // else: built concurrently by another context and published first; ours is released
  return slot;
}

// u = (the Fr transform's output words) x (the cached points), pointwise, affine, into w.aff
void fk_pointwise(kgs_ctx& c, const G1NttWork& w, const FkRow& row, const uint32_t* chat_words) {
  launch_g1_mul_each(c.st, w.xyzz, row.xhat, chat_words, 2 * row.n, false);
  launch_batch_affine(c.st, w.aff, w.xyzz, w.scratch, 2 * row.n);
}

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
  const std::shared_ptr<FkRow> row = fk_row(c, nbits);
  if (logm > c.logM) ensure_domain(c, logm);
  uint32_t* sa = c.buf("fk_fr", 64 * n);
  uint32_t* sb = c.buf("fk_chat", 64 * n);
  uint32_t* h = c.buf("fk_h", 64 * n);
  const G1NttWork w = ntt_work(c, logm);  // serves the transform of size n too
  uint32_t root[8];
  // c^ = the Fr transform of size 2n of the zero-padded coefficients, natural order
  ntt_dif(c.st, sa, d_coef, len, logm, nullptr, c.tw_fwd, c.logM);
  launch_bitrev_copy(c.st, sb, sa, logm);
  fk_pointwise(c, w, *row, sb);
  // u = the inverse transform without its 1 / 2n (the row has it), in place in w.aff; h_k = u_{n-1+k}
  fr_words(ntt_root(logm, true), root);
  g1_ntt_run(c.st, w, w.aff, w.aff, logm, root, nullptr, G1NTT_MAP_AUTO);
  if (n > 1) HC(hipMemcpyAsync(h, w.aff + 16 * (n - 1), 64 * (n - 1), hipMemcpyDeviceToDevice, c.st));
  HC(hipMemsetAsync(h + 16 * (n - 1), 0, 64, c.st));
  fr_words(ntt_root(nbits, false), root);
  g1_ntt_run(c.st, w, d_proofs, h, nbits, root, nullptr, G1NTT_MAP_AUTO);
  if (d_evals) {
    ntt_dif(c.st, sa, d_coef, len, nbits, nullptr, c.tw_fwd, c.logM);
    launch_bitrev_copy(c.st, d_evals, sa, nbits);
  }
  check_launch();
}

int kzg_open_all_entry(kgs_ctx_t* ctx, const void* coef, uint64_t len, int nbits, void* proofs, void* evals,
                       bool device) {
  API_BEGIN
  const char* fn = "kgs_kzg_open_all";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_open_all(*ctx, nbits, fn);
  const uint64_t n = 1ull << nbits;
  if (len > n)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": len = " + std::to_string(len) + " coefficients do not fit the domain of 2^" +
                                  std::to_string(nbits) + " points.");
  if (!proofs || (len && !coef)) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  if (device) {
    kzg_open_all_run(c, (const uint32_t*)coef, len, nbits, (uint32_t*)proofs, (uint32_t*)evals);
  } else {
    uint32_t* dc = c.buf("fk_coef", 32 * (len ? len : 1));
    uint32_t* dp = c.buf("fk_out", 64 * n);
    uint32_t* de = evals ? c.buf("fk_ev", 32 * n) : nullptr;
    if (len) HC(hipMemcpyAsync(dc, coef, 32 * len, hipMemcpyHostToDevice, c.st));
    kzg_open_all_run(c, dc, len, nbits, dp, de);
    HC(hipMemcpyAsync(proofs, dp, 64 * n, hipMemcpyDeviceToHost, c.st));
    if (evals) HC(hipMemcpyAsync(evals, de, 32 * n, hipMemcpyDeviceToHost, c.st));
  }
  c.reset_staging();
  API_END
}

// ------------------------------------------------------------------ coset openings
// The rows of (the context's SRS, nbits, lbits >= 1, m = n / l >= 2), enqueued on the main stream and not yet
// published. X_{j l + r} = x^(r)_j = s_{(m-2-j) l + r} for j <= m - 2 and the identity above: the first n - l
// points of table row 0 with their blocks of l reversed. The l transforms of size 2m of the stride-l
// subsequences of X are the first log2(2m) stages of the transform of size 2n (g1_ntt_run, `stages`), then
// one uniform scaling by 1 / 2m. Block b of the result holds the row of residue bitrev_l(b): kzg_open_cosets_run
// lays the Fr side out in the same order (launch_coset_rows). Row 0's rho stays on the points, as in fk_build.
std::shared_ptr<FkRow> coset_build(kgs_ctx& c, int nbits, int lbits) {
  const uint64_t n = 1ull << nbits, l = 1ull << lbits;
  auto row = std::make_shared<FkRow>();
  row->device = c.device;
  row->n = n;
  HC(dev_malloc((void**)&row->xhat, 128 * n));
  uint32_t* x = c.buf("gn_io", 128 * n);
  HC(hipMemsetAsync(x, 0, 128 * n, c.st));
  launch_g1_from29(c.st, x, c.tb.table, n - l, true, lbits);
  const int logm2 = nbits - lbits + 1;
  const G1NttWork w = ntt_work(c, nbits + 1);
  uint32_t root[8], sc[8];
  fr_words(ntt_root(nbits + 1, false), root);
  fr_words(ninv_std(logm2), sc);
  g1_ntt_run(c.st, w, row->xhat, x, nbits + 1, root, sc, G1NTT_MAP_AUTO, logm2);
  check_launch();
  return row;
}

// The cached rows, built on first use under the Lagrange row's rules (lagrange_row, fk_row)
std::shared_ptr<FkRow> coset_row(kgs_ctx& c, int nbits, int lbits) {
  const std::pair<int, int> key(nbits, lbits);
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = c.srs->fk_cosets.find(key);
    if (it != c.srs->fk_cosets.end()) return it->second;
  }
  DrainOnError drain(&c);
  const std::shared_ptr<FkRow> row = coset_build(c, nbits, lbits);
  HC(hipStreamSynchronize(c.st));
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto& slot = c.srs->fk_cosets[key];
  if (!slot) slot = row;  // else: built concurrently by another context and published first; ours is released
  return slot;
}

// u^_i = sum_r (the Fr transforms' output words)_{r, i} x (the cached points)_{r, i}, i < 2m, affine, into w.aff
void coset_pointwise(kgs_ctx& c, const G1NttWork& w, const FkRow& row, const uint32_t* chat_words, int lbits,
                     int group = G1_MUL_SUM_GROUP) {
  const uint64_t cols = (2 * row.n) >> lbits;
  launch_g1_mul_sum(c.st, w.xyzz, row.xhat, chat_words, 1ull << lbits, cols, false, group);
  launch_batch_affine(c.st, w.aff, w.xyzz, w.scratch, cols);
}

// the two G1 transforms of a coset call: u = the unscaled inverse of size 2m in place in w.aff, h = u_{m-1 ..
// 2m-3} and one identity, the forward transform of size m of h into d_proofs
void coset_transforms(kgs_ctx& c, const G1NttWork& w, int logm, uint32_t* h, uint32_t* d_proofs) {
  const uint64_t m = 1ull << logm;
  uint32_t root[8];
  fr_words(ntt_root(logm + 1, true), root);
  g1_ntt_run(c.st, w, w.aff, w.aff, logm + 1, root, nullptr, G1NTT_MAP_AUTO);
  HC(hipMemcpyAsync(h, w.aff + 16 * (m - 1), 64 * (m - 1), hipMemcpyDeviceToDevice, c.st));
  HC(hipMemsetAsync(h + 16 * (m - 1), 0, 64, c.st));
  fr_words(ntt_root(logm, false), root);
  g1_ntt_run(c.st, w, d_proofs, h, logm, root, nullptr, G1NTT_MAP_AUTO);
}

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
    const std::shared_ptr<FkRow> row = coset_row(c, nbits, lbits);
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

int kzg_open_cosets_entry(kgs_ctx_t* ctx, const void* coef, uint64_t len, int nbits, int lbits, void* proofs, void* evals,
                          bool device) {
  API_BEGIN
  const char* fn = "kgs_kzg_open_cosets";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_open_all(*ctx, nbits, fn);
  if (lbits < 0 || lbits > nbits)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": lbits must be in 0 .. nbits = " + std::to_string(nbits));
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  if (len > n)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": len = " + std::to_string(len) + " coefficients do not fit the domain of 2^" +
                                  std::to_string(nbits) + " points.");
  if (!proofs || (len && !coef)) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  if (device) {
    kzg_open_cosets_run(c, (const uint32_t*)coef, len, nbits, lbits, (uint32_t*)proofs, (uint32_t*)evals);
  } else {
    uint32_t* dc = c.buf("fk_coef", 32 * (len ? len : 1));
    uint32_t* dp = c.buf("fk_out", 64 * m);
    uint32_t* de = evals ? c.buf("fk_ev", 32 * n) : nullptr;
    if (len) HC(hipMemcpyAsync(dc, coef, 32 * len, hipMemcpyHostToDevice, c.st));
    kzg_open_cosets_run(c, dc, len, nbits, lbits, dp, de);
    HC(hipMemcpyAsync(proofs, dp, 64 * m, hipMemcpyDeviceToHost, c.st));
    if (evals) HC(hipMemcpyAsync(evals, de, 32 * n, hipMemcpyDeviceToHost, c.st));
  }
  c.reset_staging();
  API_END
}

// ------------------------------------------------------------------ coset openings of many polynomials
constexpr uint64_t KZG_MANY_MAX_SLOTS = 1ull << 24;  // polys * n

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
void cosets_many_pointwise(kgs_ctx& c, const CosetsMany& q, const FkRow& row) {
  launch_g1_mul_sum_many(c.st, q.w.xyzz, row.xhat, q.chat, q.l, q.polys, 2 * q.m);
  launch_batch_affine(c.st, q.w.aff, q.w.xyzz, q.w.scratch, 2 * q.m * q.polys);
}

// coset_transforms for all the polynomials: the unscaled inverses of size 2m in place in q.w.aff, the slices, the
// forward transforms of size m into d_proofs
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
  std::shared_ptr<FkRow> row;
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

// the refusals of kgs_kzg_open_cosets_many beyond a NULL context (the caller holds the context)
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

int kzg_open_cosets_many_entry(kgs_ctx_t* ctx, const void* coef, uint64_t polys, uint64_t stride, uint64_t len, int nbits,
                               int lbits, void* proofs, void* evals, bool device) {
  API_BEGIN
  const char* fn = "kgs_kzg_open_cosets_many";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  if (!polys) return KGS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_cosets_many(*ctx, polys, stride, len, nbits, lbits, fn);
  if (!proofs) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL proofs buffer");
  if (len && !coef) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL coefficient buffer");
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  if (device) {
    kzg_open_cosets_many_run(c, (const uint32_t*)coef, polys, stride, len, nbits, lbits, (uint32_t*)proofs, (uint32_t*)evals);
  } else {
    uint32_t* dc = c.buf("km_coef", 32 * (len ? len * polys : 1));  // packed: the gaps stay on the host
    uint32_t* dp = c.buf("km_out", 64 * m * polys);
    uint32_t* de = evals ? c.buf("km_ev", 32 * n * polys) : nullptr;
    if (len && stride == len)
      HC(hipMemcpyAsync(dc, coef, 32 * len * polys, hipMemcpyHostToDevice, c.st));
    else if (len)
      HC(hipMemcpy2DAsync(dc, 32 * len, coef, 32 * stride, 32 * len, polys, hipMemcpyHostToDevice, c.st));
    kzg_open_cosets_many_run(c, dc, polys, len, len, nbits, lbits, dp, de);
    HC(hipMemcpyAsync(proofs, dp, 64 * m * polys, hipMemcpyDeviceToHost, c.st));
    if (evals) HC(hipMemcpyAsync(evals, de, 32 * n * polys, hipMemcpyDeviceToHost, c.st));
  }
  c.reset_staging();
  API_END
}

int g1_mul_sum_entry(kgs_ctx_t* ctx, const void* points, const void* scalars, uint64_t rows, uint64_t cols, void* out,
                     bool device) {
  API_BEGIN
  const char* fn = "kgs_g1_mul_sum";
  if (!rows) throw KgsError(KGS_E_ARG, std::string(fn) + ": rows must be at least 1");
  if (rows > G1_MUL_EACH_MAX || cols > G1_MUL_EACH_MAX || rows * cols > G1_MUL_EACH_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": at most 2^26 terms");
  if (cols && (!points || !scalars || !out)) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (!ctx) {
    if (device) throw KgsError(KGS_E_ARG, "kgs_g1_mul_sum_device: NULL ctx");
    std::vector<uint8_t> p(64 * rows), s(32 * rows);
    for (uint64_t i = 0; i < cols; i++) {  // a column's terms side by side, then the host MSM's segment sum
      for (uint64_t r = 0; r < rows; r++) {
        memcpy(p.data() + 64 * r, (const uint8_t*)points + 64 * (r * cols + i), 64);
        memcpy(s.data() + 32 * r, (const uint8_t*)scalars + 32 * (r * cols + i), 32);
      }
      host::g1_lincomb_segment(p.data(), s.data(), rows).to_affine_lem((uint8_t*)out + 64 * i);
    }
    return KGS_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_ctx(*ctx, fn);
  if (!cols) return KGS_OK;
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  const uint64_t n = rows * cols;
  uint32_t* xyzz = c.buf("gn_xyzz", 128 * n);
  uint32_t* scratch = c.buf("gn_scratch", 32 * cols);
  const uint32_t *dp = (const uint32_t*)points, *ds = (const uint32_t*)scalars;
  uint32_t* dout = (uint32_t*)out;
  if (!device) {
    uint32_t* io = c.buf("gn_io", 64 * n);
    uint32_t* sc = c.buf("fk_chat", 32 * n);
    HC(hipMemcpyAsync(io, points, 64 * n, hipMemcpyHostToDevice, c.st));
    HC(hipMemcpyAsync(sc, scalars, 32 * n, hipMemcpyHostToDevice, c.st));
    dp = io;
    ds = sc;
    dout = c.buf("fk_out", 64 * cols);
  }
  launch_g1_mul_sum(c.st, xyzz, dp, ds, rows, cols, true);
  launch_batch_affine(c.st, dout, xyzz, scratch, cols);
  check_launch();
  if (!device) HC(hipMemcpyAsync(out, dout, 64 * cols, hipMemcpyDeviceToHost, c.st));
  HC(hipStreamSynchronize(c.st));
  API_END
}

int g1_mul_each_entry(kgs_ctx_t* ctx, const void* points, const void* scalars, uint64_t n, void* out, bool device) {
  API_BEGIN
  const char* fn = "kgs_g1_mul_each";
  if (n > G1_MUL_EACH_MAX) throw KgsError(KGS_E_ARG, std::string(fn) + ": at most 2^26 points");
  if (n && (!points || !scalars || !out)) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (!ctx) {
    if (device) throw KgsError(KGS_E_ARG, "kgs_g1_mul_each_device: NULL ctx");
    for (uint64_t i = 0; i < n; i++)  // the group has order r: the integer multiple is the multiple mod r
      host::g1_lincomb_segment((const uint8_t*)points + 64 * i, (const uint8_t*)scalars + 32 * i, 1)
          .to_affine_lem((uint8_t*)out + 64 * i);
    return KGS_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_ctx(*ctx, fn);
  if (!n) return KGS_OK;
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  uint32_t* xyzz = c.buf("gn_xyzz", 128 * n);
  uint32_t* scratch = c.buf("gn_scratch", 32 * n);
  const uint32_t *dp = (const uint32_t*)points, *ds = (const uint32_t*)scalars;
  uint32_t* dout = (uint32_t*)out;
  if (!device) {
    uint32_t* io = c.buf("gn_io", 64 * n);
    uint32_t* sc = c.buf("fk_chat", 32 * n);
    HC(hipMemcpyAsync(io, points, 64 * n, hipMemcpyHostToDevice, c.st));
    HC(hipMemcpyAsync(sc, scalars, 32 * n, hipMemcpyHostToDevice, c.st));
    dp = dout = io;
    ds = sc;
  }
  launch_g1_mul_each(c.st, xyzz, dp, ds, n, true);
  launch_batch_affine(c.st, dout, xyzz, scratch, n);
  check_launch();
  if (!device) HC(hipMemcpyAsync(out, dout, 64 * n, hipMemcpyDeviceToHost, c.st));
  HC(hipStreamSynchronize(c.st));
  API_END
}

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

int kgs_g1_mul_each(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t n, uint8_t* out_lem) {
  return g1_mul_each_entry(ctx, points_lem, scalars_std, n, out_lem, false);
}

int kgs_g1_mul_each_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t n,
                           void* d_out_lem) {
  return g1_mul_each_entry(ctx, d_points_lem, d_scalars_std, n, d_out_lem, true);
}

int kgs_kzg_open(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t z_mont[32], uint8_t y_mont[32],
                 uint8_t proof_lem[64]) {
  API_BEGIN
  const char* fn = "kgs_kzg_open";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  if (!z_mont || !y_mont || !proof_lem || (len && !coef_mont)) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_ctx(*ctx, fn);
  if (ctx->srs_power < 0 || !ctx->srs) throw KgsError(KGS_E_SRS, "no SRS loaded");
  if (ctx->srs_slice_world > 1)
    throw KgsError(KGS_E_ARG, std::string(fn) + " needs the whole SRS: this context holds a rank's slice of it.");
  if (len > ctx->tb.npts + 1) throw KgsError(KGS_E_SRS, "MSM larger than the resident SRS");
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  kzg_open_run(*ctx, coef_mont, len, Fr::from_bytes(z_mont), y_mont, proof_lem);
  API_END
}

int kgs_kzg_open_all(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, int nbits, uint8_t* proofs_lem,
                     uint8_t* evals_mont) {
  return kzg_open_all_entry(ctx, coef_mont, len, nbits, proofs_lem, evals_mont, false);
}

int kgs_kzg_open_all_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, void* d_proofs_lem,
                            void* d_evals_mont) {
  return kzg_open_all_entry(ctx, d_coef_mont, len, nbits, d_proofs_lem, d_evals_mont, true);
}

int kgs_kzg_open_cosets(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, int nbits, int lbits, uint8_t* proofs_lem,
                        uint8_t* evals_mont) {
  return kzg_open_cosets_entry(ctx, coef_mont, len, nbits, lbits, proofs_lem, evals_mont, false);
}

int kgs_kzg_open_cosets_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t len, int nbits, int lbits,
                               void* d_proofs_lem, void* d_evals_mont) {
  return kzg_open_cosets_entry(ctx, d_coef_mont, len, nbits, lbits, d_proofs_lem, d_evals_mont, true);
}

int kgs_kzg_open_cosets_cached(kgs_ctx_t* ctx, int nbits, int lbits) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "kgs_kzg_open_cosets_cached: NULL ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->srs) return 0;
  std::lock_guard<std::mutex> reg(g_reg_mu);
  return lbits ? (int)ctx->srs->fk_cosets.count({nbits, lbits}) : (int)ctx->srs->fk.count(nbits);
  API_END
}

int kgs_kzg_open_cosets_many(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t polys, uint64_t stride, uint64_t len,
                             int nbits, int lbits, uint8_t* proofs_lem, uint8_t* evals_mont) {
  return kzg_open_cosets_many_entry(ctx, coef_mont, polys, stride, len, nbits, lbits, proofs_lem, evals_mont, false);
}

int kgs_kzg_open_cosets_many_device(kgs_ctx_t* ctx, const void* d_coef_mont, uint64_t polys, uint64_t stride,
                                    uint64_t len, int nbits, int lbits, void* d_proofs_lem, void* d_evals_mont) {
  return kzg_open_cosets_many_entry(ctx, d_coef_mont, polys, stride, len, nbits, lbits, d_proofs_lem, d_evals_mont, true);
}

int kgs_g1_mul_sum(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t rows, uint64_t cols,
                   uint8_t* out_lem) {
  return g1_mul_sum_entry(ctx, points_lem, scalars_std, rows, cols, out_lem, false);
}

int kgs_g1_mul_sum_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t rows,
                          uint64_t cols, void* d_out_lem) {
  return g1_mul_sum_entry(ctx, d_points_lem, d_scalars_std, rows, cols, d_out_lem, true);
}

int kgs_g1_ntt(kgs_ctx_t* ctx, const uint8_t* points_lem, uint8_t* out_lem, int logm, int inverse) {
  return g1_ntt_entry(ctx, points_lem, out_lem, false, logm, inverse);
}

int kgs_g1_ntt_device(kgs_ctx_t* ctx, const void* d_points_lem, void* d_out_lem, int logm, int inverse) {
  return g1_ntt_entry(ctx, d_points_lem, d_out_lem, true, logm, inverse);
}

int kgs_srs_lagrange(kgs_ctx_t* ctx, int nbits, uint8_t* out_lem) {
  API_BEGIN
  const char* fn = "kgs_srs_lagrange";
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_lagrange(*ctx, nbits, fn);
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  const std::shared_ptr<LagrangeRow> row = lagrange_row(*ctx, nbits);
  if (out_lem) {
    const uint64_t n = 1ull << nbits;
    uint32_t* tmp = ctx->buf("gn_io", 64 * n);
    launch_g1_from29(ctx->st, tmp, row->row29, n);
    check_launch();
    HC(hipMemcpyAsync(out_lem, tmp, 64 * n, hipMemcpyDeviceToHost, ctx->st));
    HC(hipStreamSynchronize(ctx->st));
  }
  API_END
}

int kgs_commit_evals(kgs_ctx_t* ctx, const uint8_t* evals_std, int nbits, uint8_t out_lem[64]) {
  return commit_evals_entry(ctx, evals_std, false, nbits, out_lem);
}

int kgs_commit_evals_device(kgs_ctx_t* ctx, const void* d_evals_std, int nbits, uint8_t out_lem[64]) {
  return commit_evals_entry(ctx, d_evals_std, true, nbits, out_lem);
}

// ---- timing helpers of profiles/g1_ntt_time.py
int kgs_bench_g1_ntt(kgs_ctx_t* ctx, const void* d_in, void* d_out, int logm, int what, int mapping, int reps,
                     double* ms) {
  API_BEGIN
  if (!ctx || !d_in || !d_out || !ms) throw KgsError(KGS_E_ARG, "kgs_bench_g1_ntt: NULL argument");
  if (logm < 1 || logm > G1_NTT_LOG_MAX || what < 0 || what > 2 || mapping < G1NTT_MAP_AUTO ||
      mapping > G1NTT_MAP_WAVE || reps < 1)
    throw KgsError(KGS_E_ARG, "kgs_bench_g1_ntt: bad logm / what / mapping / reps");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_ctx(*ctx, "kgs_bench_g1_ntt");
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  kgs_ctx& c = *ctx;
  const G1NttWork w = ntt_work(c, logm);
  uint32_t root[8], sc[8];
  fr_words(ntt_root(logm, what == 1), root);
  fr_words(ninv_std(logm), sc);
  hipEvent_t e0, e1;
  HC(hipEventCreate(&e0));
  HC(hipEventCreate(&e1));
  for (int r = -1; r < reps; r++) {  // r == -1: warm-up
    HC(hipEventRecord(e0, c.st));
    if (what == 2)
      launch_g1_scale(c.st, w, (uint32_t*)d_out, (const uint32_t*)d_in, 1ull << logm, sc);
    else
      g1_ntt_run(c.st, w, (uint32_t*)d_out, (const uint32_t*)d_in, logm, root, what == 1 ? sc : nullptr, mapping);
    HC(hipEventRecord(e1, c.st));
    check_launch();
    HC(hipEventSynchronize(e1));
    float f = 0;
    HC(hipEventElapsedTime(&f, e0, e1));
    if (r >= 0) ms[r] = f;
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
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
  uint32_t* out = c.buf("fk_out", 64 * n);
  // every leg after one whole call: the row cached, the buffers grown, c^ in "fk_chat"
  kzg_open_all_run(c, (const uint32_t*)d_coef_mont, len, nbits, out, nullptr);
  HC(hipStreamSynchronize(c.st));
  const std::shared_ptr<FkRow> row = fk_row(c, nbits);
  const G1NttWork w = ntt_work(c, nbits + 1);
  const uint32_t* chat = c.buf("fk_chat", 64 * n);
  hipEvent_t e0, e1;
  HC(hipEventCreate(&e0));
  HC(hipEventCreate(&e1));
  for (int r = 0; r < reps; r++) {
    std::shared_ptr<FkRow> built;
    HC(hipEventRecord(e0, c.st));
    if (what == 0)
      kzg_open_all_run(c, (const uint32_t*)d_coef_mont, len, nbits, out, nullptr);
    else if (what == 1)
      built = fk_build(c, nbits);
    else
      fk_pointwise(c, w, *row, chat);
    HC(hipEventRecord(e1, c.st));
    check_launch();
    HC(hipEventSynchronize(e1));
    float f = 0;
    HC(hipEventElapsedTime(&f, e0, e1));
    ms[r] = f;
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
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
  uint32_t* out = c.buf("fk_out", 64 * m);
  // every leg after one whole call: the rows cached, the buffers grown, c^ in "fk_chat", u in "gn_aff" and h
  // in "fk_h" (the operands the transform legs run over: points of this polynomial, no periodic vector)
  kzg_open_cosets_run(c, (const uint32_t*)d_coef_mont, len, nbits, lbits, out, nullptr);
  HC(hipStreamSynchronize(c.st));
  const std::shared_ptr<FkRow> row = coset_row(c, nbits, lbits);
  const G1NttWork w = ntt_work(c, nbits + 1);
  const uint32_t* chat = c.buf("fk_chat", 64 * n);
  uint32_t* h = c.buf("fk_h", 64 * m);
  hipEvent_t e0, e1;
  HC(hipEventCreate(&e0));
  HC(hipEventCreate(&e1));
  for (int r = 0; r < reps; r++) {
    std::shared_ptr<FkRow> built;
    HC(hipEventRecord(e0, c.st));
    if (what == 0)
      kzg_open_cosets_run(c, (const uint32_t*)d_coef_mont, len, nbits, lbits, out, nullptr);
    else if (what == 1)
      built = coset_build(c, nbits, lbits);
    else if (what == 2)
      coset_pointwise(c, w, *row, chat, lbits);
    else if (what == 3)
      coset_transforms(c, w, nbits - lbits, h, out);
    else if (what == 4)
      launch_g1_mul_each(c.st, w.xyzz, row->xhat, chat, 2 * n, false);
    else
      coset_pointwise(c, w, *row, chat, lbits, 1);
    HC(hipEventRecord(e1, c.st));
    check_launch();
    HC(hipEventSynchronize(e1));
    float f = 0;
    HC(hipEventElapsedTime(&f, e0, e1));
    ms[r] = f;
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
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
  const std::shared_ptr<FkRow> row = coset_row(c, nbits, lbits);
  const CosetsMany q = cosets_many_plan(c, polys, stride, len, nbits, lbits);
  hipEvent_t e0, e1;
  HC(hipEventCreate(&e0));
  HC(hipEventCreate(&e1));
  for (int r = 0; r < reps; r++) {
    HC(hipEventRecord(e0, c.st));
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
    HC(hipEventRecord(e1, c.st));
    check_launch();
    HC(hipEventSynchronize(e1));
    float f = 0;
    HC(hipEventElapsedTime(&f, e0, e1));
    ms[r] = f;
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  c.reset_staging();
  API_END
}

int kgs_bench_coeff_commit(kgs_ctx_t* ctx, const void* d_evals_std, int nbits, uint8_t out_lem[64]) {
  API_BEGIN
  if (!ctx || !d_evals_std || !out_lem) throw KgsError(KGS_E_ARG, "kgs_bench_coeff_commit: NULL argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_lagrange(*ctx, nbits, "kgs_bench_coeff_commit");
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  kgs_ctx& c = *ctx;
  const uint64_t n = 1ull << nbits;
  c.reset_staging();
  uint32_t* a = c.buf("prim_a", 32 * n);
  uint32_t* b = c.buf("prim_b", 32 * n);
  launch_to_mont(c.st, a, (const uint32_t*)d_evals_std, n);
  intt_nat(c, b, a, nbits);
  Commit cm = commit_launch(c, b, n, 0);
  c.sync();
  commit_finish(c, cm, out_lem);
  c.reset_staging();
  API_END
}

}  // extern "C"
