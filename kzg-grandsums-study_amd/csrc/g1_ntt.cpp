// The G1 transform and what it is for (include/kgs.h; kernels and the device driver in
// g1ntt.hip, g1_ntt_run): kgs_g1_ntt / kgs_g1_ntt_device ([ffjs] G1.fft / G1.ifft), kgs_srs_lagrange (the
// Lagrange-basis SRS of the resident SRS) and kgs_commit_evals / kgs_commit_evals_device (a commitment
// straight from evaluations, over those bases).
//
// Also here: kgs_g1_mul_each and kgs_g1_mul_sum, the pointwise passes on their own. The openings built on all
// this (kgs_kzg_open*) are in kzg_open.cpp; what both files need of the transform's
// host side is declared in context.hpp.
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

// ------------------------------------------------------------------ shared with kzg_open.cpp (context.hpp)
void kgsi::fr_words(const Fr& x, uint32_t w[8]) { memcpy(w, x.v, 32); }

Fr kgsi::ntt_root(int logm, bool inverse) {
  const Fr w = host::fr_w_cached(logm);
  return inverse ? w.inverse() : w;
}

Fr kgsi::ninv_std(int logm) {
  uint64_t s[4];
  Fr::from_u64(1ull << logm).inverse().to_std(s);
  Fr r;
  memcpy(r.v, s, 32);
  return r;
}

G1NttWork kgsi::ntt_work(kgs_ctx& c, int logm) {
  const G1NttSizes z = g1_ntt_sizes(logm);
  G1NttWork w;
  w.xyzz = c.buf("gn_xyzz", z.xyzz);
  w.aff = c.buf("gn_aff", z.aff);
  w.scratch = c.buf("gn_scratch", z.scratch);
  w.tw = c.buf("gn_tw", z.tw);
  return w;
}

void kgsi::ntt_enqueue(kgs_ctx& c, uint32_t* out, const uint32_t* in, int logm, bool inverse, const Fr* scale_words) {
  const G1NttWork w = ntt_work(c, logm);
  uint32_t root[8], sc[8];
  fr_words(ntt_root(logm, inverse), root);
  if (scale_words) fr_words(*scale_words, sc);
  g1_ntt_run(c.st, w, out, in, logm, root, scale_words ? sc : nullptr, G1NTT_MAP_AUTO);
  check_launch();
}

void kgsi::check_whole_srs(const kgs_ctx& c, const char* fn) {
  if (c.srs_power < 0 || !c.srs) throw KgsError(KGS_E_SRS, "no SRS loaded");
  if (c.srs_slice_world > 1)
    throw KgsError(KGS_E_ARG, std::string(fn) + " needs the whole SRS: this context holds a rank's slice of it.");
}

void kgsi::check_lagrange(const kgs_ctx& c, int nbits, const char* fn) {
  check_plain_ctx(c, fn);
  if (nbits < 0 || nbits > G1_NTT_LOG_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " + std::to_string(G1_NTT_LOG_MAX));
  check_whole_srs(c, fn);
  if (nbits > c.nbits_max || (1ull << nbits) > c.tb.npts)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits = " + std::to_string(nbits) + " is above the nbits_max = " +
                                  std::to_string(c.nbits_max) + " the SRS was loaded for.");
}

namespace {

constexpr uint64_t G1_MUL_EACH_MAX = 1ull << 26;

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
  check_plain_ctx(*ctx, "kgs_g1_ntt");
  HC(hipSetDevice(ctx->device));
  g1_ntt_gpu(*ctx, in, out, device, logm, inverse != 0);
  API_END
}

// The cached row of (the context's SRS, nbits), built on first use: the inverse transform of the first
// 2^nbits points of table row 0, scaled by 2^256 / n, in msm_points_run's form. The caller holds the
// context and has checked it (check_lagrange); cached under srs_row_cached's rule.
std::shared_ptr<SrsRow> lagrange_row(kgs_ctx& c, int nbits) {
  return srs_row_cached(c, c.srs->lagrange, nbits, [&] {
    const uint64_t n = 1ull << nbits;
    auto row = SrsRow::make(c.device, n, 64 * n);
    uint32_t* in = c.buf("gn_io", 64 * n);
    launch_g1_from29(c.st, in, c.tb.table, n);
    const Fr scale = Fr::from_u64(n).inverse();  // its Montgomery words: the standard form of 2^256 / n
    ntt_enqueue(c, row->p, in, nbits, true, &scale);
    msm_points_row29(c.st, row->p, n);
    check_launch();
    return row;
  });
}

void commit_evals_gpu(kgs_ctx& c, const void* evals, bool device, int nbits, uint8_t out[64]) {
  DrainOnError drain(&c);
  const uint64_t n = 1ull << nbits;
  const std::shared_ptr<SrsRow> row = lagrange_row(c, nbits);
  const uint32_t* sc = (const uint32_t*)evals;
  if (!device) {
    uint32_t* d = c.buf("mp_scal", 32 * n);
    HC(hipMemcpyAsync(d, evals, 32 * n, hipMemcpyHostToDevice, c.st));
    sc = d;
  }
  msm_points_over_row(c, row->p, sc, n, 0, out);
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
  check_plain_ctx(*ctx, fn);
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
  check_plain_ctx(*ctx, fn);
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


}  // namespace

extern "C" {

int kgs_g1_mul_each(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t n, uint8_t* out_lem) {
  return g1_mul_each_entry(ctx, points_lem, scalars_std, n, out_lem, false);
}

int kgs_g1_mul_each_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t n,
                           void* d_out_lem) {
  return g1_mul_each_entry(ctx, d_points_lem, d_scalars_std, n, d_out_lem, true);
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
  const std::shared_ptr<SrsRow> row = lagrange_row(*ctx, nbits);
  if (out_lem) {
    const uint64_t n = 1ull << nbits;
    uint32_t* tmp = ctx->buf("gn_io", 64 * n);
    launch_g1_from29(ctx->st, tmp, row->p, n);
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
  check_plain_ctx(*ctx, "kgs_bench_g1_ntt");
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  kgs_ctx& c = *ctx;
  const G1NttWork w = ntt_work(c, logm);
  uint32_t root[8], sc[8];
  fr_words(ntt_root(logm, what == 1), root);
  fr_words(ninv_std(logm), sc);
  EventTimer timer;
  for (int r = -1; r < reps; r++) {  // r == -1: warm-up
    const double t = timer.ms(c.st, [&] {
      if (what == 2)
        launch_g1_scale(c.st, w, (uint32_t*)d_out, (const uint32_t*)d_in, 1ull << logm, sc);
      else
        g1_ntt_run(c.st, w, (uint32_t*)d_out, (const uint32_t*)d_in, logm, root, what == 1 ? sc : nullptr, mapping);
    });
    if (r >= 0) ms[r] = t;
  }
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
