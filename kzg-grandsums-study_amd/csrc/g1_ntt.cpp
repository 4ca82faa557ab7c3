// The G1 transform and what it is for (include/kgs.h; kernels and the device driver in
// g1ntt.hip, g1_ntt_run): kgs_g1_ntt / kgs_g1_ntt_device ([ffjs] G1.fft / G1.ifft), kgs_srs_lagrange (the
// Lagrange-basis SRS of the resident SRS) and kgs_commit_evals / kgs_commit_evals_device (a commitment
// straight from evaluations, over those bases).
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

}  // namespace

extern "C" {

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
