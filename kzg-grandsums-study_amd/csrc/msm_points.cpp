// Variable-base G1 MSM over arbitrary bases: kgs_msm_points, kgs_msm_points_device (include/kgs.h;
// DESIGN.md §17; kernels and the device driver in msm.hip, msm_points_run).
//
// Host: argument checks, the window, the call's own device buffers ("mp_*" in the context's pool, grown
// on demand, sized by msm_points_work_sizes(n, c)), and the finish: one Horner pass over the W * c bit-sum
// points the device returns, then the affine conversion. Nothing of the prover's state is touched: not
// the SRS tables, not mw / mw2 / work_npts, not the pinned staging. msm_points_over_row is the part after
// the bases' conversion; kgs_commit_evals (g1_ntt.cpp) runs it over the cached Lagrange row.
#include <mutex>

#include "context.hpp"
#include "verify_linear.hpp"

namespace {

constexpr uint64_t MSM_POINTS_MAX = 1ull << 26;

// The signed-digit recoding of a scalar s < r must not carry out of the top window: the top window's
// bits plus an incoming carry stay <= 2^(c-1). r < 2^254 and W * c >= 255 make it so; checked here for
// every supported window from the top limb of r (bits 192 .. 255), not argued in a comment.
constexpr uint64_t R_TOP_LIMB = host::FR_MOD.p[3];
constexpr bool top_digit_fits(int c) {
  const int W = (255 + c - 1) / c, shift = (W - 1) * c;
  if (shift < 192 || shift > 255) return false;  // the top window must start inside the top limb
  return (R_TOP_LIMB >> (shift - 192)) + 1 <= (1ull << (c - 1));
}
constexpr bool top_digits_fit() {
  for (int c = MSM_POINTS_C_MIN; c <= MSM_POINTS_C_MAX; c++)
    if (!top_digit_fits(c)) return false;
  return true;
}
static_assert(top_digits_fit(), "a window in MSM_POINTS_C_MIN .. MSM_POINTS_C_MAX carries out of its top digit");

// clamp(ceil(log2 n) - 4, 7, 16): the fixed-base rule (choose_c), capped where the key space ends.
// KGS_MSM_POINTS_C overrides it for A/B timing.
int choose_points_c(uint64_t n) {
  return choose_window(n, MSM_POINTS_C_MIN, MSM_POINTS_C_MAX, "KGS_MSM_POINTS_C", MSM_POINTS_C_MAX);
}

void check_args(const void* points, const void* scalars, uint64_t n, int window_c, const uint8_t* out) {
  if (!out) throw KgsError(KGS_E_ARG, "kgs_msm_points: NULL output");
  if (window_c != 0 && (window_c < MSM_POINTS_C_MIN || window_c > MSM_POINTS_C_MAX))
    throw KgsError(KGS_E_ARG, "kgs_msm_points: window_c must be 0 or in " + std::to_string(MSM_POINTS_C_MIN) + " .. " +
                                  std::to_string(MSM_POINTS_C_MAX));
  if (n > MSM_POINTS_MAX) throw KgsError(KGS_E_ARG, "kgs_msm_points: at most 2^26 points");
  if (n && (!points || !scalars)) throw KgsError(KGS_E_ARG, "kgs_msm_points: NULL argument");
}

}  // namespace

// The bucket passes over a row in msm_points_run's form and the host finish (context.hpp): what
// kgs_msm_points runs after converting its bases, and kgs_commit_evals over the cached Lagrange row.
void kgsi::msm_points_over_row(kgs_ctx& c, const uint32_t* row29, const uint32_t* d_scalars_std, uint64_t n,
                               int window_c, uint8_t out[64]) {
  const int cc = window_c ? window_c : choose_points_c(n);
  const int W = (255 + cc - 1) / cc;
  if (n * (uint64_t)W > (1ull << 31))
    throw KgsError(KGS_E_ARG, "kgs_msm_points: window_c = " + std::to_string(cc) + " holds at most 2^31 / " +
                                  std::to_string(W) + " points");
  DrainOnError drain(&c);
  const MsmSizes z = msm_points_work_sizes(n, cc);
  MsmWork w;
  msm_work_from_pool(c, w, "mp_", "", z);
  uint32_t* dT = c.buf("mp_T", z.T);
  if (!msm_points_run(c.st, w, row29, d_scalars_std, n, cc, dT)) throw KgsError(KGS_E_ARG, "unsupported MSM window");
  check_launch();
  std::vector<uint8_t> T(z.T);
  HC(hipMemcpyAsync(T.data(), dT, z.T, hipMemcpyDeviceToHost, c.st));
  HC(hipStreamSynchronize(c.st));
  // sum_j 2^(c j) sum_k 2^k T[j][k] = sum_m 2^m T[m], m = j * c + k
  combine_partials(T.data(), z.T, 1, W * cc, out);
}

namespace {

// The MSM on the context's device; the caller holds the context's mutex and has set the device.
// points / scalars: host pointers (device = false) or device pointers. Ends with the main stream drained.
void msm_points_gpu(kgs_ctx& c, const void* points, const void* scalars, bool device, uint64_t n, int window_c,
                    uint8_t out[64]) {
  DrainOnError drain(&c);
  uint32_t* row = c.buf("mp_row", 64 * n);
  uint32_t* sc = device ? nullptr : c.buf("mp_scal", 32 * n);
  HC(hipMemcpyAsync(row, points, 64 * n, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.st));
  if (!device) HC(hipMemcpyAsync(sc, scalars, 32 * n, hipMemcpyHostToDevice, c.st));
  msm_points_row29(c.st, row, n);
  msm_points_over_row(c, row, device ? (const uint32_t*)scalars : sc, n, window_c, out);
}

int msm_points_entry(kgs_ctx_t* ctx, const void* points, const void* scalars, bool device, uint64_t n, int window_c,
                     uint8_t out[64]) {
  API_BEGIN
  check_args(points, scalars, n, window_c, out);
  if (!ctx) {
    if (device) throw KgsError(KGS_E_ARG, "kgs_msm_points_device: NULL ctx");
    host::g1_lincomb_segment((const uint8_t*)points, (const uint8_t*)scalars, n).to_affine_lem(out);
    return KGS_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, "kgs_msm_points");
  if (!n) {
    memset(out, 0, 64);
    return KGS_OK;
  }
  HC(hipSetDevice(ctx->device));
  msm_points_gpu(*ctx, points, scalars, device, n, window_c, out);
  API_END
}

}  // namespace

extern "C" {

int kgs_msm_points(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, uint64_t n, int window_c,
                   uint8_t out_lem[64]) {
  return msm_points_entry(ctx, points_lem, scalars_std, false, n, window_c, out_lem);
}

int kgs_msm_points_device(kgs_ctx_t* ctx, const void* d_points_lem, const void* d_scalars_std, uint64_t n,
                          int window_c, uint8_t out_lem[64]) {
  return msm_points_entry(ctx, d_points_lem, d_scalars_std, true, n, window_c, out_lem);
}

}  // extern "C"
