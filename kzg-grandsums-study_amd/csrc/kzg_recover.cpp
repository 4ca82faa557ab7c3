// kgs_kzg_recover_cosets (include/kgs.h; kernels in recover.hip): a polynomial of known length
// back from a subset of its cosets. Fr only: no SRS, no G1, no pairing. Host: argument checks, the call's own
// "rc_*" buffers in the context's pool, the launch sequence, and the reading of the four flag words at the end.
// Every kernel's accesses are bounded whatever the flags say, so one drain at the end is the only one.
// kgs_kzg_recover_cosets_many follows it: many polynomials side by side through the same stages,
// each launched once, with buffers of its own ("rcm_*").
#include <mutex>

#include "context.hpp"

namespace {

constexpr int RC_NBITS_MAX = 23;  // what the shared domain tables cover

struct RcBufs {
  uint32_t *row_of, *flags, *T, *W, *zc, *zs, *zev, *zsh, *inv, *A, *R;
};

RcBufs rc_bufs(kgs_ctx& c, int nbits, int lbits) {
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  RcBufs b;
  b.row_of = c.buf("rc_row_of", 4 * m);
  b.flags = c.buf("rc_flags", 64);
  b.T = c.buf("rc_T", 32 * m);
  b.W = c.buf("rc_W", 64 * m);
  b.zc = c.buf("rc_zc", 32 * m);
  b.zs = c.buf("rc_zs", 32 * m);
  b.zev = c.buf("rc_zev", 32 * m);
  b.zsh = c.buf("rc_zsh", 32 * m);
  b.inv = c.buf("rc_inv", 32 * m);
  b.A = c.buf("rc_A", 32 * n);
  b.R = c.buf("rc_R", 32 * n);
  return b;
}

int rc_leaf_log(int logm, int leaf_log) { return leaf_log < logm ? leaf_log : logm; }

// the marks and the product tree: T = Y^count z(Y), the vanishing polynomial of the missing cosets in Y = X^l
void rc_tree(kgs_ctx& c, const RcBufs& b, const uint64_t* d_index, uint64_t count, int logm, int leaf_log) {
  const uint64_t m = 1ull << logm;
  HC(hipMemsetAsync(b.row_of, 0xFF, 4 * m, c.st));
  HC(hipMemsetAsync(b.flags, 0xFF, 12, c.st));
  HC(hipMemsetAsync(b.flags + RC_FLAG_HIGH, 0, 4, c.st));
  launch_rc_mark(c.st, b.row_of, b.flags, d_index, count, m);
  const int ll = rc_leaf_log(logm, leaf_log);
  launch_rc_leaves(c.st, b.T, b.row_of, c.tw_fwd, logm, ll);
  for (int logd = ll; logd < logm; logd++) launch_rc_level(c.st, b.T, b.W, logm, logd, c.tw_fwd, c.tw_inv, c.invm);
}

// z(a_i) and 1 / z(g^l a_i), i < m, both at position bitrev(i): two transforms of size m and one batch inversion
void rc_mside(kgs_ctx& c, const RcBufs& b, uint64_t count, int logm, int lbits) {
  const uint64_t m = 1ull << logm;
  launch_rc_zcoef(c.st, b.zc, b.zs, b.T, count, m, c.coset_pow, lbits);
  ntt_dif(c.st, b.zev, b.zc, m, logm, nullptr, c.tw_fwd, c.logM);
  ntt_dif(c.st, b.zsh, b.zs, m, logm, nullptr, c.tw_fwd, c.logM);
  launch_rc_batch_inv(c.st, b.inv, b.zsh, m);
}

// the three transforms of size n with the division between the second and the third: A = E Z (natural) ->
// R = its coefficients -> R on g <w> (bit-reversed) / Z there -> q (natural) in R
void rc_nside(kgs_ctx& c, const RcBufs& b, int nbits, int lbits, bool divide = true) {
  intt_nat(c, b.R, b.A, nbits);
  coset_fwd(c, b.A, b.R, 1ull << nbits, nbits);
  if (divide) launch_rc_divide(c.st, b.A, b.inv, lbits, 1ull << nbits);
  ntt_dit(c.st, b.R, b.A, 1, nbits, c.tw_inv, c.logM, c.coset_ipow, c.invm + 8 * nbits);
}

// The whole call on device pointers, enqueued on the main stream (not synchronised). The caller holds the context,
// has checked the arguments and grown the domain to 2^nbits.
void rc_run(kgs_ctx& c, const RcBufs& b, int nbits, int lbits, const uint64_t* d_index, const uint32_t* d_ys, uint64_t count,
            uint64_t len, uint32_t* d_coef, uint32_t* d_evals, int leaf_log = RC_LEAF_LOG) {
  const int logm = nbits - lbits;
  const uint64_t n = 1ull << nbits;
  rc_tree(c, b, d_index, count, logm, leaf_log);
  rc_mside(c, b, count, logm, lbits);
  launch_rc_scatter(c.st, b.A, d_ys, b.row_of, b.zev, b.flags, logm, lbits);
  rc_nside(c, b, nbits, lbits);
  launch_rc_check_copy(c.st, d_coef, b.R, len, n, b.flags);
  if (d_evals) {
    ntt_dif(c.st, b.A, d_coef, len, nbits, nullptr, c.tw_fwd, c.logM);
    launch_bitrev_copy(c.st, d_evals, b.A, nbits);
  }
  check_launch();
}

void rc_check_args(kgs_ctx_t* ctx, const char* fn, int nbits, int lbits, const void* index, const void* ys, uint64_t count,
                   uint64_t len, const void* coef) {
  if (!ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx (recovery has no host path)");
  if (!index || !ys || !coef) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (nbits < 0 || nbits > RC_NBITS_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " + std::to_string(RC_NBITS_MAX));
  if (lbits < 0 || lbits > nbits)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": lbits must be in 0 .. nbits = " + std::to_string(nbits));
  const uint64_t n = 1ull << nbits, l = 1ull << lbits, m = n >> lbits;
  if (len < 1 || len > n)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": len = " + std::to_string(len) + " must be in 1 .. 2^nbits = " + std::to_string(n));
  const uint64_t need = (len + l - 1) >> lbits;
  if (count < need || count > m)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": count = " + std::to_string(count) + " must be in ceil(len / l) = " +
                                  std::to_string(need) + " .. m = " + std::to_string(m));
}

// the flag words after the drain: the refusals they stand for, else the verdict
int rc_verdict(kgs_ctx& c, const char* fn, const uint32_t* hf, const uint64_t* index, bool device, int nbits, int lbits) {
  const uint64_t m = 1ull << (nbits - lbits);
  auto index_at = [&](uint64_t k) {
    uint64_t v = 0;
    if (device)
      HC(hipMemcpy(&v, index + k, 8, hipMemcpyDeviceToHost));
    else
      v = index[k];
    return v;
  };
  if (hf[RC_FLAG_INDEX] != RC_NONE) {
    const uint64_t k = hf[RC_FLAG_INDEX];
    throw KgsError(KGS_E_ARG, std::string(fn) + ": index[" + std::to_string(k) + "] = " + std::to_string(index_at(k)) +
                                  " is not a coset of the domain (m = " + std::to_string(m) + ").");
  }
  if (hf[RC_FLAG_DUP] != RC_NONE) {
    const uint64_t k = hf[RC_FLAG_DUP];
    throw KgsError(KGS_E_ARG, std::string(fn) + ": index[" + std::to_string(k) + "] = " + std::to_string(index_at(k)) +
                                  " names a coset for the second time.");
  }
  if (hf[RC_FLAG_VALUE] != RC_NONE) {
    const uint64_t e = hf[RC_FLAG_VALUE];
    throw KgsError(KGS_E_ARG, std::string(fn) + ": value " + std::to_string(e & ((1ull << lbits) - 1)) + " of row " +
                                  std::to_string(e >> lbits) + " is not below r.");
  }
  (void)c;
  return hf[RC_FLAG_HIGH] ? 0 : 1;
}

int recover_entry(kgs_ctx_t* ctx, int nbits, int lbits, const void* index, const void* ys, uint64_t count, uint64_t len,
                  void* coef, void* evals, bool device) {
  API_BEGIN
  const char* fn = device ? "kgs_kzg_recover_cosets_device" : "kgs_kzg_recover_cosets";
  rc_check_args(ctx, fn, nbits, lbits, index, ys, count, len, coef);
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn);
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  const uint64_t n = 1ull << nbits, l = 1ull << lbits;
  if (nbits > c.logM) ensure_domain(c, nbits);
  const RcBufs b = rc_bufs(c, nbits, lbits);
  uint32_t* hf = (uint32_t*)c.pin(16);
  if (device) {
    rc_run(c, b, nbits, lbits, (const uint64_t*)index, (const uint32_t*)ys, count, len, (uint32_t*)coef, (uint32_t*)evals);
  } else {
    uint64_t* di = (uint64_t*)c.buf("rc_index", 8 * count);
    uint32_t* dy = c.buf("rc_ys", 32 * count * l);
    uint32_t* dc = c.buf("rc_coef", 32 * len);
    uint32_t* de = evals ? c.buf("rc_ev", 32 * n) : nullptr;
    HC(hipMemcpyAsync(di, index, 8 * count, hipMemcpyHostToDevice, c.st));
    HC(hipMemcpyAsync(dy, ys, 32 * count * l, hipMemcpyHostToDevice, c.st));
    rc_run(c, b, nbits, lbits, di, dy, count, len, dc, de);
    HC(hipMemcpyAsync(coef, dc, 32 * len, hipMemcpyDeviceToHost, c.st));
    if (evals) HC(hipMemcpyAsync(evals, de, 32 * n, hipMemcpyDeviceToHost, c.st));
  }
  HC(hipMemcpyAsync(hf, b.flags, 16, hipMemcpyDeviceToHost, c.st));
  c.sync();
  uint32_t flags[4];
  memcpy(flags, hf, 16);
  c.reset_staging();
  return rc_verdict(c, fn, flags, (const uint64_t*)index, device, nbits, lbits);
  API_END
}

// ------------------------------------------------------------------ many polynomials in one call
// P = polys rounded up to a power of two polynomials side by side, every stage one launch sequence for all of them:
// the trees of the P polynomials are the levels of one array of P m slots stopped at degree m, the transforms are
// block transforms (ntt_dif_blocks / ntt_dit_blocks). Buffers of the call's own ("rcm_*").
struct RcmBufs {
  int logP;
  uint32_t *row_of, *flags, *cnt, *high, *T, *W, *zc, *zs, *inv, *A;
  uint64_t flag_words;  // 4 flag words, P counts, P "nonzero from len on" words: one block, one transfer back
};

int rcm_log2_ceil(uint64_t x) {
  int lg = 0;
  while ((1ull << lg) < x) lg++;
  return lg;
}

RcmBufs rcm_bufs(kgs_ctx& c, int nbits, int lbits, uint64_t polys) {
  RcmBufs b;
  b.logP = rcm_log2_ceil(polys);
  const uint64_t P = 1ull << b.logP, pn = P << nbits, pm = pn >> lbits;
  b.flag_words = 4 + 2 * P;
  b.row_of = c.buf("rcm_row_of", 4 * pm);
  b.flags = c.buf("rcm_flags", 4 * b.flag_words);
  b.cnt = b.flags + 4;
  b.high = b.cnt + P;
  b.T = c.buf("rcm_T", 32 * pm);
  b.W = c.buf("rcm_W", 64 * pm);
  b.zc = c.buf("rcm_zc", 32 * pm);
  b.zs = c.buf("rcm_zs", 32 * pm);
  b.inv = c.buf("rcm_inv", 32 * pm);
  b.A = c.buf("rcm_A", 32 * pn);
  return b;
}

// the marks and the P trees: block b of T = Y^cnt[b] z_b(Y)
void rcm_tree(kgs_ctx& c, const RcmBufs& b, const uint32_t* d_poly_of, const uint64_t* d_index, uint64_t count, uint64_t polys,
              int logm) {
  const int logpm = b.logP + logm;
  HC(hipMemsetAsync(b.row_of, 0xFF, 4ull << logpm, c.st));
  HC(hipMemsetAsync(b.flags, 0xFF, 16, c.st));
  HC(hipMemsetAsync(b.cnt, 0, 4 * (b.flag_words - 4), c.st));
  launch_rcm_mark(c.st, b.row_of, b.flags, b.cnt, d_poly_of, d_index, count, polys, 1ull << logm);
  const int ll = rc_leaf_log(logm, RC_LEAF_LOG);
  launch_rcm_leaves(c.st, b.T, b.row_of, c.tw_fwd, logpm, logm, ll);
  for (int logd = ll; logd < logm; logd++) launch_rc_level(c.st, b.T, b.W, logpm, logd, c.tw_fwd, c.tw_inv, c.invm);
}

// z_b(a_i) in zc and 1 / z_b(g^l a_i) in inv, both at b m + bitrev(i)
void rcm_mside(kgs_ctx& c, const RcmBufs& b, int logm, int lbits) {
  const int logpm = b.logP + logm;
  launch_rcm_zcoef(c.st, b.zc, b.zs, b.T, b.cnt, logpm, logm, c.coset_pow, lbits);
  ntt_dif_blocks(c.st, b.zc, logpm, logm, c.tw_fwd);
  ntt_dif_blocks(c.st, b.zs, logpm, logm, c.tw_fwd);
  launch_rc_batch_inv(c.st, b.inv, b.zs, 1ull << logpm);
}

// A: E_b Z_b bit-reversed within each block -> coefficients -> on g <w> (bit-reversed) / Z_b there -> q_b(g X), natural
void rcm_nside(kgs_ctx& c, const RcmBufs& b, int nbits, int lbits, bool divide = true) {
  const int logpn = b.logP + nbits;
  ntt_dit_blocks(c.st, b.A, logpn, nbits, c.tw_inv, c.invm + 8 * nbits);
  launch_rcm_twist(c.st, b.A, c.coset_pow, logpn, nbits);
  ntt_dif_blocks(c.st, b.A, logpn, nbits, c.tw_fwd);
  if (divide) launch_rc_divide(c.st, b.A, b.inv, lbits, 1ull << logpn);
  ntt_dit_blocks(c.st, b.A, logpn, nbits, c.tw_inv, c.invm + 8 * nbits);
}

// The whole call on device pointers, enqueued on the main stream (not synchronised); as rc_run
void rcm_run(kgs_ctx& c, const RcmBufs& b, int nbits, int lbits, uint64_t polys, const uint32_t* d_poly_of,
             const uint64_t* d_index, const uint32_t* d_ys, uint64_t count, uint64_t len, uint64_t stride, uint32_t* d_coef,
             uint32_t* d_evals) {
  const int logm = nbits - lbits;
  rcm_tree(c, b, d_poly_of, d_index, count, polys, logm);
  rcm_mside(c, b, logm, lbits);
  launch_rcm_scatter(c.st, b.A, d_ys, b.row_of, b.zc, b.flags, b.logP + nbits, logm, lbits);
  rcm_nside(c, b, nbits, lbits);
  launch_rcm_check_copy(c.st, d_coef, b.A, c.coset_ipow, len, stride, nbits, polys, b.high);
  if (d_evals && !nbits) {  // n = 1: the value is the coefficient
    HC(hipMemcpy2DAsync(d_evals, 32, d_coef, 32 * stride, 32, polys, hipMemcpyDeviceToDevice, c.st));
  } else if (d_evals) {  // kgs_kzg_open_cosets_many's route
    launch_coset_rows_many(c.st, b.A, d_coef, polys, stride, len, nbits, 0, nbits, 1ull << b.logP);
    ntt_dif_blocks(c.st, b.A, b.logP + nbits, nbits, c.tw_fwd);
    launch_bitrev_blocks(c.st, d_evals, b.A, nbits, polys);
  }
  check_launch();
}

void rcm_check_args(const std::string& fn, int nbits, int lbits, uint64_t polys, const void* poly_of,
                    const void* index, const void* ys, uint64_t count, uint64_t len, uint64_t stride, const void* coef) {
  if (nbits < 0 || nbits > RC_NBITS_MAX) throw KgsError(KGS_E_ARG, fn + ": nbits must be in 0 .. " + std::to_string(RC_NBITS_MAX));
  if (lbits < 0 || lbits > nbits) throw KgsError(KGS_E_ARG, fn + ": lbits must be in 0 .. nbits = " + std::to_string(nbits));
  const uint64_t n = 1ull << nbits, m = n >> lbits;
  if (len < 1 || len > n)
    throw KgsError(KGS_E_ARG, fn + ": len = " + std::to_string(len) + " must be in 1 .. 2^nbits = " + std::to_string(n));
  if (polys > (1ull << 24) >> nbits)
    throw KgsError(KGS_E_ARG, fn + ": polys = " + std::to_string(polys) + " times 2^nbits must be at most 2^24");
  if (count > polys * m)
    throw KgsError(KGS_E_ARG, fn + ": count = " + std::to_string(count) + " must be at most polys m = " + std::to_string(polys * m));
  if (stride < len)
    throw KgsError(KGS_E_ARG, fn + ": stride = " + std::to_string(stride) + " must be at least len = " + std::to_string(len));
  if (!coef) throw KgsError(KGS_E_ARG, fn + ": NULL coefficient buffer");
  if (count && (!poly_of || !index || !ys)) throw KgsError(KGS_E_ARG, fn + ": NULL cell array");
}

// the refusals the three flag words stand for
void rcm_refusals(const std::string& fn, const uint32_t* hf, const uint32_t* poly_of, const uint64_t* index, bool device,
                  uint64_t polys, int nbits, int lbits) {
  const uint64_t m = 1ull << (nbits - lbits);
  auto cell = [&](uint64_t k, uint64_t& b, uint64_t& i) {
    uint32_t bb = 0;
    if (device) {
      HC(hipMemcpy(&bb, poly_of + k, 4, hipMemcpyDeviceToHost));
      HC(hipMemcpy(&i, index + k, 8, hipMemcpyDeviceToHost));
    } else {
      bb = poly_of[k], i = index[k];
    }
    b = bb;
  };
  uint64_t b = 0, i = 0;
  if (hf[RC_FLAG_INDEX] != RC_NONE) {
    const uint64_t k = hf[RC_FLAG_INDEX];
    cell(k, b, i);
    if (b >= polys)
      throw KgsError(KGS_E_ARG, fn + ": poly_of[" + std::to_string(k) + "] = " + std::to_string(b) + " is not below polys = " +
                                    std::to_string(polys) + ".");
    throw KgsError(KGS_E_ARG, fn + ": index[" + std::to_string(k) + "] = " + std::to_string(i) +
                                  " is not a coset of the domain (m = " + std::to_string(m) + ").");
  }
  if (hf[RC_FLAG_DUP] != RC_NONE) {
    const uint64_t k = hf[RC_FLAG_DUP];
    cell(k, b, i);
    throw KgsError(KGS_E_ARG, fn + ": index[" + std::to_string(k) + "] = " + std::to_string(i) + " names a coset of polynomial " +
                                  std::to_string(b) + " for the second time.");
  }
  if (hf[RC_FLAG_VALUE] != RC_NONE) {
    const uint64_t e = hf[RC_FLAG_VALUE];
    throw KgsError(KGS_E_ARG, fn + ": value " + std::to_string(e & ((1ull << lbits) - 1)) + " of row " +
                                  std::to_string(e >> lbits) + " is not below r.");
  }
}

int recover_many_entry(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const void* poly_of, const void* index,
                       const void* ys, uint64_t count, uint64_t len, uint64_t stride, void* coef, void* evals,
                       uint8_t* status_out, bool device) {
  API_BEGIN
  const std::string fn = device ? "kgs_kzg_recover_cosets_many_device" : "kgs_kzg_recover_cosets_many";
  if (!ctx) throw KgsError(KGS_E_ARG, fn + ": NULL ctx (recovery has no host path)");
  if (!polys) return 1;
  rcm_check_args(fn, nbits, lbits, polys, poly_of, index, ys, count, len, stride, coef);
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn.c_str());
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  const uint64_t n = 1ull << nbits, l = 1ull << lbits;
  if (nbits > c.logM) ensure_domain(c, nbits);
  const RcmBufs b = rcm_bufs(c, nbits, lbits, polys);
  c.ensure_pin(4 * b.flag_words + 64);
  uint32_t* hf = (uint32_t*)c.pin(4 * b.flag_words);
  if (device) {
    rcm_run(c, b, nbits, lbits, polys, (const uint32_t*)poly_of, (const uint64_t*)index, (const uint32_t*)ys, count, len, stride,
            (uint32_t*)coef, (uint32_t*)evals);
  } else {
    uint32_t* dp = c.buf("rcm_poly_of", 4 * count);
    uint64_t* di = (uint64_t*)c.buf("rcm_index", 8 * count);
    uint32_t* dy = c.buf("rcm_ys", 32 * count * l);
    uint32_t* dc = c.buf("rcm_coef", 32 * len * polys);  // packed: the gaps of a stride above len stay on the host
    uint32_t* de = evals ? c.buf("rcm_ev", 32 * n * polys) : nullptr;
    if (count) {
      HC(hipMemcpyAsync(dp, poly_of, 4 * count, hipMemcpyHostToDevice, c.st));
      HC(hipMemcpyAsync(di, index, 8 * count, hipMemcpyHostToDevice, c.st));
      HC(hipMemcpyAsync(dy, ys, 32 * count * l, hipMemcpyHostToDevice, c.st));
    }
    rcm_run(c, b, nbits, lbits, polys, dp, di, dy, count, len, len, dc, de);
    if (stride == len)
      HC(hipMemcpyAsync(coef, dc, 32 * len * polys, hipMemcpyDeviceToHost, c.st));
    else
      HC(hipMemcpy2DAsync(coef, 32 * stride, dc, 32 * len, 32 * len, polys, hipMemcpyDeviceToHost, c.st));
    if (evals) HC(hipMemcpyAsync(evals, de, 32 * n * polys, hipMemcpyDeviceToHost, c.st));
  }
  HC(hipMemcpyAsync(hf, b.flags, 4 * b.flag_words, hipMemcpyDeviceToHost, c.st));
  c.sync();
  const std::vector<uint32_t> flags(hf, hf + b.flag_words);
  c.reset_staging();
  rcm_refusals(fn, flags.data(), (const uint32_t*)poly_of, (const uint64_t*)index, device, polys, nbits, lbits);
  // a polynomial's status: from its count first, the arithmetic only where the count allows a verdict
  const uint64_t need = (len + l - 1) >> lbits;
  const uint32_t *cnt = flags.data() + 4, *high = cnt + (1ull << b.logP);
  int all = 1;
  for (uint64_t p = 0; p < polys; p++) {
    const uint8_t s = cnt[p] < need ? 2 : high[p] ? 0 : 1;
    if (status_out) status_out[p] = s;
    if (s != 1) all = 0;
  }
  return all;
  API_END
}

}  // namespace

extern "C" {

int kgs_kzg_recover_cosets_many(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const uint32_t* poly_of,
                                const uint64_t* index, const uint8_t* ys_mont, uint64_t count, uint64_t len, uint64_t stride,
                                uint8_t* coef_mont, uint8_t* evals_mont, uint8_t* status_out) {
  return recover_many_entry(ctx, nbits, lbits, polys, poly_of, index, ys_mont, count, len, stride, coef_mont, evals_mont,
                            status_out, false);
}

int kgs_kzg_recover_cosets_many_device(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const void* d_poly_of,
                                       const void* d_index, const void* d_ys_mont, uint64_t count, uint64_t len,
                                       uint64_t stride, void* d_coef_mont, void* d_evals_mont, uint8_t* status_out) {
  return recover_many_entry(ctx, nbits, lbits, polys, d_poly_of, d_index, d_ys_mont, count, len, stride, d_coef_mont,
                            d_evals_mont, status_out, true);
}

// ---- timing helper of profiles/kzg_recover_cosets_many_time.py
int kgs_bench_kzg_recover_cosets_many(kgs_ctx_t* ctx, int nbits, int lbits, uint64_t polys, const void* d_poly_of,
                                      const void* d_index, const void* d_ys_mont, uint64_t count, uint64_t len,
                                      uint64_t stride, void* d_coef_mont, int what, int reps, double* ms) {
  API_BEGIN
  const std::string fn = "kgs_bench_kzg_recover_cosets_many";
  if (!ctx) throw KgsError(KGS_E_ARG, fn + ": NULL ctx (recovery has no host path)");
  if (!polys) throw KgsError(KGS_E_ARG, fn + ": polys must be at least 1");
  rcm_check_args(fn, nbits, lbits, polys, d_poly_of, d_index, d_ys_mont, count, len, stride, d_coef_mont);
  if (!ms || what < 0 || what > 4 || reps < 1) throw KgsError(KGS_E_ARG, fn + ": bad what / reps / ms");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn.c_str());
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  if (nbits > c.logM) ensure_domain(c, nbits);
  const int logm = nbits - lbits;
  const uint64_t l = 1ull << lbits, m = 1ull << logm;
  const uint32_t* dp = (const uint32_t*)d_poly_of;
  const uint64_t* di = (const uint64_t*)d_index;
  const uint32_t* dy = (const uint32_t*)d_ys_mont;
  uint32_t* dc = (uint32_t*)d_coef_mont;
  // the yardstick takes each polynomial's cells as one run of the arrays: first[p] .. first[p + 1]
  std::vector<uint64_t> first;
  RcBufs sb{};
  if (what == 4) {
    std::vector<uint32_t> po(count);
    if (count) HC(hipMemcpy(po.data(), dp, 4 * count, hipMemcpyDeviceToHost));
    first.assign(polys + 1, count);
    uint64_t p = 0;
    first[0] = 0;
    for (uint64_t k = 0; k < count; k++) {
      if (po[k] >= polys || po[k] < p) throw KgsError(KGS_E_ARG, fn + ": what = 4 takes the cells grouped by ascending polynomial");
      while (p < po[k]) first[++p] = k;
    }
    const uint64_t need = (len + l - 1) >> lbits;
    for (p = 0; p < polys; p++)
      if (first[p + 1] - first[p] < need || first[p + 1] - first[p] > m)
        throw KgsError(KGS_E_ARG, fn + ": what = 4 needs ceil(len / l) .. m cells for every polynomial");
    sb = rc_bufs(c, nbits, lbits);
  }
  const RcmBufs b = rcm_bufs(c, nbits, lbits, polys);
  // every leg after one whole call: the buffers grown and holding this input's intermediate values
  rcm_run(c, b, nbits, lbits, polys, dp, di, dy, count, len, stride, dc, nullptr);
  HC(hipStreamSynchronize(c.st));
  EventTimer timer;
  for (int r = 0; r < reps; r++)
    ms[r] = timer.ms(c.st, [&] {
      if (what == 0)
        rcm_run(c, b, nbits, lbits, polys, dp, di, dy, count, len, stride, dc, nullptr);
      else if (what == 1)
        rcm_tree(c, b, dp, di, count, polys, logm);
      else if (what == 2)
        rcm_mside(c, b, logm, lbits);
      else if (what == 3)
        rcm_nside(c, b, nbits, lbits, false);
      else
        for (uint64_t p = 0; p < polys; p++)
          rc_run(c, sb, nbits, lbits, di + first[p], dy + 8 * (first[p] << lbits), first[p + 1] - first[p], len,
                 dc + 8 * stride * p, nullptr);
    });
  c.reset_staging();
  API_END
}

int kgs_kzg_recover_cosets(kgs_ctx_t* ctx, int nbits, int lbits, const uint64_t* index, const uint8_t* ys_mont,
                           uint64_t count, uint64_t len, uint8_t* coef_mont, uint8_t* evals_mont) {
  return recover_entry(ctx, nbits, lbits, index, ys_mont, count, len, coef_mont, evals_mont, false);
}

int kgs_kzg_recover_cosets_device(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                  uint64_t count, uint64_t len, void* d_coef_mont, void* d_evals_mont) {
  return recover_entry(ctx, nbits, lbits, d_index, d_ys_mont, count, len, d_coef_mont, d_evals_mont, true);
}

// ---- timing helper of profiles/kzg_recover_cosets_time.py
int kgs_bench_kzg_recover_cosets(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                 uint64_t count, uint64_t len, void* d_coef_mont, int what, int leaf_log, int reps,
                                 double* ms) {
  API_BEGIN
  const char* fn = "kgs_bench_kzg_recover_cosets";
  rc_check_args(ctx, fn, nbits, lbits, d_index, d_ys_mont, count, len, d_coef_mont);
  if (!ms || what < 0 || what > 3 || reps < 1) throw KgsError(KGS_E_ARG, std::string(fn) + ": bad what / reps / ms");
  if (!leaf_log) leaf_log = RC_LEAF_LOG;
  if (leaf_log < RC_LEAF_LOG_MIN || leaf_log > RC_LEAF_LOG_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": leaf_log must be 0 or in " + std::to_string(RC_LEAF_LOG_MIN) + " .. " +
                                  std::to_string(RC_LEAF_LOG_MAX));
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn);
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(&c);
  c.reset_staging();
  if (nbits > c.logM) ensure_domain(c, nbits);
  const RcBufs b = rc_bufs(c, nbits, lbits);
  const int logm = nbits - lbits;
  // every leg after one whole call: the buffers grown and holding this input's intermediate values
  rc_run(c, b, nbits, lbits, (const uint64_t*)d_index, (const uint32_t*)d_ys_mont, count, len, (uint32_t*)d_coef_mont, nullptr,
         leaf_log);
  HC(hipStreamSynchronize(c.st));
  EventTimer timer;
  for (int r = 0; r < reps; r++)
    ms[r] = timer.ms(c.st, [&] {
      if (what == 0)
        rc_run(c, b, nbits, lbits, (const uint64_t*)d_index, (const uint32_t*)d_ys_mont, count, len, (uint32_t*)d_coef_mont,
               nullptr, leaf_log);
      else if (what == 1)
        rc_tree(c, b, (const uint64_t*)d_index, count, logm, leaf_log);
      else if (what == 2)
        rc_mside(c, b, count, logm, lbits);
      else
        rc_nside(c, b, nbits, lbits, false);
    });
  c.reset_staging();
  API_END
}

}  // extern "C"
