// Batch verifier for coset openings: kgs_kzg_verify_cosets_batch, kgs_kzg_verify_cosets_batch_device,
// kgs_coset_interp_fold, kgs_coset_interp_fold_device (include/kgs.h; kernels in coset_fold.hip).
//
// count openings (commitment c(k), coset i_k, values y_k, proof pi_k) against one SRS collapse, under the weights
// w_k = rho^k, into ONE check e(-A, [tau^l]_2) e(B, [1]_2) == 1 with
//   A = sum_k w_k pi_k,   B = sum_k w_k C_c(k) + sum_k (w_k a_{i_k}) pi_k - [D(tau)]_1,   D = sum_k w_k I_k.
// Host: the seed and rho, the pairing checks, the bisection that names the invalid openings, and with
// ctx == NULL or below the routing threshold everything else too (host::Fr, g1_lincomb_segment). GPU: the
// structural checks, the weights, D (k_coset_interp_fold), the terms of A and B (k_coset_terms) and their sums
// (two msm_points_run), on the context's main stream in
// device buffers of the call's own ("cb_*" and msm_points' "mp_*" in the context's pool, grown on demand).
#include <chrono>
#include <mutex>

#include "context.hpp"
#include "host_pairing.hpp"
#include "keccak.hpp"
#include "verify_linear.hpp"

using host::G1;

namespace {

constexpr uint64_t CB_MAX_VALUES = 1ull << 26;  // count * l with a context
constexpr int CB_NBITS_CTX = 23, CB_NBITS_HOST = 28;

// A batch of fewer terms (3 count + l) folds on the host even with a context. Measured on MI355X
// (profiles/kzg_verify_cosets_batch_time.json): the host fold costs 0.031 ms per term (0.13 ms at 4
// terms, 0.34 at 11, 1.6 at 49, 3.3 at 104), the GPU fold 0.39 - 0.76 ms for every batch up to 112 terms (0.39 at
// 4, 0.44 at 11, 0.73 at 49): they cross between 11 and 49 terms, at about 0.75 ms.
constexpr uint64_t CB_GPU_MIN_TERMS = 24;
// A and B are two msm_points_run at every size. kgs_g1_lincomb's fold (launch_g1_fold, two segments) was the
// candidate for small batches; forced onto the same batches it took 3.3 - 5.2 ms up to 112 terms, 10 ms at 832 and
// 39 ms at 4096, against 0.39 - 0.76, 1.1 and 2.0 ms for the buckets (same JSON): there is no size at which it
// wins, so nothing is routed to it. KGS_VERIFY_COSETS_MSM = "fold" | "points" forces one for that A/B.
constexpr bool CB_SUMS_BY_FOLD = false;

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Keccak-256 (keccak.hpp's permutation and padding) over a message given in pieces
struct Keccak {
  uint64_t s[25];
  uint8_t block[136];
  size_t fill = 0;
  Keccak() { memset(s, 0, sizeof(s)); }
  void absorb_block() {
    for (size_t i = 0; i < 17; i++) {
      uint64_t w;
      memcpy(&w, block + 8 * i, 8);
      s[i] ^= w;
    }
    host::keccak_f1600(s);
    fill = 0;
  }
  void update(const void* data, size_t len) {
    const uint8_t* p = (const uint8_t*)data;
    while (len) {
      const size_t take = std::min(len, sizeof(block) - fill);
      memcpy(block + fill, p, take);
      fill += take;
      p += take;
      len -= take;
      if (fill == sizeof(block)) absorb_block();
    }
  }
  void le32(uint32_t x) { update(&x, 4); }  // little-endian host
  void le64(uint64_t x) { update(&x, 8); }
  void finish(uint8_t out[32]) {
    memset(block + fill, 0, sizeof(block) - fill);
    block[fill] |= 0x01;
    block[sizeof(block) - 1] |= 0x80;
    absorb_block();
    memcpy(out, s, 32);
  }
};

struct Batch {
  int nbits, lbits;
  const uint8_t* commits;
  uint64_t ncommits;
  const uint32_t* commit_of;
  const uint64_t* index;
  const uint8_t* ys;
  const uint8_t* proofs;
  uint64_t count;
  const uint8_t* srs;
  uint64_t l() const { return 1ull << lbits; }
  uint64_t m() const { return 1ull << (nbits - lbits); }
};

// rho = keccak256("kgs-verify-cosets-batch-v1/rho" || seed) as a little-endian integer mod r, 0 -> 1
Fr rho_from_seed(const uint8_t seed[32], uint8_t rho_std[32]) {
  static const char tag[] = "kgs-verify-cosets-batch-v1/rho";
  Keccak k;
  k.update(tag, sizeof(tag) - 1);
  k.update(seed, 32);
  uint8_t h[32];
  k.finish(h);
  uint64_t s[4];
  memcpy(s, h, 32);
  while (Fr::geq_p(s)) Fr::sub_p(s);  // h < 2^256 < 6 r
  if (!(s[0] | s[1] | s[2] | s[3])) s[0] = 1;
  memcpy(rho_std, s, 32);
  return Fr::from_std(s);
}

void derive_seed(const Batch& b, const uint8_t* tau_l_g2, uint8_t seed[32]) {
  static const char tag[] = "kgs-verify-cosets-batch-v1";
  Keccak k;
  k.update(tag, sizeof(tag) - 1);
  k.update(tau_l_g2, 128);
  k.le32((uint32_t)b.nbits);
  k.le32((uint32_t)b.lbits);
  k.le64(b.ncommits);
  k.update(b.commits, 64 * b.ncommits);
  k.le64(b.count);
  k.update(b.commit_of, 4 * b.count);
  k.update(b.index, 8 * b.count);
  k.update(b.ys, 32 * b.count * b.l());
  k.update(b.proofs, 64 * b.count);
  k.finish(seed);
}

// out[j] = sum_{lo <= k < hi, w_k != 0} w_k w^(-i_k j) J_{k,j}: kgs_kzg_verify_coset's interpolant, weighted and
// summed. skip: NULL, or one byte per row, 0 = leave the row out.
std::vector<Fr> interp_fold_host(int nbits, int lbits, const uint64_t* index, const uint8_t* ys, const Fr* w,
                                 const uint8_t* keep, uint64_t lo, uint64_t hi) {
  const size_t l = (size_t)1 << lbits;
  std::vector<Fr> D(l, Fr::zero()), J(l), tw(l > 1 ? l / 2 : 1);
  // tw[t] = Fr.w[lbits]^(-t), t < l / 2: stage h reads tw[t * (l / 2h)]
  const Fr pinv = host::fr_w_cached(lbits).inverse();
  tw[0] = Fr::one();
  for (size_t t = 1; t < l / 2; t++) tw[t] = tw[t - 1] * pinv;
  const Fr winv = host::fr_w_cached(nbits).inverse(), linv = Fr::from_u64(l).inverse();
  for (uint64_t k = lo; k < hi; k++) {
    if ((keep && !keep[k]) || w[k].is_zero()) continue;
    for (size_t j = 0; j < l; j++) {
      size_t b = 0;
      for (int s = 0; s < lbits; s++) b |= ((j >> s) & 1) << (lbits - 1 - s);
      J[b] = Fr::from_bytes(ys + 32 * (k * l + j));
    }
    for (size_t h = 1; h < l; h *= 2) {
      const size_t stride = l / (2 * h);
      for (size_t g = 0; g < l; g += 2 * h)
        for (size_t t = 0; t < h; t++) {
          const Fr a = J[g + t], bb = t ? J[g + t + h] * tw[t * stride] : J[g + t + h];
          J[g + t] = a + bb;
          J[g + t + h] = a - bb;
        }
    }
    const Fr step = winv.pow_u64(index[k]);
    Fr f = w[k] * linv;
    for (size_t j = 0; j < l; j++) {
      D[j] = D[j] + J[j] * f;
      f = f * step;
    }
  }
  return D;
}

void to_std_bytes(const Fr& x, uint8_t* out) {
  uint64_t s[4];
  x.to_std(s);
  memcpy(out, s, 32);
}

// -1: no override, 0 / 1: the first / the second of the two values
int env_choice(const char* name, const char* first, const char* second) {
  const char* e = getenv(name);
  if (!e) return -1;
  if (!strcmp(e, first)) return 0;
  if (!strcmp(e, second)) return 1;
  return -1;
}

// One way of folding a range of openings into (A, B); valid[] holds the structural verdicts once prepare() is done
struct Folder {
  virtual ~Folder() {}
  // the structural checks and the weights; fills valid (count bytes) as far as it is known before the first fold
  virtual void prepare(const Fr& rho, std::vector<uint8_t>& valid) = 0;
  // A || B (affine LEM) of the openings lo <= k < hi; the first call covers the whole batch and completes valid;
  // D_out: NULL or l x 32 B that receive D
  virtual void fold(uint64_t lo, uint64_t hi, uint8_t AB[128], uint8_t* D_out, std::vector<uint8_t>& valid) = 0;
};

struct HostFolder : Folder {
  const Batch& b;
  std::vector<Fr> w;
  explicit HostFolder(const Batch& bb) : b(bb) {}
  void prepare(const Fr& rho, std::vector<uint8_t>& valid) override {
    const uint64_t l = b.l();
    std::vector<uint8_t> cok(b.ncommits);
    for (uint64_t c = 0; c < b.ncommits; c++) cok[c] = host::g1_valid(b.commits + 64 * c);
    w.assign(b.count, Fr::zero());
    Fr p = Fr::one();
    for (uint64_t k = 0; k < b.count; k++, p = p * rho) {
      bool ok = b.commit_of[k] < b.ncommits && cok[b.commit_of[k]] && b.index[k] < b.m() &&
                host::g1_valid(b.proofs + 64 * k);
      for (uint64_t j = 0; ok && j < l; j++) ok = host::lt_mod(b.ys + 32 * (k * l + j), host::FR_MOD.p);
      valid[k] = ok;
      if (ok) w[k] = p;
    }
  }
  void fold(uint64_t lo, uint64_t hi, uint8_t AB[128], uint8_t* D_out, std::vector<uint8_t>& valid) override {
    const uint64_t l = b.l(), cnt = hi - lo;
    const std::vector<Fr> D = interp_fold_host(b.nbits, b.lbits, b.index, b.ys, w.data(), valid.data(), lo, hi);
    if (D_out)
      for (uint64_t j = 0; j < l; j++) D[j].to_bytes(D_out + 32 * j);
    std::vector<uint8_t> pts(64 * (3 * cnt + l), 0), sc(32 * (3 * cnt + l), 0);
    const Fr wm = host::fr_w_cached(b.nbits - b.lbits);
    for (uint64_t t = 0; t < cnt; t++) {
      const uint64_t k = lo + t;
      if (!valid[k]) continue;
      memcpy(&pts[64 * t], b.proofs + 64 * k, 64);
      memcpy(&pts[64 * (cnt + t)], b.commits + 64 * (uint64_t)b.commit_of[k], 64);
      memcpy(&pts[64 * (2 * cnt + t)], b.proofs + 64 * k, 64);
      to_std_bytes(w[k], &sc[32 * t]);
      memcpy(&sc[32 * (cnt + t)], &sc[32 * t], 32);
      to_std_bytes(w[k] * wm.pow_u64(b.index[k]), &sc[32 * (2 * cnt + t)]);
    }
    for (uint64_t j = 0; j < l; j++) {
      memcpy(&pts[64 * (3 * cnt + j)], b.srs + 64 * j, 64);
      to_std_bytes(D[j].neg(), &sc[32 * (3 * cnt + j)]);
    }
    host::g1_lincomb_segment(pts.data(), sc.data(), cnt).to_affine_lem(AB);
    host::g1_lincomb_segment(pts.data() + 64 * cnt, sc.data() + 32 * cnt, 2 * cnt + l).to_affine_lem(AB + 64);
  }
};

// The domain tables grown to 2^nbits (the call may do that, kgs.h); the staging areas it builds through are
// reset before and after, as every primitive does.
void need_domain(kgs_ctx& c, int nbits) {
  if (nbits <= c.logM) return;
  c.reset_staging();
  ensure_domain(c, nbits);
  c.reset_staging();
}

// D on the device: out, part as launch_coset_interp_fold takes them
void interp_fold_gpu(kgs_ctx& c, uint32_t* d_out, uint8_t* d_valid, uint32_t* d_bad, const uint32_t* d_ys,
                     const uint64_t* d_index, const uint32_t* d_w, uint64_t rows, int nbits, int lbits) {
  uint32_t* part = c.buf("cb_part", coset_fold_part_bytes(rows, lbits));
  if (!launch_coset_interp_fold(c.st, d_out, part, d_valid, d_bad, d_ys, d_index, d_w, rows, c.tw_inv, c.invm, nbits,
                                lbits))
    throw KgsError(KGS_E_ARG, "the interpolation fold on the GPU covers lbits 0 .. " +
                                  std::to_string(COSET_FOLD_LBITS_MAX));
  check_launch();
}

struct GpuFolder : Folder {
  kgs_ctx& c;
  const Batch& b;  // commit_of, index, ys, proofs: device pointers if `device`
  bool device;
  const uint32_t *d_commit_of = nullptr, *d_ys = nullptr, *d_proofs = nullptr;
  const uint64_t* d_index = nullptr;
  uint32_t *d_commits = nullptr, *d_srs = nullptr, *d_w = nullptr, *d_D = nullptr, *d_small = nullptr;
  uint8_t* d_valid = nullptr;
  uint32_t rho_words[8];
  bool first = true;
  GpuFolder(kgs_ctx& cc, const Batch& bb, bool dev) : c(cc), b(bb), device(dev) {}

  const uint32_t* input(const char* name, const void* p, size_t bytes) {
    if (device) return (const uint32_t*)p;
    uint32_t* d = c.buf(name, bytes);
    HC(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, c.st));
    return d;
  }
  void prepare(const Fr& rho, std::vector<uint8_t>&) override {
    const uint64_t l = b.l();
    need_domain(c, b.nbits);
    d_commit_of = input("cb_cof", b.commit_of, 4 * b.count);
    d_index = (const uint64_t*)input("cb_idx", b.index, 8 * b.count);
    d_ys = input("cb_ys", b.ys, 32 * b.count * l);
    d_proofs = input("cb_proofs", b.proofs, 64 * b.count);
    d_commits = c.buf("cb_commits", 64 * b.ncommits);
    if (b.ncommits) HC(hipMemcpyAsync(d_commits, b.commits, 64 * b.ncommits, hipMemcpyHostToDevice, c.st));
    d_srs = c.buf("cb_srs", 64 * l);
    HC(hipMemcpyAsync(d_srs, b.srs, 64 * l, hipMemcpyHostToDevice, c.st));
    d_w = c.buf("cb_w", 32 * b.count);
    d_D = c.buf("cb_D", 32 * l);
    d_small = c.buf("cb_small", 256);  // words 0 .. 7: rho; word 8: the fold's flag; 16 ..: the fold's offsets
    d_valid = (uint8_t*)c.buf("cb_valid", b.count);
    uint8_t* ok = (uint8_t*)c.buf("cb_ok", b.count + b.ncommits);
    memcpy(rho_words, rho.v, 32);
    HC(hipMemsetAsync(d_small, 0, 256, c.st));
    HC(hipMemcpyAsync(d_small, rho_words, 32, hipMemcpyHostToDevice, c.st));
    launch_g1_on_curve(c.st, ok, d_proofs, b.count);
    launch_g1_on_curve(c.st, ok + b.count, d_commits, b.ncommits);
    launch_coset_screen(c.st, d_valid, ok, ok + b.count, d_commit_of, d_index, b.count, b.ncommits, b.m());
    launch_powers(c.st, d_w, b.count, d_small, nullptr);
    check_launch();
  }
  void fold(uint64_t lo, uint64_t hi, uint8_t AB[128], uint8_t* D_out, std::vector<uint8_t>& valid) override {
    const uint64_t l = b.l(), cnt = hi - lo, nterms = 3 * cnt + l;
    // the range check of the values runs inside the fold and clears d_valid: the first fold covers every row
    interp_fold_gpu(c, d_D, d_valid + lo, d_small + 8, d_ys + 8 * lo * l, d_index + lo, d_w + 8 * lo, cnt, b.nbits,
                    b.lbits);
    uint32_t* scal = c.buf("cb_scal", 32 * nterms);
    uint32_t* pts = c.buf("cb_pts", 64 * nterms);
    launch_coset_terms(c.st, scal, pts, d_valid, d_w, d_index, d_commit_of, d_commits, d_proofs, d_D, d_srs, c.tw_fwd,
                       lo, cnt, b.nbits, b.lbits);
    check_launch();
    if (D_out) HC(hipMemcpyAsync(D_out, d_D, 32 * l, hipMemcpyDeviceToHost, c.st));
    if (first) HC(hipMemcpyAsync(valid.data(), d_valid, b.count, hipMemcpyDeviceToHost, c.st));
    first = false;
    const int force = env_choice("KGS_VERIFY_COSETS_MSM", "fold", "points");
    if (force == 1 || (force != 0 && !CB_SUMS_BY_FOLD)) {
      msm_points_row29(c.st, pts, nterms);
      msm_points_over_row(c, pts, scal, cnt, 0, AB);
      msm_points_over_row(c, pts + 16 * cnt, scal + 8 * cnt, 2 * cnt + l, 0, AB + 64);
    } else {
      const uint32_t off[3] = {0, (uint32_t)cnt, (uint32_t)nterms};
      uint32_t* d_off = d_small + 16;
      HC(hipMemcpyAsync(d_off, off, sizeof(off), hipMemcpyHostToDevice, c.st));
      uint32_t* out = c.buf("cb_out", 128);
      launch_g1_fold(c.st, out, pts, scal, d_off, nterms, 2, c.buf("cb_term", 128 * nterms), c.buf("cb_seg", 256),
                     c.buf("cb_scr", 64));
      check_launch();
      HC(hipMemcpyAsync(AB, out, 128, hipMemcpyDeviceToHost, c.st));
      HC(hipStreamSynchronize(c.st));
    }
  }
};

struct Bisect {
  Folder& f;
  std::vector<uint8_t>& valid;
  const host::G2A& tau_l;
  host::G2A g2 = host::g2_gen();
  kgs_coset_batch_diag_t* diag;
  uint32_t checks = 0;
  double fold_ms = 0, pairing_ms = 0;

  bool check(uint64_t lo, uint64_t hi) {
    uint8_t AB[128];
    const bool whole = checks == 0;
    double t0 = now_ms();
    f.fold(lo, hi, AB, whole && diag ? diag->interp_out : nullptr, valid);
    fold_ms += now_ms() - t0;
    if (whole && diag && diag->folded_out) memcpy(diag->folded_out, AB, 128);
    t0 = now_ms();
    const bool ok = host::pairing_eq2(G1::from_affine_lem(AB).neg(), tau_l, G1::from_affine_lem(AB + 64), g2);
    pairing_ms += now_ms() - t0;
    checks++;
    return ok;
  }
  // [lo, hi) is known to hold an opening that fails the equation
  void locate(uint64_t lo, uint64_t hi) {
    if (hi - lo == 1) {
      valid[lo] = 0;
      return;
    }
    const uint64_t mid = lo + (hi - lo) / 2;
    if (check(lo, mid)) {
      locate(mid, hi);  // the left half passes under a failing parent: the right half fails
    } else {
      locate(lo, mid);
      if (!check(mid, hi)) locate(mid, hi);
    }
  }
};

int verify_cosets_impl(kgs_ctx* ctx, const Batch& b, bool device, const uint8_t* tau_l_g2, const uint8_t* seed32,
                       uint8_t* valid_out, kgs_coset_batch_diag_t* diag) {
  const char* fn = device ? "kgs_kzg_verify_cosets_batch_device" : "kgs_kzg_verify_cosets_batch";
  if (diag) {
    diag->pairing_checks = 0;
    diag->on_gpu = 0;
    diag->hash_ms = diag->fold_ms = diag->pairing_ms = 0;
  }
  if (device && !ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  if (device && !seed32)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": the seed is not derived from device buffers, give seed32");
  if (b.nbits < 0 || b.nbits > (ctx ? CB_NBITS_CTX : CB_NBITS_HOST) || b.lbits < 0 || b.lbits > b.nbits)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " +
                                  std::to_string(ctx ? CB_NBITS_CTX : CB_NBITS_HOST) + ", lbits in 0 .. nbits");
  if (!tau_l_g2) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL tau_l_g2");
  const host::G2A t2 = host::g2_from_lem(tau_l_g2);
  if (!host::g2_on_curve(t2)) throw KgsError(KGS_E_ARG, std::string(fn) + ": tau_l_g2 is not on the curve");
  if (b.count && (!b.commit_of || !b.index || !b.ys || !b.proofs || !b.srs || (b.ncommits && !b.commits)))
    throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL buffer");
  if (b.count > CB_MAX_VALUES || b.ncommits > CB_MAX_VALUES || (ctx && (b.count << b.lbits) > CB_MAX_VALUES))
    throw KgsError(KGS_E_ARG, std::string(fn) + ": at most 2^26 openings, commitments and (with a context) values");
  std::unique_lock<std::mutex> lk;
  if (ctx) {
    lk = std::unique_lock<std::mutex>(ctx->mu);
    check_plain_ctx(*ctx, fn);
  }
  if (!b.count) return 1;

  const uint64_t l = b.l(), nterms = 3 * b.count + l;
  const int force = env_choice("KGS_VERIFY_COSETS_FOLD", "host", "gpu");
  bool gpu = ctx && (force == 1 || (force != 0 && nterms >= CB_GPU_MIN_TERMS));
  if (device) gpu = true;  // the inputs are on the device: they are not copied back
  if (gpu && b.lbits > COSET_FOLD_LBITS_MAX) {
    if (device)
      throw KgsError(KGS_E_ARG, std::string(fn) + ": lbits above " + std::to_string(COSET_FOLD_LBITS_MAX) +
                                    " is folded on the host only");
    gpu = false;
  }

  // an SRS point off the curve: nothing can be checked against it
  for (uint64_t j = 0; j < l; j++)
    if (!host::g1_valid(b.srs + 64 * j)) {
      if (valid_out) memset(valid_out, 0, b.count);
      return 0;
    }

  double t0 = now_ms();
  uint8_t seed[32], rho_std[32];
  if (seed32) memcpy(seed, seed32, 32);
  else derive_seed(b, tau_l_g2, seed);
  const Fr rho = rho_from_seed(seed, rho_std);
  if (diag) diag->hash_ms = now_ms() - t0;
  if (diag && diag->rho_out) memcpy(diag->rho_out, rho_std, 32);

  std::vector<uint8_t> valid(b.count, 1);
  std::unique_ptr<Folder> folder;
  std::unique_ptr<DrainOnError> drain;
  if (gpu) {
    HC(hipSetDevice(ctx->device));
    drain.reset(new DrainOnError(ctx));
    folder.reset(new GpuFolder(*ctx, b, device));
  } else {
    folder.reset(new HostFolder(b));
  }
  t0 = now_ms();
  folder->prepare(rho, valid);
  Bisect bs{*folder, valid, t2};
  bs.diag = diag;
  bs.fold_ms = now_ms() - t0;
  // the whole batch; the structural verdicts are complete once its fold has run
  const bool pass = bs.check(0, b.count);
  bool all = pass;
  for (uint64_t k = 0; k < b.count && all; k++) all = valid[k] != 0;
  if (!pass && b.count == 1) valid[0] = 0;
  else if (!pass && valid_out) bs.locate(0, b.count);
  if (gpu) HC(hipStreamSynchronize(ctx->st));
  if (valid_out) memcpy(valid_out, valid.data(), b.count);
  if (diag) {
    diag->pairing_checks = bs.checks;
    diag->on_gpu = gpu ? 1 : 0;
    diag->fold_ms = bs.fold_ms;
    diag->pairing_ms = bs.pairing_ms;
  }
  return all ? 1 : 0;
}

int interp_fold_impl(kgs_ctx* ctx, int nbits, int lbits, const void* index, const void* ys, const void* weights,
                     uint64_t count, void* out, bool device) {
  const char* fn = device ? "kgs_coset_interp_fold_device" : "kgs_coset_interp_fold";
  if (device && !ctx) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL ctx");
  if (nbits < 0 || nbits > (ctx ? CB_NBITS_CTX : CB_NBITS_HOST) || lbits < 0 || lbits > nbits)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": nbits must be in 0 .. " +
                                  std::to_string(ctx ? CB_NBITS_CTX : CB_NBITS_HOST) + ", lbits in 0 .. nbits");
  if (!out || (count && (!index || !ys || !weights))) throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument");
  if (count > CB_MAX_VALUES || (count << lbits) > CB_MAX_VALUES)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": at most 2^26 values");
  const uint64_t l = 1ull << lbits, m = 1ull << (nbits - lbits);
  if (!ctx) {
    const uint64_t* idx = (const uint64_t*)index;
    std::vector<Fr> w(count);
    for (uint64_t k = 0; k < count; k++) {
      if (idx[k] >= m) throw KgsError(KGS_E_ARG, std::string(fn) + ": index " + std::to_string(k) + " is not below m");
      if (!host::lt_mod((const uint8_t*)weights + 32 * k, host::FR_MOD.p))
        throw KgsError(KGS_E_ARG, std::string(fn) + ": weight " + std::to_string(k) + " is not below r");
      w[k] = Fr::from_bytes((const uint8_t*)weights + 32 * k);
      for (uint64_t j = 0; j < l && !w[k].is_zero(); j++)
        if (!host::lt_mod((const uint8_t*)ys + 32 * (k * l + j), host::FR_MOD.p))
          throw KgsError(KGS_E_ARG, std::string(fn) + ": a value of row " + std::to_string(k) + " is not below r");
    }
    const std::vector<Fr> D = interp_fold_host(nbits, lbits, idx, (const uint8_t*)ys, w.data(), nullptr, 0, count);
    for (uint64_t j = 0; j < l; j++) D[j].to_bytes((uint8_t*)out + 32 * j);
    return KGS_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn);
  if (lbits > COSET_FOLD_LBITS_MAX)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": with a context lbits must be in 0 .. " +
                                  std::to_string(COSET_FOLD_LBITS_MAX));
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(ctx);
  need_domain(c, nbits);
  const uint32_t *d_ys = (const uint32_t*)ys, *d_w = (const uint32_t*)weights;
  const uint64_t* d_idx = (const uint64_t*)index;
  if (!device && count) {
    uint32_t* a = c.buf("cb_ys", 32 * count * l);
    uint32_t* w = c.buf("cb_w", 32 * count);
    uint32_t* i = c.buf("cb_idx", 8 * count);
    HC(hipMemcpyAsync(a, ys, 32 * count * l, hipMemcpyHostToDevice, c.st));
    HC(hipMemcpyAsync(w, weights, 32 * count, hipMemcpyHostToDevice, c.st));
    HC(hipMemcpyAsync(i, index, 8 * count, hipMemcpyHostToDevice, c.st));
    d_ys = a, d_w = w, d_idx = (const uint64_t*)i;
  }
  uint32_t* d_small = c.buf("cb_small", 256);
  HC(hipMemsetAsync(d_small, 0, 256, c.st));
  uint32_t* d_out = device ? (uint32_t*)out : c.buf("cb_D", 32 * l);
  interp_fold_gpu(c, d_out, nullptr, d_small + 8, d_ys, d_idx, d_w, count, nbits, lbits);
  uint32_t bad = 0;
  if (!device) HC(hipMemcpyAsync(out, d_out, 32 * l, hipMemcpyDeviceToHost, c.st));
  HC(hipMemcpyAsync(&bad, d_small + 8, 4, hipMemcpyDeviceToHost, c.st));
  HC(hipStreamSynchronize(c.st));
  if (bad) throw KgsError(KGS_E_ARG, std::string(fn) + ": an index is not below m or a value is not below r");
  return KGS_OK;
}

}  // namespace

extern "C" {

int kgs_kzg_verify_cosets_batch(kgs_ctx_t* ctx, int nbits, int lbits, const uint8_t* commits_lem, uint64_t ncommits,
                                const uint32_t* commit_of, const uint64_t* index, const uint8_t* ys_mont,
                                const uint8_t* proofs_lem, uint64_t count, const uint8_t* srs_g1_lem,
                                const uint8_t tau_l_g2[128], const uint8_t* seed32, uint8_t* valid_out,
                                kgs_coset_batch_diag_t* diag) {
  API_BEGIN
  const Batch b{nbits, lbits, commits_lem, ncommits, commit_of, index, ys_mont, proofs_lem, count, srs_g1_lem};
  return verify_cosets_impl(ctx, b, false, tau_l_g2, seed32, valid_out, diag);
  API_END
}

int kgs_kzg_verify_cosets_batch_device(kgs_ctx_t* ctx, int nbits, int lbits, const uint8_t* commits_lem,
                                       uint64_t ncommits, const void* d_commit_of, const void* d_index,
                                       const void* d_ys_mont, const void* d_proofs_lem, uint64_t count,
                                       const uint8_t* srs_g1_lem, const uint8_t tau_l_g2[128], const uint8_t* seed32,
                                       uint8_t* valid_out, kgs_coset_batch_diag_t* diag) {
  API_BEGIN
  const Batch b{nbits, lbits, commits_lem, ncommits, (const uint32_t*)d_commit_of, (const uint64_t*)d_index,
                (const uint8_t*)d_ys_mont, (const uint8_t*)d_proofs_lem, count, srs_g1_lem};
  return verify_cosets_impl(ctx, b, true, tau_l_g2, seed32, valid_out, diag);
  API_END
}

int kgs_coset_interp_fold(kgs_ctx_t* ctx, int nbits, int lbits, const uint64_t* index, const uint8_t* ys_mont,
                          const uint8_t* weights_mont, uint64_t count, uint8_t* out_mont) {
  API_BEGIN
  return interp_fold_impl(ctx, nbits, lbits, index, ys_mont, weights_mont, count, out_mont, false);
  API_END
}

int kgs_coset_interp_fold_device(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                 const void* d_weights_mont, uint64_t count, void* d_out_mont) {
  API_BEGIN
  return interp_fold_impl(ctx, nbits, lbits, d_index, d_ys_mont, d_weights_mont, count, d_out_mont, true);
  API_END
}

int kgs_bench_coset_interp_fold(kgs_ctx_t* ctx, int nbits, int lbits, const void* d_index, const void* d_ys_mont,
                                const void* d_weights_mont, uint64_t count, int reps, double* ms) {
  API_BEGIN
  const char* fn = "kgs_bench_coset_interp_fold";
  if (!ctx || !ms || reps < 1 || !count || !d_index || !d_ys_mont || !d_weights_mont)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": NULL argument, no rows or no repetitions");
  if (nbits < 0 || nbits > CB_NBITS_CTX || lbits < 0 || lbits > nbits || lbits > COSET_FOLD_LBITS_MAX ||
      (count << lbits) > CB_MAX_VALUES)
    throw KgsError(KGS_E_ARG, std::string(fn) + ": sizes out of range");
  std::lock_guard<std::mutex> lk(ctx->mu);
  check_plain_ctx(*ctx, fn);
  HC(hipSetDevice(ctx->device));
  kgs_ctx& c = *ctx;
  DrainOnError drain(ctx);
  need_domain(c, nbits);
  uint32_t* d_small = c.buf("cb_small", 256);
  uint32_t* d_out = c.buf("cb_D", 32ull << lbits);
  HC(hipMemsetAsync(d_small, 0, 256, c.st));
  EventTimer timer;
  for (int r = -1; r < reps; r++) {  // run -1 warms up
    const double t = timer.ms(c.st, [&] {
      interp_fold_gpu(c, d_out, nullptr, d_small + 8, (const uint32_t*)d_ys_mont, (const uint64_t*)d_index,
                      (const uint32_t*)d_weights_mont, count, nbits, lbits);
    });
    if (r >= 0) ms[r] = t;
  }
  API_END
}

}  // extern "C"
