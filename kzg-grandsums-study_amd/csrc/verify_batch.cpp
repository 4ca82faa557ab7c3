// Batch verifier and the segmented G1 linear combination behind it: kgs_verify_batch,
// kgs_verify_batch_ptau, kgs_g1_lincomb (include/kgs.h; DESIGN.md "Batch verifier").
//
// Host: structural screening, transcript replay and Fr arithmetic per proof (verify_linear.hpp), the
// weights, the aggregate pairing check and the bisection that locates invalid proofs. GPU: the fold
// of every proof's rho_i * A_i and rho_i * B_i (fold.hip) on the context's main stream, in device
// buffers of its own ("fold_*" in the context's pool, grown on demand, sized by the term count).
#include <chrono>
#include <mutex>

#include "context.hpp"
#include "host_pairing.hpp"
#include "keccak.hpp"
#include "verify_linear.hpp"

using host::G1;

namespace {

constexpr uint64_t FOLD_MAX = 1ull << 26;  // terms / segments of one fold (device offsets are 32-bit)

// A batch of fewer terms folds on the host even with a context. Measured on MI355X (DESIGN.md "Batch
// verifier"): the GPU fold takes 4.4 - 4.8 ms whatever the batch size up to 4096 proofs (one wave per
// SIMD does 256 dependent double-and-add steps), the host fold 0.034 ms per term: they cross at about
// 130 terms, 11 - 12 proofs.
constexpr uint64_t VB_GPU_MIN_TERMS = 128;

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void fold_host(const uint8_t* points, const uint8_t* scalars, const uint64_t* seg_off, uint64_t nseg, uint8_t* out) {
  for (uint64_t s = 0; s < nseg; s++) {
    const uint64_t lo = seg_off[s], hi = seg_off[s + 1];
    host::g1_lincomb_segment(points + 64 * lo, scalars + 32 * lo, hi - lo).to_affine_lem(out + 64 * s);
  }
}

// The fold on the context's device (the caller holds the context's mutex and has set the device).
// Returns with the main stream drained, also when it throws.
void fold_gpu(kgs_ctx& c, const uint8_t* points, const uint8_t* scalars, const uint64_t* seg_off, uint64_t nseg,
              uint8_t* out) {
  const uint64_t nterms = seg_off[nseg];
  std::vector<uint32_t> off32(nseg + 1);
  for (uint64_t s = 0; s <= nseg; s++) off32[s] = (uint32_t)seg_off[s];
  try {
    uint32_t* d_pts = c.buf("fold_pts", 64 * nterms);
    uint32_t* d_sc = c.buf("fold_sc", 32 * nterms);
    uint32_t* d_off = c.buf("fold_off", 4 * (nseg + 1));
    uint32_t* d_term = c.buf("fold_term", 128 * nterms);
    uint32_t* d_seg = c.buf("fold_seg", 128 * nseg);
    uint32_t* d_scr = c.buf("fold_scr", 32 * nseg);
    uint32_t* d_out = c.buf("fold_out", 64 * nseg);
    if (nterms) {
      HC(hipMemcpyAsync(d_pts, points, 64 * nterms, hipMemcpyHostToDevice, c.st));
      HC(hipMemcpyAsync(d_sc, scalars, 32 * nterms, hipMemcpyHostToDevice, c.st));
    }
    HC(hipMemcpyAsync(d_off, off32.data(), 4 * (nseg + 1), hipMemcpyHostToDevice, c.st));
    launch_g1_fold(c.st, d_out, d_pts, d_sc, d_off, nterms, nseg, d_term, d_seg, d_scr);
    check_launch();
    HC(hipMemcpyAsync(out, d_out, 64 * nseg, hipMemcpyDeviceToHost, c.st));
    HC(hipStreamSynchronize(c.st));
  } catch (...) {
    (void)hipStreamSynchronize(c.st);
    (void)hipGetLastError();
    throw;
  }
}

void check_segments(const uint64_t* seg_off, uint64_t nseg) {
  if (nseg > FOLD_MAX) throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: at most 2^26 segments");
  if (seg_off[0] != 0) throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: seg_off[0] must be 0");
  for (uint64_t s = 0; s < nseg; s++)
    if (seg_off[s + 1] < seg_off[s]) throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: seg_off must not decrease");
  if (seg_off[nseg] > FOLD_MAX) throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: at most 2^26 terms");
}

struct CtxUse {  // the context's mutex and device for the rest of the call (no-op without a context)
  std::unique_lock<std::mutex> lk;
  explicit CtxUse(kgs_ctx* c, const char* what) {
    if (!c) return;
    lk = std::unique_lock<std::mutex>(c->mu);
    check_no_group(*c, what);  // MSM sharding is not refused here
    HC(hipSetDevice(c->device));
  }
};

void put_le32(std::vector<uint8_t>& v, uint32_t x) {
  for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i)));
}

// -1: no override, 0: host, 1: gpu
int fold_override() {
  const char* e = getenv("KGS_VERIFY_BATCH_FOLD");
  if (!e) return -1;
  if (!strcmp(e, "host")) return 0;
  if (!strcmp(e, "gpu")) return 1;
  return -1;
}

struct Bisect {
  const std::vector<G1>&PA, &PB;  // prefix sums of the folded points over the structurally valid proofs
  const std::vector<int>& idx;    // their positions in the batch
  const host::G2A& tau;
  host::G2A g2;
  uint8_t* valid;
  uint32_t checks = 0;
  double ms = 0;

  bool check(size_t lo, size_t hi) {
    const double t0 = now_ms();
    const G1 A = PA[hi].add(PA[lo].neg()), B = PB[hi].add(PB[lo].neg());
    const bool ok = host::pairing_eq2(A.neg(), tau, B, g2);
    checks++;
    ms += now_ms() - t0;
    return ok;
  }
  // [lo, hi) is known to hold an invalid proof
  void locate(size_t lo, size_t hi) {
    if (hi - lo == 1) {
      valid[idx[lo]] = 0;
      return;
    }
    const size_t mid = lo + (hi - lo) / 2;
    if (check(lo, mid)) {
      locate(mid, hi);  // the left half passes under a failing parent: the right half fails
    } else {
      locate(lo, mid);
      if (!check(mid, hi)) locate(mid, hi);
    }
  }
};

int verify_batch_impl(kgs_ctx* ctx, const kgs_proof_ref_t* proofs, int count, const uint8_t* tau_g2, uint8_t* valid_out,
                      kgs_batch_diag_t* diag) {
  if (diag) {
    diag->pairing_checks = diag->terms = 0;
    diag->on_gpu = 0;
    diag->fold_ms = diag->pairing_ms = 0;
  }
  if (count < 0 || !tau_g2 || (count && !proofs)) throw KgsError(KGS_E_ARG, "kgs_verify_batch: NULL argument or negative count");
  const host::G2A t2 = host::g2_from_lem(tau_g2);
  if (!host::g2_on_curve(t2)) throw KgsError(KGS_E_ARG, "kgs_verify_batch: tau_g2 is not on the curve");
  size_t seed_len = 19 + 128 + 4;
  for (int i = 0; i < count; i++) {
    const kgs_proof_ref_t& q = proofs[i];
    const std::string at = "kgs_verify_batch: proof " + std::to_string(i) + ": ";
    if (q.kind != KGS_GRANDSUM && q.kind != KGS_GRANDPRODUCT && q.kind != KGS_LOOKUP) throw KgsError(KGS_E_ARG, at + "unknown kind");
    if (q.kind == KGS_LOOKUP && !q.selected) throw KgsError(KGS_E_ARG, at + "a lookup proof needs its selectors");
    if (q.nbits < 1 || q.nbits > 28) throw KgsError(KGS_E_ARG, at + "nbits must be in 1 .. 28");
    if (q.npols < 1 || q.npols > (1 << 20)) throw KgsError(KGS_E_ARG, at + "npols must be in 1 .. 2^20");
    if (!q.commitments || !q.evaluations) throw KgsError(KGS_E_ARG, at + "NULL buffer");
    int nc = 0, ne = 0;
    kgs_proof_shape(q.kind, q.npols, q.selected, &nc, &ne);
    seed_len += 16 + 64 * (size_t)nc + 32 * (size_t)ne;
  }
  CtxUse use(ctx, "The batch verifier");
  if (count == 0) return 1;

  // weights
  std::vector<uint8_t> msg;
  msg.reserve(seed_len);
  static const char tag[] = "kgs-verify-batch-v1";
  msg.insert(msg.end(), tag, tag + 19);
  msg.insert(msg.end(), tau_g2, tau_g2 + 128);
  put_le32(msg, (uint32_t)count);
  std::vector<host::Proof> ps(count);
  for (int i = 0; i < count; i++) {
    const kgs_proof_ref_t& q = proofs[i];
    ps[i] = host::Proof{q.npols, q.selected != 0, q.kind != KGS_GRANDPRODUCT, q.commitments, q.evaluations, q.kind == KGS_LOOKUP};
    put_le32(msg, (uint32_t)q.kind);
    put_le32(msg, (uint32_t)q.nbits);
    put_le32(msg, (uint32_t)q.npols);
    put_le32(msg, (uint32_t)(q.selected ? 1 : 0));
    msg.insert(msg.end(), q.commitments, q.commitments + 64 * (size_t)ps[i].ncom());
    msg.insert(msg.end(), q.evaluations, q.evaluations + 32 * (size_t)ps[i].nev());
  }
  uint8_t seed[36];
  host::keccak256(msg.data(), msg.size(), seed);
  std::vector<uint8_t>().swap(msg);
  std::vector<Fr> rho(count);
  for (int i = 0; i < count; i++) {
    uint8_t h[32];
    for (int k = 0; k < 4; k++) seed[32 + k] = (uint8_t)((uint32_t)i >> (8 * k));
    host::keccak256(seed, 36, h);
    uint64_t s[4] = {0, 0, 0, 0};
    memcpy(s, h, 16);
    if (!(s[0] | s[1])) s[0] = 1;
    rho[i] = Fr::from_std(s);
    if (diag && diag->weights_out) memcpy(diag->weights_out + 32 * (size_t)i, s, 32);
  }

  // terms: segment 2i = rho_i * A_i, segment 2i + 1 = rho_i * B_i; both empty for a proof that fails
  // the structural checks
  std::vector<uint8_t> valid(count, 1);
  std::vector<uint64_t> seg_off(2 * (size_t)count + 1, 0);
  std::vector<uint8_t> pts, scs;
  uint8_t gen[64];
  host::g1_gen_lem(gen);
  auto term = [&](const uint8_t* p, const Fr& s) {
    pts.insert(pts.end(), p, p + 64);
    uint64_t w[4];
    s.to_std(w);
    const uint8_t* b = (const uint8_t*)w;
    scs.insert(scs.end(), b, b + 32);
  };
  std::vector<int> idx;
  for (int i = 0; i < count; i++) {
    const host::Proof& p = ps[i];
    if (!host::proof_structure_ok(p)) {
      valid[i] = 0;
      seg_off[2 * (size_t)i + 1] = seg_off[2 * (size_t)i + 2] = pts.size() / 64;
      continue;
    }
    idx.push_back(i);
    const host::LinearForm lf = host::linear_form(p, proofs[i].nbits);
    term(p.Wxi(), rho[i] * lf.a_wxi);
    term(p.Wxiw(), rho[i] * lf.a_wxiw);
    seg_off[2 * (size_t)i + 1] = pts.size() / 64;
    for (int j = 0; j < p.ncom(); j++) term(p.C(j), rho[i] * lf.b[j]);
    term(gen, rho[i] * lf.b_g);
    seg_off[2 * (size_t)i + 2] = pts.size() / 64;
  }
  const uint64_t nseg = 2 * (uint64_t)count, nterms = pts.size() / 64;
  if (nterms > FOLD_MAX) throw KgsError(KGS_E_ARG, "kgs_verify_batch: more than 2^26 terms in one batch");

  // the fold
  const int force = fold_override();
  const bool gpu = ctx && (force == 1 || (force != 0 && nterms >= VB_GPU_MIN_TERMS));
  std::vector<uint8_t> folded(64 * nseg);
  double t0 = now_ms();
  if (gpu)
    fold_gpu(*ctx, pts.data(), scs.data(), seg_off.data(), nseg, folded.data());
  else
    fold_host(pts.data(), scs.data(), seg_off.data(), nseg, folded.data());
  const double fold_ms = now_ms() - t0;
  if (diag && diag->folded_out) memcpy(diag->folded_out, folded.data(), folded.size());

  // aggregate check, then bisection over the per-proof points
  const size_t m = idx.size();
  std::vector<G1> PA(m + 1), PB(m + 1);
  PA[0] = PB[0] = G1::inf();
  for (size_t j = 0; j < m; j++) {
    PA[j + 1] = PA[j].add(G1::from_affine_lem(&folded[128 * (size_t)idx[j]]));
    PB[j + 1] = PB[j].add(G1::from_affine_lem(&folded[128 * (size_t)idx[j] + 64]));
  }
  Bisect bs{PA, PB, idx, t2, host::g2_gen(), valid.data()};
  bool all = m == (size_t)count;
  if (m && !bs.check(0, m)) {
    all = false;
    if (valid_out) bs.locate(0, m);
  }
  if (valid_out) memcpy(valid_out, valid.data(), count);
  if (diag) {
    diag->pairing_checks = bs.checks;
    diag->terms = (uint32_t)nterms;
    diag->on_gpu = gpu ? 1 : 0;
    diag->fold_ms = fold_ms;
    diag->pairing_ms = bs.ms;
  }
  return all ? 1 : 0;
}

}  // namespace

extern "C" {

int kgs_verify_batch(kgs_ctx_t* ctx, const kgs_proof_ref_t* proofs, int count, const uint8_t tau_g2[128],
                     uint8_t* valid_out, kgs_batch_diag_t* diag) {
  API_BEGIN
  return verify_batch_impl(ctx, proofs, count, tau_g2, valid_out, diag);
  API_END
}

int kgs_verify_batch_ptau(kgs_ctx_t* ctx, const char* ptau_path, const kgs_proof_ref_t* proofs, int count,
                          uint8_t* valid_out, kgs_batch_diag_t* diag) {
  uint8_t t2[128];
  const int rc = kgs_ptau_read_tau_g2(ptau_path, t2);
  if (rc < 0) return rc;
  return kgs_verify_batch(ctx, proofs, count, t2, valid_out, diag);
}

int kgs_g1_lincomb(kgs_ctx_t* ctx, const uint8_t* points_lem, const uint8_t* scalars_std, const uint64_t* seg_off,
                   uint64_t nseg, uint8_t* out_lem) {
  API_BEGIN
  if (!seg_off || (nseg && !out_lem)) throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: NULL argument");
  check_segments(seg_off, nseg);
  const uint64_t nterms = seg_off[nseg];
  if (nterms && (!points_lem || !scalars_std)) throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: NULL argument");
  for (uint64_t t = 0; t < nterms; t++)
    if (!host::g1_valid(points_lem + 64 * t))
      throw KgsError(KGS_E_ARG, "kgs_g1_lincomb: point " + std::to_string(t) + " is not on the curve");
  CtxUse use(ctx, "kgs_g1_lincomb");
  if (!nseg) return KGS_OK;
  if (ctx)
    fold_gpu(*ctx, points_lem, scalars_std, seg_off, nseg, out_lem);
  else
    fold_host(points_lem, scalars_std, seg_off, nseg, out_lem);
  API_END
}

}  // extern "C"
