// The distributed prover: one proof over a group of W ranks (one context per rank, one GPU each
// on a node), every vector sharded, so that the NTTs, the builder, the quotient, the Horner
// evaluations, the synthetic divisions AND the MSMs all shrink as 1/W per rank (SURVEY.md §8e;
// north_star: "the MSM and NTT shard ... by scalar/point range and by butterfly stage").
//
// This file holds the five rounds. What they stand on lives beside it: dist_layout.hpp (struct Dist: the
// BLOCK / CYCLIC / E layouts, the exchange steps between them and the exchange accounting; specified and
// checked on CPU by tests/test_dist_layouts.py), dist_math.hpp (the host arithmetic on all-gathered
// values between the kernel launches; checked by tests/native/dist_math_check.cpp), dist.hip (the
// rank-local kernels), dist_group.cpp (the transports behind kgs_group and the kgs_group_* entry points)
// and transcript.hpp (the Fiat-Shamir schedule, shared with the round engine and the verifiers).
//
// Per grand-sum proof (k = 1, no selectors) the data exchanges are 10 all-to-alls of one vector each
// (RCCL send/recv over xGMI, stream-ordered) plus a handful of small host all-gathers (rank totals,
// halos, Horner partials, division carries, MSM bit-sum partials). Every rank ends with the identical
// proof; inputs are the full vectors on every rank (each rank reads only its slices), outputs identical
// to the single-GPU prover byte for byte.
//
//   round 1  F_i, T_i: H-evaluations gathered in E layout -> iDFT (E -> CYCLIC) -> MSM over the
//            rank's CYCLIC slice (SRS points r, r + W, ...)
//   round 2  builder on BLOCK slices + one all-gather of rank totals (prefix offsets, the "not well
//            calculated" check) -> BLOCK -> E -> iDFT -> S (CYCLIC); coset DFTs CYCLIC -> E
//   round 3  divisibility check on BLOCK (one halo element), quotient on E (rot halo elements per
//            block), inverse coset DFT E -> CYCLIC -> MSM
//   round 4  Horner on CYCLIC slices at x^W, combined as sum_r x^r v_r after one all-gather
//   round 5  linear combination on CYCLIC -> BLOCK -> synthetic division with one all-gather of
//            carries (Polynomial.divByXSubValue, polynomial.js:814-851) -> MSM over BLOCK ranges
#include "context.hpp"
#include "dist_layout.hpp"
#include "dist_math.hpp"
#include "transcript.hpp"

using namespace kgs;
using namespace kgsi;

namespace kgsi {

// Rank-local preconditions (SRS loaded and large enough, the loaded SRS slice matching this rank,
// pinned staging): a rank failing one of them must not leave its peers waiting in the first
// exchange, so every rank decides them together — one all-gather of each rank's first failure, and
// every rank throws the lowest failing rank's error (the group stays usable: nothing was exchanged).
void dist_preconditions(kgs_ctx& c, const ProveIn& in) {
  const int W = c.group->world, r = c.group_rank;
  struct Verdict {
    int32_t code;
    char msg[252];
  } mine{};
  try {
    const int nbits = in.nbits, k = in.npols;
    const int logW = ilog2(W);
    if ((1 << logW) != W || W > 16) throw KgsError(KGS_E_ARG, "distributed prover: world must be 1, 2, 4, 8 or 16");
    if (nbits < 2 * logW + 1) throw KgsError(KGS_E_ARG, "distributed prover: domain too small for the group (need n >= 2 W^2)");
    if (c.srs_power < 0) throw KgsError(KGS_E_ARG, "no SRS loaded");
    if (c.srs_power < nbits)
      throw KgsError(KGS_E_SRS, "The Powers of Tau file is not sufficiently large to commit the polynomials.");
    if (nbits > c.nbits_max) throw KgsError(KGS_E_SRS, "SRS loaded for a smaller maximum domain; reload with larger nbits_max");
    if (c.srs_slice_world > 1 && (c.srs_slice_world != W || c.srs_slice_rank != r))
      throw KgsError(KGS_E_ARG, "the loaded SRS slice (rank " + std::to_string(c.srs_slice_rank) + " of " +
                                    std::to_string(c.srs_slice_world) + ") is not this context's (rank " + std::to_string(r) +
                                    " of " + std::to_string(W) + ")");
    if (k < 1) throw KgsError(KGS_E_ARG, "The number of multisets must be greater than 0.");
    if (k > KGS_MAX_POLS) throw KgsError(KGS_E_ARG, "too many multisets");
    const uint64_t M = (1ull << nbits) / W;
    const int ncom_all = 2 * k + (in.sel_f ? 2 : 0) + 4;
    c.msm_slots = ncom_all + 4;
    c.ensure_pin(((size_t)ncom_all + 8) * ((size_t)c.tb.c * 128 + 64) +
                 32 * (size_t)((M + EVAL_TILE - 1) / EVAL_TILE) * (2 * k + 8) + ((size_t)kgs_ctx::SCAL_BYTES * 2) +
                 (8 << 20));
  } catch (const KgsError& e) {
    mine.code = e.code;
    snprintf(mine.msg, sizeof(mine.msg), "%s", e.what());
  } catch (const std::exception& e) {
    mine.code = KGS_E_HIP;
    snprintf(mine.msg, sizeof(mine.msg), "%s", e.what());
  }
  std::vector<Verdict> all(W);
  c.group->allgather(r, &mine, all.data(), sizeof(Verdict));
  for (int j = 0; j < W; j++)
    if (all[j].code != KGS_OK) {
      all[j].msg[sizeof(all[j].msg) - 1] = 0;
      throw KgsError(all[j].code, j == r ? std::string(all[j].msg)
                                         : std::string(all[j].msg) + " (on rank " + std::to_string(j) + ")");
    }
}

namespace {

// One distributed proof on this rank: what the five rounds hand to each other. Device pointers are this
// rank's slices (B: BLOCK of H, c: CYCLIC coefficients, cos*: E layout over the coset domain).
// Preconditions: dist_preconditions (decided by every rank together).
struct DistProof {
  kgs_ctx& c;
  const ProveIn& in;
  Dist D;
  const int W, r;
  const bool gs, lk, sel;  // KGS_LOOKUP is a selected grand-sum
  const int k, nbits;
  const uint64_t n, M;  // M: local length of an n-vector in every layout
  const size_t EM;
  const uint32_t ntiles;
  const ArgIn arg;
  uint32_t* flags = nullptr;
  // round 1
  std::vector<uint32_t*> fB, tB;
  ArgPolys P;  // Fc, Tc, sFc, sTc, then Sc, polT (round 2) and Qc (round 3)
  const uint32_t *sFB = nullptr, *sTB = nullptr;
  std::vector<uint8_t> com;  // proof order
  int ci = 0, slot = 0;
  host::Schedule sched;
  // round 2
  Fr beta, gamma;
  const uint32_t *fcomb = nullptr, *tcomb = nullptr, *polF = nullptr;
  uint32_t *SB = nullptr, *d_offs = nullptr;
  int lcs = 0;
  uint64_t cs = 0, Mc = 0;  // the coset domain and its local length
  uint32_t *cosS = nullptr, *cosF = nullptr, *cosT = nullptr, *cosSF = nullptr, *cosST = nullptr, *nxm1 = nullptr;
  // rounds 3 to 5
  Fr alpha, xi, xiw, sxiw;
  uint32_t* Qc = nullptr;
  uint64_t qlen = 0;  // deg Q + 1 bound
  XiEvals x;
  std::vector<Fr> evals;  // proof order

  DistProof(kgs_ctx& cc, const ProveIn& pin)
      : c(cc), in(pin), D(cc), W(D.W), r(D.r), gs(pin.kind != KGS_GRANDPRODUCT), lk(pin.kind == KGS_LOOKUP),
        sel(pin.sel_f != nullptr), k(pin.npols), nbits(pin.nbits), n(1ull << pin.nbits), M(n / W), EM(32 * M),
        ntiles((uint32_t)((M + EVAL_TILE - 1) / EVAL_TILE)), arg(pin.arg()),
        com(64 * (size_t)(2 * pin.npols + (pin.sel_f ? 2 : 0) + 4)) {
    c.reset_staging();
    flags = c.buf("flags", 64);
    HC(hipMemsetAsync(flags, 0, 64, c.st));
  }

  uint8_t* com_at(int i) { return com.data() + 64 * (size_t)i; }
  // CYCLIC slice: scalar j of rank r multiplies SRS point r + W j
  Commit commit_cyc(const uint32_t* sc, uint64_t N) {
    return commit_launch_slice(c, sc, D.cyc_count(N), (uint64_t)r, (uint64_t)W, N, slot++, 0);
  }
  // the next commitments of the proof from their per-rank partials
  void finish_commits(const std::vector<Commit>& cms) {
    std::vector<uint8_t*> outs;
    for (size_t i = 0; i < cms.size(); i++) outs.push_back(com_at(ci++));
    commits_finish_with(c, cms, outs, W, D.host_ag());
  }

  void round1();
  void round2();
  void round3();
  bool replay_reference_quotient();
  void round4();
  void round5();
};

// ---------------- round 1: witness polynomials + commitments (prover.js:144-179)
void DistProof::round1() {
  fB.resize(k);
  tB.resize(k);
  P.Fc.resize(k);
  P.Tc.resize(k);
  uint32_t* eTmp = c.buf("d_eTmp", EM);
  for (int i = 0; i < k; i++) {
    fB[i] = c.buf("d_fB" + std::to_string(i), EM);
    tB[i] = c.buf("d_tB" + std::to_string(i), EM);
    P.Fc[i] = c.buf("d_Fc" + std::to_string(i), EM);
    P.Tc[i] = c.buf("d_Tc" + std::to_string(i), EM);
    launch_to_mont(c.st, fB[i], in.f_std[i] + (size_t)8 * r * M, M);
    launch_to_mont(c.st, tB[i], in.t_std[i] + (size_t)8 * r * M, M);
    launch_gather_e(c.st, eTmp, in.f_std[i], n, W, r, true);
    D.inv_e_to_cyc(P.Fc[i], eTmp, nbits, false);
    launch_gather_e(c.st, eTmp, in.t_std[i], n, W, r, true);
    D.inv_e_to_cyc(P.Tc[i], eTmp, nbits, false);
  }
  check_launch();
  // Montgomery write-back (prover.js:147-148): every rank returns the caller's full vectors
  bool wb = false;
  for (int i = 0; i < k; i++) wb |= !in.mont_f_out.empty() && (in.mont_f_out[i] || in.mont_t_out[i]);
  if (wb) {
    uint32_t* full = c.buf("d_wb", 32 * n);
    for (int i = 0; i < k; i++)
      for (int ft = 0; ft < 2; ft++) {
        uint8_t* dst = ft ? in.mont_t_out[i] : in.mont_f_out[i];
        if (!dst) continue;
        launch_to_mont(c.st, full, ft ? in.t_std[i] : in.f_std[i], n);
        HC(hipMemcpyAsync(dst, full, 32 * n, hipMemcpyDeviceToHost, c.st));
      }
  }
  if (sel) {
    sFB = in.sel_f + (size_t)8 * r * M;
    sTB = in.sel_t + (size_t)8 * r * M;
    P.sFc = c.buf("d_sFc", EM);
    P.sTc = c.buf("d_sTc", EM);
    launch_gather_e(c.st, eTmp, in.sel_f, n, W, r, false);
    D.inv_e_to_cyc(P.sFc, eTmp, nbits, false);
    launch_gather_e(c.st, eTmp, in.sel_t, n, W, r, false);
    D.inv_e_to_cyc(P.sTc, eTmp, nbits, false);
  }
  std::vector<Commit> r1;
  for (int i = 0; i < k; i++) {
    r1.push_back(commit_cyc(P.Fc[i], n));
    r1.push_back(commit_cyc(P.Tc[i], n));
  }
  if (sel) {
    r1.push_back(commit_cyc(P.sFc, n));
    r1.push_back(commit_cyc(P.sTc, n));
  }
  c.sync();
  if (in.after_round1) in.after_round1();
  finish_commits(r1);
}

// ---------------- round 2: challenges, combined polynomials, S / Z (prover.js:181-231)
void DistProof::round2() {
  const host::Schedule::BetaGamma bg = sched.after_round1(com_at(0), ci, k > 1);
  beta = bg.beta;
  gamma = bg.gamma;
  fcomb = fB[0];
  tcomb = tB[0];
  polF = P.Fc[0];
  P.polT = P.Tc[0];
  if (k > 1) {
    uint32_t* b_fe = c.buf("d_fcomb", EM);
    uint32_t* b_te = c.buf("d_tcomb", EM);
    uint32_t* b_F = c.buf("d_polF", EM);
    uint32_t* b_T = c.buf("d_polT", EM);
    const BetaComb bc = beta_combination(fB, tB, P.Fc, P.Tc, k, beta, M);
    run_lincomb(c.st, b_fe, M, bc.fcomb);
    run_lincomb(c.st, b_te, M, bc.tcomb);
    run_lincomb(c.st, b_F, M, bc.polF);
    run_lincomb(c.st, b_T, M, bc.polT);
    fcomb = b_fe;
    tcomb = b_te;
    polF = b_F;
    P.polT = b_T;
  }
  // builder on this rank's BLOCK of H (local scan), then the cross-rank offsets
  SB = c.buf("d_SB", EM);
  uint32_t* d_gamma = c.scal(&gamma, 1);
  launch_builder(c.st, !gs, sel, SB, fcomb, tcomb, sFB, sTB, d_gamma, M, c.buf("bt_tp", 32 * (ntiles + 1)),
                 c.buf("bt_ti", 32 * (ntiles + 1)), flags + 8);  // flags[8]: the local wrap check, unused
  check_launch();
  uint8_t* h_tot = c.pin(32);
  HC(hipMemcpyAsync(h_tot, SB, 32, hipMemcpyDeviceToHost, c.st));  // SB[0] = local total
  HC(hipStreamSynchronize(c.st));
  const ScanOffsets so = scan_offsets(D.gather_fr({Fr::from_bytes(h_tot)}), r, gs);
  if (!(so.all == (gs ? Fr::zero() : Fr::one())))  // S[0] = the total must be 0 (Z[0] = 1): grandsum.js:55-57, grandproduct.js:50-52
    throw KgsError(KGS_E_NOT_WELL_CALC, gs ? "The grand-sum polynomial S is not well calculated"
                                           : "The grand-product polynomial Z is not well calculated");
  Fr offs[2] = {so.off, so.next};
  d_offs = c.scal(offs, 2);
  launch_scan_fix(c.st, !gs, SB, d_offs, M);
  uint32_t* SE = c.buf("d_SE", EM);
  P.Sc = c.buf("d_Sc", EM);
  D.block_to_e(SE, SB, M);
  D.inv_e_to_cyc(P.Sc, SE, nbits, false);
  Commit cS = commit_cyc(P.Sc, n);
  // round 3's challenge-independent coset evaluations (E layout over the coset domain)
  lcs = (!gs && !sel) ? nbits : nbits + 1;
  cs = 1ull << lcs;
  Mc = cs / W;
  cosS = c.buf("d_cosS", 32 * Mc);
  cosF = c.buf("d_cosF", 32 * Mc);
  cosT = c.buf("d_cosT", 32 * Mc);
  D.fwd_cyc_to_e(cosS, P.Sc, M, lcs, true);
  D.fwd_cyc_to_e(cosF, polF, M, lcs, true);
  D.fwd_cyc_to_e(cosT, P.polT, M, lcs, true);
  if (sel) {
    cosSF = c.buf("d_cosSF", 32 * Mc);
    cosST = c.buf("d_cosST", 32 * Mc);
    D.fwd_cyc_to_e(cosSF, P.sFc, M, lcs, true);
    D.fwd_cyc_to_e(cosST, P.sTc, M, lcs, true);
  }
  // 1/(n (x_i - 1)) for this rank's coset points (cached per shape)
  const std::string nk = "d_nxm1_" + std::to_string(nbits) + "_" + std::to_string(lcs) + "_" + std::to_string(W) + "_" +
                         std::to_string(r);
  nxm1 = D.cached_table(nk, 32 * Mc, [&](uint32_t* t) {
    uint32_t* tmp = c.buf("d_nxm1_tmp", 32 * Mc);
    Fr kk[2] = {Fr::from_u64(KGS_NTT_COSET_GEN), Fr::from_u64(n)};
    uint32_t* d = c.scal(kk, 2);
    launch_nxm1_e(c.st, tmp, c.tw_fwd, lcs, d, d + 8, W, r);
    launch_fr_batch_inv(c.st, t, tmp, Mc);
  });
  c.sync();
  finish_commits({cS});
}

// ---------------- round 3: quotient on a coset (prover.js:233-286)
void DistProof::round3() {
  alpha = sched.after_round2(com_at(ci - 1), 1).alpha;
  const uint32_t rot = (uint32_t)(cs >> nbits);
  qlen = (!gs && !sel) ? n - 1 : 2 * n - 2;
  Fr gn = Fr::from_u64(KGS_NTT_COSET_GEN).pow_u64(n);
  // alpha_t: weight of the selT-binary term (none for a lookup, whose selT holds multiplicities)
  Fr qs[5] = {alpha, gamma, (gn - Fr::one()).inverse(), (gn.neg() - Fr::one()).inverse(), lk ? Fr::zero() : alpha};
  uint32_t* d_qs = c.scal(qs, 5);
  // divisibility on H (BLOCK): S at the next natural index past this block is d_offs[1]
  launch_divcheck(c.st, !gs, sel, flags + 1, SB, fcomb, tcomb, sFB, sTB, d_qs, M, d_offs + 8, (uint64_t)r * M);
  // quotient halo: the first rot coset values of the chunk following each of this rank's blocks
  uint32_t* heads = c.buf("d_heads", 32 * 2 * W);
  launch_e_heads(c.st, heads, cosS, Mc, W, (int)rot);
  check_launch();
  const size_t HB = (size_t)32 * rot;  // one block's head
  uint8_t* h_heads = c.pin(HB * W);
  HC(hipMemcpyAsync(h_heads, heads, HB * W, hipMemcpyDeviceToHost, c.st));
  HC(hipStreamSynchronize(c.st));
  std::vector<uint8_t> all_heads(HB * W * W);
  D.allgather(h_heads, all_heads.data(), HB * W);
  uint8_t* h_halo = c.pin(HB * W);
  for (int k1 = 0; k1 < W; k1++) {
    const HaloSource hs = halo_source(r, W, k1);
    memcpy(h_halo + HB * k1, all_heads.data() + HB * (W * hs.src + hs.blk), HB);
  }
  uint32_t* halo = c.buf("d_halo", 32 * 2 * W);
  HC(hipMemcpyAsync(halo, h_halo, HB * W, hipMemcpyHostToDevice, c.st));
  uint32_t* Qe = c.buf("d_Qe", 32 * Mc);
  Qc = c.buf("d_Qc", 32 * Mc);
  P.Qc = Qc;
  launch_quotient_e(c.st, !gs, sel, Qe, cosS, cosF, cosT, cosSF, cosST, nxm1, d_qs, halo, Mc, W, r, (int)rot);
  check_launch();
  D.inv_e_to_cyc(Qc, Qe, lcs, true);
  const bool replayed = replay_reference_quotient();
  Commit cQ = commit_cyc(Qc, qlen);
  uint32_t* h_flags = (uint32_t*)c.pin(64);
  HC(hipMemcpyAsync(h_flags, flags, 64, hipMemcpyDeviceToHost, c.st));
  c.sync();
  if (!replayed) {
    if (D.gather_or(h_flags[1])) throw KgsError(KGS_E_NOT_DIVISIBLE, "Polynomial is not divisible");
    // Q3: the dividend of the reference's divZh has degree < n exactly when the quotient is zero
    // (degree 0 over all ranks: only global coefficient 0, rank 0's first, can still be nonzero)
    if (c.ref_quirks && !lk && D.degrees_cyc({Qc}, Mc)[0] == 0) {
      uint8_t* h0 = c.pin(32);
      HC(hipMemcpyAsync(h0, Qc, 32, hipMemcpyDeviceToHost, c.st));
      HC(hipStreamSynchronize(c.st));
      uint32_t nz = 0;
      for (int b = 0; b < 32; b++) nz |= h0[b];
      if (!D.gather_or(nz)) throw KgsError(KGS_E_RANGE, "offset is out of bounds");
    }
  }
  finish_commits({cQ});
}

// Reference-quirks mode (ref_quirks.cpp; the single-GPU prover does the same in prover_rounds.cpp): where an
// operand of degree 1 <= d < n/2 makes the reference's multiply compute something else (Q1), its
// quotient chain is replayed on the gathered full operands, identically on every rank, and its Q —
// or its error — replaces ours; otherwise only its RangeError on a zero quotient (Q3) differs.
// Every decision here is made from all-gathered values, so all ranks throw the same error together.
// Returns whether the replay's Q (and qlen) replaced ours.
bool DistProof::replay_reference_quotient() {
  if (!c.ref_quirks || lk) return false;
  std::vector<const uint32_t*> ops = {polF, P.polT, P.Sc};
  if (sel) {
    ops.push_back(P.sFc);
    ops.push_back(P.sTc);
  }
  const std::vector<uint64_t> deg = D.degrees_cyc(ops, M);
  bool need = false;
  for (uint64_t d : deg) need |= d >= 1 && 2 * d < n;
  if (!need) return false;
  // Only the replay's own decisions are the same on every rank (made from the gathered full
  // operands): its semantic errors (exempt in prove_dist_group anyway) and its "reference-quirks
  // mode:" refusals. A HIP or allocation failure in the gathers, the domain growth or the replay is
  // this rank's alone, stays un-agreed and aborts the group.
  const uint32_t* fF = D.gather_cyc(polF, M, "d_rq_F");
  const uint32_t* fT = D.gather_cyc(P.polT, M, "d_rq_T");
  const uint32_t* fS = D.gather_cyc(P.Sc, M, "d_rq_S");
  const uint32_t* fSF = sel ? D.gather_cyc(P.sFc, M, "d_rq_SF") : nullptr;
  const uint32_t* fST = sel ? D.gather_cyc(P.sTc, M, "d_rq_ST") : nullptr;
  uint32_t* fmut = nullptr;
  uint64_t qlen_ref = 0;
  const uint32_t* Qref = nullptr;
  try {
    Qref = ref_quirks_quotient(c, gs, sel, lk, nbits, alpha, gamma, fF, fT, fS, fSF, fST, qlen_ref, fmut);
  } catch (const KgsError& e) {
    if (e.code == KGS_E_ARG && e.what() && !strncmp(e.what(), "reference-quirks mode:", 22)) c.dist_err_agreed = true;
    throw;
  }
  if (fmut) {
    c.dist_err_agreed = true;
    throw KgsError(KGS_E_ARG, "reference-quirks mode: the replay wrote into polF's buffer (Q2); not reproduced by a rank group");
  }
  if (qlen_ref > cs) {
    c.dist_err_agreed = true;
    throw KgsError(KGS_E_ARG, "reference-quirks mode: the reference's Q has more coefficients than the group's coset layout");
  }
  // this rank's CYCLIC slice of the reference's Q (coefficients r + W j)
  HC(hipMemsetAsync(Qc, 0, 32 * Mc, c.st));
  const uint64_t cnt = D.cyc_count(qlen_ref);
  if (cnt) HC(hipMemcpy2DAsync(Qc, 32, Qref + 8 * r, (size_t)32 * W, 32, cnt, hipMemcpyDeviceToDevice, c.st));
  qlen = qlen_ref;
  return true;
}

// ---------------- round 4: evaluations (prover.js:288-318): Horner on CYCLIC slices at x^W
void DistProof::round4() {
  xi = sched.after_round3(com_at(ci - 1));
  xiw = xi * fr_w(nbits);
  std::vector<const uint32_t*> esrc;
  arg.each_xi(false, [&](R5Poly id, int i) { esrc.push_back(P.poly(id, i)); });
  EvalJob ej1 = eval_launch(c, esrc, std::vector<uint64_t>(esrc.size(), M), xi.pow_u64((uint64_t)W), 0);
  EvalJob ej2 = eval_launch(c, {P.Sc}, {M}, xiw.pow_u64((uint64_t)W), 1);
  c.sync();
  std::vector<Fr> loc = eval_finish(ej1);
  loc.push_back(eval_finish(ej2)[0]);
  horner_combine(D.gather_fr(loc), loc.size(), W, xi, xiw, evals, sxiw);
  x.unpack(arg, evals.data());
  evals.push_back(sxiw);
}

// ---------------- round 5: linearisation + openings (prover.js:320-413)
void DistProof::round5() {
  const Fr v = sched.after_round4(evals.data(), evals.size());
  LcTerms lw = wxi_numerator({OpenArg{&arg, &P, &x, sxiw}}, nbits, alpha, beta, gamma, {Fr::one()}, xi, v, P.Qc, M,
                             D.cyc_count(qlen));
  if (r != 0) lw.c0 = Fr::zero();  // the constant term lives at global index 0 (rank 0)
  const uint64_t L = qlen > n ? qlen : n;
  // numerator P (CYCLIC over cs >= L points) -> BLOCK -> division by (X - xi) with carries
  uint32_t* Pc = c.buf("d_Pc", 32 * Mc);
  uint32_t* PB = c.buf("d_PB", 32 * Mc);
  uint32_t* WxB = c.buf("d_WxB", 32 * Mc);
  run_lincomb(c.st, Pc, Mc, lw);
  D.cyc_to_block(PB, Pc, Mc);
  const uint32_t dt1 = (uint32_t)((Mc + EVAL_TILE - 1) / EVAL_TILE);
  launch_divide(c.st, WxB, flags + 9, PB, Mc, xpowers(c, xi), c.buf("div_part", 32 * (dt1 + 1)),
                c.buf("div_carry", 32 * (dt1 + 1)));
  EvalJob eR1 = eval_launch(c, {PB}, {Mc}, xi, 2);  // R_lo: this block's value at xi with zero carry-in
  // W_{xi w}: (S - S(xi w)) (CYCLIC over n) -> BLOCK -> division by (X - xi w)
  LcTerms l2;
  l2.add(P.Sc, M, Fr::one());
  l2.c0 = r == 0 ? sxiw.neg() : Fr::zero();
  uint32_t* P2c = c.buf("d_P2c", EM);
  uint32_t* P2B = c.buf("d_P2B", EM);
  uint32_t* W2B = c.buf("d_W2B", EM);
  run_lincomb(c.st, P2c, M, l2);
  D.cyc_to_block(P2B, P2c, M);
  launch_divide(c.st, W2B, flags + 10, P2B, M, xpowers(c, xiw), c.buf("div_part2", 32 * (ntiles + 1)),
                c.buf("div_carry2", 32 * (ntiles + 1)));
  EvalJob eR2 = eval_launch(c, {P2B}, {M}, xiw, 3);
  c.sync();
  const std::vector<Fr> Rl = D.gather_fr({eval_finish(eR1)[0], eval_finish(eR2)[0]});
  Fr c1, c2;  // this rank's carry-ins; the remainders r_0 must be zero
  const bool bad1 = !division_carries(Rl, 0, xi, Mc, W, r, c1).is_zero();
  const bool bad2 = !division_carries(Rl, 1, xiw, M, W, r, c2).is_zero();
  if (bad1 || bad2) throw KgsError(KGS_E_DOES_NOT_DIVIDE, "Polynomial does not divide");
  Fr cc[2] = {c1, c2};
  uint32_t* d_cc = c.scal(cc, 2);
  uint32_t* pz1 = c.buf("d_pz1", 32 * Mc);
  uint32_t* pz2 = c.buf("d_pz2", EM);
  Fr zz[2] = {xi, xiw};
  uint32_t* d_zz = c.scal(zz, 2);
  launch_powers(c.st, pz1, Mc, d_zz, nullptr);
  launch_powers(c.st, pz2, M, d_zz + 8, nullptr);
  launch_div_fix(c.st, WxB, pz1, d_cc, Mc);
  launch_div_fix(c.st, W2B, pz2, d_cc + 8, M);
  check_launch();
  // the openings go back to CYCLIC (one all-to-all each), so that every MSM of the proof reads the
  // same per-rank SRS slice (points r + W j: kgs_srs_load_ptau_slice)
  uint32_t* WxC = c.buf("d_WxC", 32 * Mc);
  uint32_t* W2C = c.buf("d_W2C", EM);
  D.block_to_cyc(WxC, WxB, Mc);
  D.block_to_cyc(W2C, W2B, M);
  Commit cW1 = commit_cyc(WxC, L - 1);
  Commit cW2 = commit_cyc(W2C, n - 1);
  c.sync();
  finish_commits({cW1, cW2});
}

}  // namespace

void prove_dist_impl(kgs_ctx& c, const ProveIn& in, uint8_t* com_out, uint8_t* ev_out) {
  c.timing.resize(9, 0.0);
  for (int i = 0; i < 6; i++) c.timing[i] = 0.0;
  RoundClock clock(c);
  DistProof p(c, in);
  p.round1();
  clock.lap(0);
  p.round2();
  clock.lap(1);
  p.round3();
  clock.lap(2);
  p.round4();
  clock.lap(3);
  p.round5();
  clock.lap(4);
  memcpy(com_out, p.com.data(), p.com.size());
  for (size_t i = 0; i < p.evals.size(); i++) p.evals[i].to_bytes(ev_out + 32 * i);
  c.reset_staging();
  p.D.finish_stats();
}

// Preconditions are agreed by all ranks (dist_preconditions: they all throw together, the group
// stays usable); semantic failures (decided from all-gathered values: the same on every rank) leave
// the group usable too; anything else happened on this rank alone mid-proof and aborts the group, so
// that the other ranks fail at their next exchange instead of waiting in it (RCCL: at the
// KGS_GROUP_TIMEOUT_S deadline of RcclGroup::wait).
extern thread_local int tl_group_rank;  // prover.cpp dev_malloc: per-rank fault injection
void prove_dist_group(kgs_ctx& c, const ProveIn& in, uint8_t* com_out, uint8_t* ev_out) {
  c.xs.reset();
  c.dist_err_agreed = false;
  struct RankTag {
    int prev;
    explicit RankTag(int r) : prev(tl_group_rank) { tl_group_rank = r; }
    ~RankTag() { tl_group_rank = prev; }
  } tag(c.group_rank);
  dist_preconditions(c, in);
  try {
    prove_dist_impl(c, in, com_out, ev_out);
  } catch (const KgsError& e) {
    if (e.code != KGS_E_NOT_WELL_CALC && e.code != KGS_E_NOT_DIVISIBLE && e.code != KGS_E_DOES_NOT_DIVIDE &&
        e.code != KGS_E_RANGE && !c.dist_err_agreed)
      c.group->abort();
    throw;
  } catch (...) {
    c.group->abort();
    throw;
  }
}

}  // namespace kgsi
