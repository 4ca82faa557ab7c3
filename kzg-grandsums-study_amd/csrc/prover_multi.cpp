// The multi-argument prover (include/kgs.h kgs_prove_multi): m arguments of any kinds over
// one domain share their challenges, ONE quotient and ONE pair of opening proofs.
//
// Per argument the rounds are prove_impl's (prover.cpp): the same round-1 polynomials, the same builder,
// the same quotient numerator N_j and linearisation r_j under the shared alpha, beta, gamma. The
// arguments meet in three places:
//  * Q = (sum_j delta^j N_j) / Z_H on one coset, by the fused kernel k_quotient_multi (poly.hip);
//  * W_xi opens r = sum_j delta^j r_j - Z_H(xi) Q and every round-1 polynomial at xi, one power of v each;
//  * W_xiw opens sum_j v^j S_j at xi w.
// For m = 1 no delta is drawn and every value is prove_impl's in exact-math mode: the proof is byte for
// byte the single-argument proof. Always exact-math (no reference behaviour exists to follow).
#include <hip/hip_runtime.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kgs.h"
#include "context.hpp"
#include "transcript.hpp"

using namespace kgs;
using namespace kgsi;
using host::Fr;

namespace {

struct MultiArg {
  int kind = 0, k = 0;
  std::vector<const uint32_t*> f_std, t_std;          // device, standard form
  const uint32_t *sel_f = nullptr, *sel_t = nullptr;  // device, Montgomery (nullptr: unselected)
  bool gs() const { return kind != KGS_GRANDPRODUCT; }
  bool lk() const { return kind == KGS_LOOKUP; }
  bool sel() const { return sel_f != nullptr; }
};

// device state of one argument between the rounds
struct ArgState {
  std::vector<uint32_t*> fm, tm, Fc, Tc;
  uint32_t *sFc = nullptr, *sTc = nullptr;
  const uint32_t *fcomb = nullptr, *tcomb = nullptr, *polF = nullptr, *polT = nullptr;
  uint32_t *cosS = nullptr, *cosF = nullptr, *cosT = nullptr, *cosSF = nullptr, *cosST = nullptr;
  uint32_t *Sev = nullptr, *Sc = nullptr;
  std::vector<Fr> fx, tx;
  Fr sFx = Fr::zero(), sTx = Fr::zero(), sxiw = Fr::zero();
};

std::string arg_prefix(int j) { return "argument " + std::to_string(j) + ": "; }

void prove_multi_impl(kgs_ctx& c, int nbits, const std::vector<MultiArg>& args, uint8_t* com_out, uint8_t* ev_out) {
  const int m = (int)args.size();
  c.xs.reset();
  ensure_twin(c);
  struct NttMode {
    bool prev;
    explicit NttMode(bool on) : prev(ntt_set_coresident(on)) {}
    ~NttMode() { ntt_set_coresident(prev); }
  } ntt_mode(c.msm_lanes < 2);
  using clk = std::chrono::steady_clock;
  auto t0 = clk::now();
  c.timing.assign(9, 0.0);
  Range range(ROUND_NAMES[0]);
  auto lap = [&](int r) {
    auto t1 = clk::now();
    c.timing[r] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    if (r + 1 < 5) range.push(ROUND_NAMES[r + 1]);
    else range.pop();
  };
  const uint64_t n = 1ull << nbits;
  const size_t E = 32 * n;
  if (c.srs_power < 0) throw KgsError(KGS_E_ARG, "no SRS loaded");
  if (c.srs_slice_world > 1)
    throw KgsError(KGS_E_ARG, "this context holds a rank's SRS slice: it proves only as that rank of a group (kgs_ctx_set_group)");
  if (c.srs_power < nbits)
    throw KgsError(KGS_E_SRS, "The Powers of Tau file is not sufficiently large to commit the polynomials.");
  if (nbits > c.nbits_max) throw KgsError(KGS_E_ARG, "nbits is outside the loaded SRS; reload with a larger nbits_max");

  bool any_vec = false, all_gp_unsel = true;
  int ncom_r1 = 0, nev_xi = 0;
  for (const MultiArg& a : args) {
    any_vec |= a.k > 1;
    all_gp_unsel &= !a.gs() && !a.sel();
    ncom_r1 += 2 * a.k + (a.sel() ? 2 : 0);
    nev_xi += (a.gs() ? 2 : 1) * a.k + (a.sel() ? 2 : 0);
  }
  const int ncom = ncom_r1 + m + 3;
  // pinned staging from the total commitment count: commit partials (c x 128 B each; Q and W_xi take two),
  // the Horner tile partials of every opened polynomial, flags and scalars
  c.msm_slots = ncom + 4;
  {
    const size_t ntl = (size_t)((n + EVAL_TILE - 1) / EVAL_TILE);
    const size_t need = (size_t)(ncom + 4) * ((size_t)c.tb.c * 128 + 64) + (32 * ntl + 64) * (size_t)(nev_xi + m + 2) +
                        64 * 16 + ((size_t)kgs_ctx::SCAL_BYTES * 2) + (1 << 20);
    c.ensure_pin(need > ((size_t)8 << 20) ? need : ((size_t)8 << 20));
  }
  c.reset_staging();
  // flag words: [j] builder of argument j, [16 + j] its divisibility check, [32], [33] the two divisions
  constexpr int FL_DIV = KGS_MAX_ARGS, FL_W = 2 * KGS_MAX_ARGS, FL_WORDS = 2 * KGS_MAX_ARGS + 16;
  uint32_t* flags = c.buf("mflags", 4 * FL_WORDS);
  HC(hipMemsetAsync(flags, 0, 4 * FL_WORDS, c.st));
  auto name = [](int j, const char* s, int i = -1) {
    return "m" + std::to_string(j) + "_" + s + (i >= 0 ? std::to_string(i) : std::string());
  };

  // ---------------- round 1: every argument's witness polynomials and commitments, argument by argument
  std::vector<ArgState> A(m);
  for (int j = 0; j < m; j++) {
    const MultiArg& a = args[j];
    ArgState& s = A[j];
    for (int i = 0; i < a.k; i++) {
      s.fm.push_back(c.buf(name(j, "fm", i), E));
      s.tm.push_back(c.buf(name(j, "tm", i), E));
      s.Fc.push_back(c.buf(name(j, "Fc", i), E));
      s.Tc.push_back(c.buf(name(j, "Tc", i), E));
      launch_to_mont(c.st, s.fm[i], a.f_std[i], n);
      launch_to_mont(c.st, s.tm[i], a.t_std[i], n);
      intt_nat(c, s.Fc[i], s.fm[i], nbits);
      intt_nat(c, s.Tc[i], s.tm[i], nbits);
    }
    if (a.sel()) {
      s.sFc = c.buf(name(j, "sFc"), E);
      s.sTc = c.buf(name(j, "sTc"), E);
      intt_nat(c, s.sFc, a.sel_f, nbits);
      intt_nat(c, s.sTc, a.sel_t, nbits);
    }
  }
  check_launch();
  std::vector<Commit> r1;
  int slot = 0;
  fork_lanes(c);
  for (int j = 0; j < m; j++) {
    for (int i = 0; i < args[j].k; i++) {
      r1.push_back(commit_launch(c, A[j].Fc[i], n, slot++, 0));
      r1.push_back(commit_launch(c, A[j].Tc[i], n, slot++, 1));
    }
    if (args[j].sel()) {
      r1.push_back(commit_launch(c, A[j].sFc, n, slot++, 0));
      r1.push_back(commit_launch(c, A[j].sTc, n, slot++, 1));
    }
  }
  c.sync();
  std::vector<std::vector<uint8_t>> com(ncom, std::vector<uint8_t>(64));
  int ci = 0;
  {
    std::vector<uint8_t*> outs;
    for (size_t i = 0; i < r1.size(); i++) outs.push_back(com[ci++].data());
    commits_finish(c, r1, outs);
  }
  lap(0);

  // ---------------- round 2: shared beta and gamma, every argument's S / Z
  host::Transcript tr;
  for (int i = 0; i < ci; i++) tr.add_commitment(com[i].data());
  Fr beta = Fr::zero();
  if (any_vec) {
    beta = tr.challenge();
    tr.add_scalar(beta);
  }
  const Fr gamma = tr.challenge();
  fork_lanes(c);
  hipStream_t s2 = c.msm_lanes >= 2 && c.st2 ? c.st2 : c.st;
  const int lcs = all_gp_unsel ? nbits : nbits + 1;
  const uint64_t cs = 1ull << lcs;
  const uint32_t ntiles = (uint32_t)((n + EVAL_TILE - 1) / EVAL_TILE);
  uint32_t* d_gamma = c.scal(&gamma, 1);
  uint32_t* bt_tp = c.buf("bt_tp", 32 * (ntiles + 1));
  uint32_t* bt_ti = c.buf("bt_ti", 32 * (ntiles + 1));
  std::vector<Commit> r2;
  for (int j = 0; j < m; j++) {
    const MultiArg& a = args[j];
    ArgState& s = A[j];
    s.fcomb = s.fm[0];
    s.tcomb = s.tm[0];
    s.polF = s.Fc[0];
    s.polT = s.Tc[0];
    if (a.k > 1) {
      uint32_t* b_fe = c.buf(name(j, "fcomb"), E);
      uint32_t* b_te = c.buf(name(j, "tcomb"), E);
      uint32_t* b_F = c.buf(name(j, "polF"), E);
      uint32_t* b_T = c.buf(name(j, "polT"), E);
      LcTerms l1, l2, l3, l4;
      Fr bp = Fr::one();
      for (int i = 0; i < a.k; i++) {
        l1.add(s.fm[i], n, bp);
        l2.add(s.tm[i], n, bp);
        l3.add(s.Fc[i], n, bp);
        l4.add(s.Tc[i], n, bp);
        bp = bp * beta;
      }
      run_lincomb(c.st, b_fe, n, l1);
      run_lincomb(c.st, b_te, n, l2);
      run_lincomb(s2, b_F, n, l3);
      run_lincomb(s2, b_T, n, l4);
      s.fcomb = b_fe;
      s.tcomb = b_te;
      s.polF = b_F;
      s.polT = b_T;
    }
    s.cosS = c.buf(name(j, "cosS"), 32 * cs);
    s.cosF = c.buf(name(j, "cosF"), 32 * cs);
    s.cosT = c.buf(name(j, "cosT"), 32 * cs);
    coset_fwd(c, s.cosF, s.polF, n, lcs, s2);
    coset_fwd(c, s.cosT, s.polT, n, lcs, s2);
    if (a.sel()) {
      s.cosSF = c.buf(name(j, "cosSF"), 32 * cs);
      s.cosST = c.buf(name(j, "cosST"), 32 * cs);
      coset_fwd(c, s.cosSF, s.sFc, n, lcs, s2);
      coset_fwd(c, s.cosST, s.sTc, n, lcs, s2);
    }
    s.Sev = c.buf(name(j, "Sev"), E);
    s.Sc = c.buf(name(j, "Sc"), E);
    launch_builder(c.st, !a.gs(), a.sel(), s.Sev, s.fcomb, s.tcomb, a.sel_f, a.sel_t, d_gamma, n, bt_tp, bt_ti, flags + j);
    intt_nat(c, s.Sc, s.Sev, nbits);
    check_launch();
    lane_join(c, c.st, s2);
    coset_fwd(c, s.cosS, s.Sc, n, lcs, s2);
    r2.push_back(commit_launch(c, s.Sc, n, slot++, j & 1));  // lane 1 follows the join: it sees Sc
  }
  uint32_t* nxm1 = get_nxm1(c, nbits, lcs);
  check_launch();
  uint32_t* h_flags = (uint32_t*)c.pin(4 * FL_WORDS);
  HC(hipMemcpyAsync(h_flags, flags, 4 * FL_WORDS, hipMemcpyDeviceToHost, c.st));
  c.sync();
  for (int j = 0; j < m; j++)
    if (h_flags[j])
      throw KgsError(KGS_E_NOT_WELL_CALC, arg_prefix(j) + (args[j].gs() ? "The grand-sum polynomial S is not well calculated"
                                                                        : "The grand-product polynomial Z is not well calculated"));
  const int iS = ci;
  {
    std::vector<uint8_t*> outs;
    for (int j = 0; j < m; j++) outs.push_back(com[ci++].data());
    commits_finish(c, r2, outs);
  }
  lap(1);

  // ---------------- round 3: alpha, the separator delta, one quotient
  tr.add_scalar(gamma);
  for (int j = 0; j < m; j++) tr.add_commitment(com[iS + j].data());
  const Fr alpha = tr.challenge();
  Fr delta = Fr::one();
  if (m > 1) {
    tr.add_scalar(alpha);
    delta = tr.challenge();
  }
  std::vector<Fr> dpow(m);
  dpow[0] = Fr::one();
  for (int j = 1; j < m; j++) dpow[j] = dpow[j - 1] * delta;
  const uint32_t rot = (uint32_t)(cs >> nbits);
  const uint64_t qlen = all_gp_unsel ? n - 1 : 2 * n - 2;
  const Fr gn = Fr::from_u64(5).pow_u64(n);
  const Fr inv_cs = Fr::from_u64(cs).inverse();
  // one set of prove_impl's quotient scalars per argument: slot 4 (the selT-binary weight) is the
  // argument's own, the rest is shared; the divisibility checks read them, the fused kernel set 0
  uint32_t* d_qs0 = nullptr;
  for (int j = 0; j < m; j++) {
    Fr qs[9] = {alpha, gamma, (gn - Fr::one()).inverse() * inv_cs, (gn.neg() - Fr::one()).inverse() * inv_cs,
                args[j].lk() ? Fr::zero() : alpha};
    fr29_record(alpha * qs[2], qs + 5);
    fr29_record(alpha * qs[3], qs + 7);
    uint32_t* d_qs = c.scal(qs, 9);
    if (j == 0) d_qs0 = d_qs;
    launch_divcheck(c.st, !args[j].gs(), args[j].sel(), flags + FL_DIV + j, A[j].Sev, A[j].fcomb, A[j].tcomb,
                    args[j].sel_f, args[j].sel_t, d_qs, n);
  }
  uint32_t* Qc = c.buf("mQc", 32 * cs);
  for (int j0 = 0; j0 < m; j0 += QM_MAX) {
    QuotMulti qm{};
    qm.nargs = m - j0 < QM_MAX ? m - j0 : QM_MAX;
    qm.accumulate = j0 > 0;
    for (int i = 0; i < qm.nargs; i++) {
      const int j = j0 + i;
      QuotArg& q = qm.a[i];
      q.S = A[j].cosS;
      q.F = A[j].cosF;
      q.T = A[j].cosT;
      q.SF = A[j].cosSF;
      q.ST = A[j].cosST;
      q.prod = !args[j].gs();
      q.sel = args[j].sel();
      q.lookup = args[j].lk();
      dpow[j].to_bytes((uint8_t*)q.delta);
      Fr rec[2];
      fr29_record(dpow[j], rec);
      memcpy(q.delta29, rec, 4 * LC_W29);
    }
    launch_quotient_multi(c.st, Qc, qm, nxm1, d_qs0, lcs, rot);
  }
  coset_inv_prescaled(c, Qc, Qc, lcs);
  check_launch();
  fork_lanes(c);
  Commit cQ = commit_launch_split(c, Qc, qlen, qlen / 2, slot);
  slot += 2;
  HC(hipMemcpyAsync(h_flags, flags, 4 * FL_WORDS, hipMemcpyDeviceToHost, c.st));
  c.sync();
  for (int j = 0; j < m; j++)
    if (h_flags[FL_DIV + j]) throw KgsError(KGS_E_NOT_DIVISIBLE, arg_prefix(j) + "Polynomial is not divisible");
  const int iQ = ci;
  commit_finish(c, cQ, com[ci++].data());
  lap(2);

  // ---------------- round 4: evaluations at xi, argument by argument, then every S_j at xi w
  tr.add_scalar(m > 1 ? delta : alpha);
  tr.add_commitment(com[iQ].data());
  const Fr xi = tr.challenge();
  const Fr xiw = xi * fr_w(nbits);
  std::vector<const uint32_t*> esrc, ssrc;
  std::vector<uint64_t> elen, slen;
  for (int j = 0; j < m; j++) {
    for (int i = 0; i < args[j].k; i++) {
      esrc.push_back(A[j].Fc[i]);
      if (args[j].gs()) esrc.push_back(A[j].Tc[i]);
    }
    if (args[j].sel()) {
      esrc.push_back(A[j].sFc);
      esrc.push_back(A[j].sTc);
    }
    ssrc.push_back(A[j].Sc);
  }
  elen.assign(esrc.size(), n);
  slen.assign(ssrc.size(), n);
  EvalJob ej1 = eval_launch(c, esrc, elen, xi, 0);
  EvalJob ej2 = eval_launch(c, ssrc, slen, xiw, 1);
  c.sync();
  const std::vector<Fr> ev1 = eval_finish(ej1), ev2 = eval_finish(ej2);
  std::vector<Fr> evals;  // proof order
  {
    size_t p = 0;
    for (int j = 0; j < m; j++) {
      ArgState& s = A[j];
      s.fx.assign(args[j].k, Fr::zero());
      s.tx.assign(args[j].k, Fr::zero());
      for (int i = 0; i < args[j].k; i++) {
        s.fx[i] = ev1[p++];
        if (args[j].gs()) s.tx[i] = ev1[p++];
      }
      if (args[j].sel()) {
        s.sFx = ev1[p++];
        s.sTx = ev1[p++];
      }
      s.sxiw = ev2[j];
    }
    evals = ev1;
    evals.insert(evals.end(), ev2.begin(), ev2.end());
  }
  lap(3);

  // ---------------- round 5: r = sum_j delta^j r_j - Z_H(xi) Q, the two openings
  tr.add_scalar(xi);
  for (const Fr& e : evals) tr.add_scalar(e);
  const Fr v = tr.challenge();
  LcTerms lw;
  Fr c0 = Fr::zero();
  Fr zh_neg = Fr::zero();
  for (int j = 0; j < m; j++) {
    // round5_terms at v = 0 is argument j's linearisation alone: its opening terms get coefficient zero,
    // c0 is r_j's constant and the S / polT coefficients are r_j's
    const R5 r5 = round5_terms(args[j].gs(), args[j].sel(), args[j].k, nbits, alpha, beta, gamma, Fr::zero(), xi, A[j].fx,
                               A[j].tx, A[j].sFx, A[j].sTx, A[j].sxiw, args[j].lk());
    for (const R5Term& t : r5.terms) {
      if (t.id == R5_S) lw.add(A[j].Sc, n, dpow[j] * t.coef);
      else if (t.id == R5_POLT) lw.add(A[j].polT, n, dpow[j] * t.coef);
      else if (t.id == R5_Q) zh_neg = t.coef;
    }
    c0 = c0 + dpow[j] * r5.c0;
  }
  lw.add(Qc, qlen, zh_neg);
  Fr vp = Fr::one();
  auto open = [&](const uint32_t* P, const Fr& at_xi) {
    vp = vp * v;
    lw.add(P, n, vp);
    c0 = c0 - vp * at_xi;
  };
  for (int j = 0; j < m; j++) {
    for (int i = 0; i < args[j].k; i++) open(A[j].Fc[i], A[j].fx[i]);
    if (args[j].gs())
      for (int i = 0; i < args[j].k; i++) open(A[j].Tc[i], A[j].tx[i]);
    if (args[j].sel()) {
      open(A[j].sFc, A[j].sFx);
      open(A[j].sTc, A[j].sTx);
    }
  }
  lw.c0 = c0;
  const uint64_t L = qlen > n ? qlen : n;
  uint32_t* Pbuf = c.buf("mPw", 32 * L);
  uint32_t* Wx = c.buf("mWxi", 32 * L);
  const uint32_t* xp1 = xpowers(c, xi);
  const uint32_t* xp2 = xpowers(c, xiw);
  fork_lanes(c);
  run_lincomb(c.st, Pbuf, L, lw);
  const uint32_t dtiles = (uint32_t)((L + EVAL_TILE - 1) / EVAL_TILE);
  launch_divide(c.st, Wx, flags + FL_W, Pbuf, L, xp1, c.buf("div_part", 32 * (dtiles + 1)),
                c.buf("div_carry", 32 * (dtiles + 1)));
  // W_{xi w} = sum_j v^j (S_j - S_j(xi w)) / (X - xi w)
  LcTerms l2;
  vp = Fr::one();
  for (int j = 0; j < m; j++) {
    l2.add(A[j].Sc, n, vp);
    l2.c0 = l2.c0 - vp * A[j].sxiw;
    vp = vp * v;
  }
  uint32_t* P2 = c.buf("mPw2", E);
  uint32_t* Wxw = c.buf("mWxiw", E);
  run_lincomb(s2, P2, n, l2);
  launch_divide(s2, Wxw, flags + FL_W + 1, P2, n, xp2, c.buf("div_part2", 32 * (ntiles + 1)),
                c.buf("div_carry2", 32 * (ntiles + 1)));
  check_launch();
  Commit cW2 = commit_launch(c, Wxw, n - 1, slot++, 1);
  lane_join(c, c.st, s2);
  Commit cW1 = commit_launch_split(c, Wx, L - 1, (L - 1 + n - 1) / 2, slot);
  slot += 2;
  HC(hipMemcpyAsync(h_flags, flags, 4 * FL_WORDS, hipMemcpyDeviceToHost, c.st));
  c.sync();
  if (h_flags[FL_W] || h_flags[FL_W + 1]) throw KgsError(KGS_E_DOES_NOT_DIVIDE, "Polynomial does not divide");
  commits_finish(c, {cW1, cW2}, {com[ci].data(), com[ci + 1].data()});
  ci += 2;
  lap(4);

  for (int i = 0; i < ncom; i++) memcpy(com_out + 64 * i, com[i].data(), 64);
  for (size_t i = 0; i < evals.size(); i++) evals[i].to_bytes(ev_out + 32 * i);
  c.reset_staging();
}

// the provers' error contract (prover.cpp DrainOnError): a call that leaves by an exception drains the
// context's streams first, so nothing of it still reads the caller's buffers
struct DrainOnError {
  kgs_ctx* ctx;
  int unwinding = std::uncaught_exceptions();
  explicit DrainOnError(kgs_ctx* c) : ctx(c) {}
  ~DrainOnError() {
    if (std::uncaught_exceptions() <= unwinding) return;
    hipSetDevice(ctx->device);
    for (hipStream_t s : {ctx->st, ctx->st2, ctx->st_copy, ctx->st_wb})
      if (s) (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
  }
};

// shape checks shared by the two entry points; `host`: the pointers are host memory, staged by plain copies
void prove_multi_entry(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* in, int count, uint8_t* com_out, uint8_t* ev_out,
                       bool host) {
  if (!ctx || !in || !com_out || !ev_out) throw KgsError(KGS_E_ARG, "NULL argument");
  if (count < 1 || count > KGS_MAX_ARGS)
    throw KgsError(KGS_E_ARG, "the number of arguments must be in 1 .. " + std::to_string(KGS_MAX_ARGS));
  if (nbits < 1 || nbits > 28) throw KgsError(KGS_E_ARG, "nbits must be in 1 .. 28");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (ctx->group)
    throw KgsError(KGS_E_ARG, "A multi-argument proof is not computed on a context attached to a rank group.");
  if (ctx->shard_world > 1)
    throw KgsError(KGS_E_ARG, "A multi-argument proof is not computed on a context with MSM sharding (kgs_ctx_set_shard).");
  size_t nvec = 0;
  for (int j = 0; j < count; j++) {
    const kgs_arg_t& a = in[j];
    if (a.kind != KGS_GRANDSUM && a.kind != KGS_GRANDPRODUCT && a.kind != KGS_LOOKUP)
      throw KgsError(KGS_E_ARG, arg_prefix(j) + "unknown argument kind");
    if (a.npols < 1) throw KgsError(KGS_E_ARG, arg_prefix(j) + "The number of multisets must be greater than 0.");
    if (a.npols > KGS_MAX_POLS) throw KgsError(KGS_E_ARG, arg_prefix(j) + "too many multisets");
    if (!a.evals_f || !a.evals_t) throw KgsError(KGS_E_ARG, arg_prefix(j) + "NULL argument");
    for (int i = 0; i < a.npols; i++)
      if (!a.evals_f[i] || !a.evals_t[i]) throw KgsError(KGS_E_ARG, arg_prefix(j) + "NULL argument");
    if ((a.sel_f == nullptr) != (a.sel_t == nullptr))
      throw KgsError(KGS_E_ARG, arg_prefix(j) + "selectors must be both given or both NULL");
    if (a.kind == KGS_LOOKUP && !a.sel_f)
      throw KgsError(KGS_E_ARG, arg_prefix(j) + "a lookup needs both selectors (sel_t holds the multiplicities)");
    nvec += 2 * (size_t)a.npols + (a.sel_f ? 2 : 0);
  }
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  const size_t E = (size_t)32 << nbits;
  uint32_t* stage = nullptr;
  if (host) {
    ctx->sync();
    stage = ctx->buf("multi_in", nvec * E);
  }
  size_t at = 0;
  auto take = [&](const void* p) -> const uint32_t* {
    if (!host) return (const uint32_t*)p;
    uint32_t* d = stage + (E / 4) * at++;
    HC(hipMemcpyAsync(d, p, E, hipMemcpyHostToDevice, ctx->st));
    return d;
  };
  std::vector<MultiArg> args(count);
  for (int j = 0; j < count; j++) {
    args[j].kind = in[j].kind;
    args[j].k = in[j].npols;
    for (int i = 0; i < in[j].npols; i++) {
      args[j].f_std.push_back(take(in[j].evals_f[i]));
      args[j].t_std.push_back(take(in[j].evals_t[i]));
    }
    if (in[j].sel_f) {
      args[j].sel_f = take(in[j].sel_f);
      args[j].sel_t = take(in[j].sel_t);
    }
  }
  prove_multi_impl(*ctx, nbits, args, com_out, ev_out);
}

}  // namespace

#define API_BEGIN try {
#define API_END                     \
  }                                 \
  catch (const KgsError& e) {       \
    return kgs_fail(e);             \
  }                                 \
  catch (const std::exception& e) { \
    kgs_errbuf() = e.what();        \
    return KGS_E_HIP;               \
  }                                 \
  return KGS_OK;

extern "C" {

int kgs_prove_multi(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* args, int count, uint8_t* commitments_out,
                    uint8_t* evaluations_out) {
  API_BEGIN
  prove_multi_entry(ctx, nbits, args, count, commitments_out, evaluations_out, true);
  API_END
}

int kgs_prove_multi_device(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* args, int count, uint8_t* commitments_out,
                           uint8_t* evaluations_out) {
  API_BEGIN
  prove_multi_entry(ctx, nbits, args, count, commitments_out, evaluations_out, false);
  API_END
}

}  // extern "C"
