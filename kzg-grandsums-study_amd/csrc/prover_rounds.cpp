// The five protocol rounds on one GPU, written once: m >= 1 arguments of any kinds over
// one domain share their challenges, ONE quotient and ONE pair of opening proofs. The single-argument
// prover (prover.cpp prove_impl) and the multi-argument prover (prover_multi.cpp) are its two callers;
// RoundOpts says what is special about each.
//
// Per argument: the round-1 polynomials, the builder, the quotient numerator N_j and the linearisation
// r_j under the shared alpha, beta, gamma. The arguments meet in three places:
//  * Q = (sum_j delta^j N_j) / Z_H on one coset: k_quotient for one argument, the fused
//    k_quotient_multi (poly.hip) in groups of QM_MAX for more;
//  * W_xi opens r = sum_j delta^j r_j - Z_H(xi) Q and every round-1 polynomial at xi, one power of v each;
//  * W_xiw opens sum_j v^j S_j at xi w.
// For m = 1 no delta is drawn and the proof is the reference's (prover.js) byte for byte.
//
// The order of the work on each stream is part of the behaviour: it was measured into place with several
// contexts in flight. Where one argument and many, or the two callers, differ, the choice is made at one
// visible place.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kgs.h"
#include "context.hpp"
#include "transcript.hpp"

namespace kgsi {

std::string arg_prefix(int j) { return "argument " + std::to_string(j) + ": "; }

void check_srs(const kgs_ctx& c, int nbits) {
  if (c.srs_power < 0) throw KgsError(KGS_E_ARG, "no SRS loaded");
  if (c.srs_slice_world > 1)
    throw KgsError(KGS_E_ARG, "this context holds a rank's SRS slice: it proves only as that rank of a group (kgs_ctx_set_group)");
  if (c.srs_power < nbits)
    throw KgsError(KGS_E_SRS, "The Powers of Tau file is not sufficiently large to commit the polynomials.");
}

namespace {

// device state of one argument between the rounds
struct ArgState : ArgPolys {
  std::vector<uint32_t*> fm, tm;
  const uint32_t *fcomb = nullptr, *tcomb = nullptr, *polF = nullptr;
  uint32_t *cosS = nullptr, *cosF = nullptr, *cosT = nullptr, *cosSF = nullptr, *cosST = nullptr;
  uint32_t* Sev = nullptr;
  XiEvals x;
  Fr sxiw = Fr::zero();
};

// Montgomery write-back (prover.js:147-148): a vector's D2H on the write-back stream right after its
// conversion on `st` (not after the round's MSMs, and never queued between input DMAs)
void write_back(kgs_ctx& c, int& nwb, uint8_t* dst, const uint32_t* src, size_t E, hipStream_t st) {
  if (!dst) return;
  if (!c.st_wb) c.st_wb = copy_stream();
  if ((int)c.ev_wb.size() <= nwb) {
    hipEvent_t e;
    HC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c.ev_wb.push_back(e);
  }
  HC(hipEventRecord(c.ev_wb[nwb], st));
  HC(hipStreamWaitEvent(c.st_wb, c.ev_wb[nwb], 0));
  nwb++;
  // hipMemcpyAsync. Into pinned memory the runtime runs it as its copyBuffer shader kernel, not on an
  // SDMA engine: ~0.8 ms of CU residency per 32 MiB in flight; hipMemcpyDtoHAsync does the same
  // (profiles/r06/host_engine/, wb_api/). KGS_WB_COPY=kernel stores from our own shader into the
  // mapped pinned buffer instead (poly.hip k_host_store): measured slower in flight, 83-85 vs 86-88
  // proofs/s (profiles/r05/wb_ab.txt), kept for A/B
  static const unsigned wb_blocks = [] {
    const char* e = getenv("KGS_WB_COPY");
    if (!(e && !strcmp(e, "kernel"))) return 0u;
    const char* b = getenv("KGS_WB_BLOCKS");
    return b ? (unsigned)atoi(b) : 64u;
  }();
  void* mapped = nullptr;
  if (wb_blocks && hipHostGetDevicePointer(&mapped, dst, 0) != hipSuccess) {
    (void)hipGetLastError();
    mapped = nullptr;
  }
  if (mapped && E % 16 == 0) launch_host_store(c.st_wb, mapped, src, E, wb_blocks);
  else HC(hipMemcpyAsync(dst, src, E, hipMemcpyDeviceToHost, c.st_wb));
}

}  // namespace

void prove_rounds(kgs_ctx& c, int nbits, const std::vector<ArgIn>& args, const RoundOpts& o, uint8_t* com_out,
                  uint8_t* ev_out) {
  const int m = (int)args.size();
  if (o.ref_quirks && m != 1) throw KgsError(KGS_E_ARG, "reference-quirks mode proves one argument");
  NttMode ntt_mode(c.msm_lanes < 2);
  // every slot, the host-boundary ones [6..8] too: kgs_prove writes them after this returns, and a
  // device-resident proof must not report a previous host call's copy and prover times
  c.timing.assign(9, 0.0);
  RoundClock clock(c);
  const uint64_t n = 1ull << nbits;
  const size_t E = 32 * n;
  static const HostHooks no_hooks;
  const HostHooks& hk = o.hooks ? *o.hooks : no_hooks;

  bool any_vec = false, all_gp_unsel = true;
  int ncom_r1 = 0, nev_xi = 0;
  for (const ArgIn& a : args) {
    any_vec |= a.k > 1;
    all_gp_unsel &= !a.gs() && !a.sel();
    ncom_r1 += a.ncom_r1();
    nev_xi += a.nev_xi();
  }
  const int ncom = ncom_r1 + m + 3;
  // Pinned staging for this proof's host round trips, from what it allocates there: commit partials
  // (c x 128 B each; Q, W_xi and a replayed Q take two), the Horner tile partials (32 B per EVAL_TILE
  // coefficients) of every polynomial opened at xi, of every S_j and of the reference replay's second
  // look at F, flags and scalars; each bump allocation rounds up to 64 B. On paper, at m = 1: the
  // commitment term is the single-argument prover's earlier formula exactly, and the evaluation term
  // counts nev_xi + 3 polynomials where that formula had a flat 2k + 3. So it is never smaller for a
  // grand-sum or a lookup (2k + 3 or 2k + 5), and for a grand-product it lacks the k T_i, which are
  // never evaluated (k + 3, or k + 5 selected): those partials were never allocated. Either formula
  // stays under the 8 MiB floor up to k of several hundred at 2^20.
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
  uint32_t* flags = c.buf("flags", 4 * FL_WORDS);
  HC(hipMemsetAsync(flags, 0, 4 * FL_WORDS, c.st));
  auto name = [](int j, const char* s, int i = -1) {
    return "a" + std::to_string(j) + "_" + s + (i >= 0 ? std::to_string(i) : std::string());
  };

  // ---------------- round 1: witness polynomials + commitments (prover.js:144-179), argument by argument
  std::vector<ArgState> A(m);
  for (int j = 0; j < m; j++) {
    for (int i = 0; i < args[j].k; i++) {
      A[j].fm.push_back(c.buf(name(j, "fm", i), E));
      A[j].tm.push_back(c.buf(name(j, "tm", i), E));
      A[j].Fc.push_back(c.buf(name(j, "Fc", i), E));
      A[j].Tc.push_back(c.buf(name(j, "Tc", i), E));
    }
    if (args[j].sel()) {
      A[j].sFc = c.buf(name(j, "sFc"), E);
      A[j].sTc = c.buf(name(j, "sTc"), E);
    }
  }
  // Host-buffer inputs (kgs_prove) arrive vector by vector: input_issued(v) returns once vector v's DMA
  // is enqueued (its host copy may still be running on another thread before that), and ready[v] is the
  // event its first kernel waits for.
  size_t nin = 0;
  auto wait_input = [&](hipStream_t st) {
    const size_t v = nin++;
    if (hk.input_issued) hk.input_issued(v);
    if (v < hk.ready.size() && hk.ready[v]) HC(hipStreamWaitEvent(st, hk.ready[v], 0));
  };
  int nwb = 0, nmont = 0;
  auto mont_out = [&](const std::vector<uint8_t*>& v) -> uint8_t* { return v.empty() ? nullptr : v[nmont]; };
  std::vector<Commit> r1;
  int slot = 0;
  // Piped (two MSM lanes, a proof alone on its context: the latency mode): each input vector's whole
  // round-1 chain — Montgomery conversion, iNTT, commitment MSM — runs on the lane of its commitment,
  // F_i / selF on lane 0 and T_i / selT on lane 1, so that T's transfer (host buffers) and T's transform
  // overlap F's MSM instead of delaying it. Unpiped: every conversion and transform on the main stream,
  // then the commitments alternate between the lanes.
  const bool piped = o.piped_round1;
  hipStream_t lane1 = c.st;
  if (piped) {
    fork_lanes(c);
    lane1 = c.st2;
  }
  for (int j = 0; j < m; j++) {
    const ArgIn& a = args[j];
    ArgState& s = A[j];
    for (int i = 0; i < a.k; i++, nmont++) {
      wait_input(c.st);
      launch_to_mont(c.st, s.fm[i], a.f_std[i], n);
      write_back(c, nwb, mont_out(hk.mont_f_out), s.fm[i], E, c.st);
      if (piped) {
        intt_nat(c, s.Fc[i], s.fm[i], nbits);
        r1.push_back(commit_launch(c, s.Fc[i], n, slot++, 0));
      }
      wait_input(lane1);
      launch_to_mont(lane1, s.tm[i], a.t_std[i], n);
      write_back(c, nwb, mont_out(hk.mont_t_out), s.tm[i], E, lane1);
      if (!piped) intt_nat(c, s.Fc[i], s.fm[i], nbits);
      intt_nat(c, s.Tc[i], s.tm[i], nbits, lane1);
      if (piped) r1.push_back(commit_launch(c, s.Tc[i], n, slot++, 1));
    }
    // fm/tm are not written again before the round-1 sync (the write-back reads them on st_wb)
    if (a.sel()) {
      wait_input(c.st);
      intt_nat(c, s.sFc, a.sel_f, nbits);
      if (piped) r1.push_back(commit_launch(c, s.sFc, n, slot++, 0));
      wait_input(lane1);
      intt_nat(c, s.sTc, a.sel_t, nbits, lane1);
      if (piped) r1.push_back(commit_launch(c, s.sTc, n, slot++, 1));
    }
  }
  check_launch();
  if (!piped) {
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
  }
  // round 1's commitments only: the Montgomery write-back on st_wb keeps running under rounds 2-5
  // (after_round1's thread waits for it before copying to the caller)
  HC(hipStreamSynchronize(c.st));
  if (c.st2) HC(hipStreamSynchronize(c.st2));
  if (hk.after_round1) hk.after_round1();
  std::vector<uint8_t> com(64 * (size_t)ncom);  // proof order
  int ci = 0;
  auto com_at = [&](int i) { return com.data() + 64 * (size_t)i; };
  {
    std::vector<uint8_t*> outs;
    for (size_t i = 0; i < r1.size(); i++) outs.push_back(com_at(ci++));
    commits_finish(c, r1, outs);
  }
  clock.lap(0);

  // ---------------- round 2: shared beta and gamma, every argument's S / Z (prover.js:181-231)
  host::Schedule sched;
  const host::Schedule::BetaGamma bg = sched.after_round1(com_at(0), ci, any_vec);
  const Fr &beta = bg.beta, &gamma = bg.gamma;
  // Two lanes (latency mode): the challenge-independent coset evaluations of F, T (+ selectors) run on
  // lane 1 from the start of the round, beside the builder's serial part (k_tile_inverse is one
  // workgroup) and S's inverse NTT on lane 0; S's commitment follows (S_j's on lane j & 1), S's coset
  // evaluation on lane 1 once S exists. One lane: the same work in order on the main stream.
  fork_lanes(c);
  hipStream_t s2 = c.msm_lanes >= 2 && c.st2 ? c.st2 : c.st;
  const int lcs = all_gp_unsel ? nbits : nbits + 1;
  const uint64_t cs = 1ull << lcs;
  const uint32_t ntiles = (uint32_t)((n + EVAL_TILE - 1) / EVAL_TILE);
  uint32_t* d_gamma = c.scal(&gamma, 1);
  // one builder scratch pair for all arguments
  uint32_t* bt_tp = c.buf("bt_tp", 32 * (ntiles + 1));
  uint32_t* bt_ti = c.buf("bt_ti", 32 * (ntiles + 1));
  std::vector<Commit> r2;
  for (int j = 0; j < m; j++) {
    const ArgIn& a = args[j];
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
      const BetaComb bc = beta_combination(s.fm, s.tm, s.Fc, s.Tc, a.k, beta, n);
      run_lincomb(c.st, b_fe, n, bc.fcomb);
      run_lincomb(c.st, b_te, n, bc.tcomb);
      run_lincomb(s2, b_F, n, bc.polF);
      run_lincomb(s2, b_T, n, bc.polT);
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
  get_nxm1(c, nbits, lcs);  // built (first proof of this shape) under round 2's MSMs; run_quotient finds it cached
  check_launch();
  uint32_t* h_flags = (uint32_t*)c.pin(4 * FL_WORDS);
  HC(hipMemcpyAsync(h_flags, flags, 4 * FL_WORDS, hipMemcpyDeviceToHost, c.st));
  c.sync();
  auto prefix = [&](int j) { return o.name_arguments ? arg_prefix(j) : std::string(); };
  for (int j = 0; j < m; j++)
    if (h_flags[j])
      throw KgsError(KGS_E_NOT_WELL_CALC, prefix(j) + (args[j].gs() ? "The grand-sum polynomial S is not well calculated"
                                                                     : "The grand-product polynomial Z is not well calculated"));
  const int iS = ci;
  {
    std::vector<uint8_t*> outs;
    for (int j = 0; j < m; j++) outs.push_back(com_at(ci++));
    commits_finish(c, r2, outs);
  }
  clock.lap(1);

  // ---------------- round 3: alpha, the separator delta, one quotient on a coset (prover.js:233-286)
  const host::Schedule::AlphaDelta ad = sched.after_round2(com_at(iS), m);
  const Fr &alpha = ad.alpha, &delta = ad.delta;
  std::vector<Fr> dpow(m);
  dpow[0] = Fr::one();
  for (int j = 1; j < m; j++) dpow[j] = dpow[j - 1] * delta;
  uint64_t qlen = all_gp_unsel ? n - 1 : 2 * n - 2;  // deg Q + 1 bound
  // every argument's divisibility check on H, then the one quotient on the coset (run_divcheck and
  // run_quotient, prover.cpp: the scalar sets and the choice of kernel): k_quotient for the single proof,
  // the fused kernel for several arguments
  std::vector<QuotIn> qin(m);
  const uint32_t* d_qs0 = nullptr;
  for (int j = 0; j < m; j++) {
    const QuotIn on_h{args[j].kind, A[j].Sev, A[j].fcomb, A[j].tcomb, args[j].sel_f, args[j].sel_t};
    const uint32_t* d_qs = run_divcheck(c, nbits, lcs, on_h, alpha, gamma, n, flags + FL_DIV + j);
    if (j == 0) d_qs0 = d_qs;
    qin[j] = QuotIn{args[j].kind, A[j].cosS, A[j].cosF, A[j].cosT, A[j].cosSF, A[j].cosST};
  }
  const uint32_t* Qc = c.buf("Qc", 32 * cs);
  run_quotient(c, nbits, lcs, qin, alpha, gamma, dpow, (uint32_t*)Qc, m > 1, d_qs0);
  coset_inv_prescaled(c, (uint32_t*)Qc, Qc, lcs);
  check_launch();
  // latency mode: Q's 2n points over both MSM lanes (one lane's sort and tail overlap the other's
  // accumulation)
  fork_lanes(c);
  Commit cQ = commit_launch_split(c, Qc, qlen, qlen / 2, slot);
  slot += 2;
  std::vector<const uint32_t*> qops;
  const uint32_t* probe = nullptr;
  if (o.ref_quirks) {
    qops = {A[0].polF, A[0].polT, A[0].Sc};
    if (args[0].sel()) {
      qops.push_back(A[0].sFc);
      qops.push_back(A[0].sTc);
    }
    probe = ref_quirks_probe(c, n, qops, Qc, qlen);
  }
  HC(hipMemcpyAsync(h_flags, flags, 4 * FL_WORDS, hipMemcpyDeviceToHost, c.st));
  c.sync();
  // Reference-quirks mode (ref_quirks.cpp): where the reference's own quotient chain does not compute
  // the quotient (an operand of degree 1 <= d < n/2) it is replayed with the reference's buffer
  // semantics and its Q replaces ours; otherwise the only difference is the reference's RangeError
  // on a zero quotient (divZh, after its divisibility check).
  const uint32_t* Fmut = nullptr;  // polF's buffer after the replay wrote into it (Q2), else nullptr
  bool replayed = false;
  if (probe && ref_quirks_needed(probe, qops.size(), n)) {
    uint32_t* fm_out = nullptr;
    Qc = ref_quirks_quotient(c, args[0].gs(), args[0].sel(), args[0].lk(), nbits, alpha, gamma, A[0].polF, A[0].polT,
                             A[0].Sc, A[0].sFc, A[0].sTc, qlen, fm_out);
    Fmut = fm_out;
    replayed = true;
    // multiExponentiation reads degree()+1 points of the reference's 2n-point PTau buffer
    // (prover.js:83-84, polynomial.js:1106-1110); past it, ffjavascript's multiExpAffine gets fewer
    // bases than scalars, which is not reproduced
    if (qlen > 2 * n)
      throw KgsError(KGS_E_ARG, "reference-quirks mode: the reference's Q has more coefficients than its 2n-point SRS buffer");
    cQ = commit_launch_split(c, Qc, qlen, qlen / 2, slot);
    slot += 2;
    c.sync();
  }
  if (!replayed) {
    for (int j = 0; j < m; j++)
      if (h_flags[FL_DIV + j]) throw KgsError(KGS_E_NOT_DIVISIBLE, prefix(j) + "Polynomial is not divisible");
    if (probe && ref_quotient_is_zero(probe)) throw KgsError(KGS_E_RANGE, "offset is out of bounds");
  }
  const int iQ = ci;
  commit_finish(c, cQ, com_at(ci++));
  clock.lap(2);

  // ---------------- round 4: evaluations at xi, argument by argument, then every S_j at xi w (prover.js:288-318)
  const Fr xi = sched.after_round3(com_at(iQ));
  const Fr xiw = xi * fr_w(nbits);
  // reference-quirks mode, polF's buffer shared and rewritten (Q2): the reference's later reads of polF
  // see the new values — polFs[0] itself for one multiset, only polF.evaluate (prover.js:360) for vectors
  const bool fxi_set = Fmut && args[0].k > 1;
  if (Fmut && !fxi_set) A[0].Fc[0] = (uint32_t*)Fmut;
  std::vector<const uint32_t*> esrc, ssrc;
  for (int j = 0; j < m; j++) {
    args[j].each_xi(false, [&](R5Poly id, int i) { esrc.push_back(A[j].poly(id, i)); });
    ssrc.push_back(A[j].Sc);
  }
  if (fxi_set) esrc.push_back(Fmut);
  EvalJob ej1 = eval_launch(c, esrc, std::vector<uint64_t>(esrc.size(), n), xi, 0);
  EvalJob ej2 = eval_launch(c, ssrc, std::vector<uint64_t>(ssrc.size(), n), xiw, 1);
  c.sync();
  const std::vector<Fr> ev1 = eval_finish(ej1), ev2 = eval_finish(ej2);
  const Fr* at = ev1.data();
  for (int j = 0; j < m; j++) {
    at = A[j].x.unpack(args[j], at);
    A[j].sxiw = ev2[j];
  }
  const Fr fxi_mut = fxi_set ? *at : Fr::zero();
  std::vector<Fr> evals(ev1.data(), at);  // proof order
  evals.insert(evals.end(), ev2.begin(), ev2.end());
  clock.lap(3);

  // ---------------- round 5: r = sum_j delta^j r_j - Z_H(xi) Q, the two openings (prover.js:320-413)
  const Fr v = sched.after_round4(evals.data(), evals.size());
  std::vector<OpenArg> open;
  for (int j = 0; j < m; j++) open.push_back({&args[j], &A[j], &A[j].x, A[j].sxiw});
  const LcTerms lw = wxi_numerator(open, nbits, alpha, beta, gamma, dpow, xi, v, Qc, n, qlen, fxi_set ? &fxi_mut : nullptr);
  const uint64_t L = qlen > n ? qlen : n;
  uint32_t* Pbuf = c.buf("Pw", 32 * L);
  uint32_t* Wx = c.buf("Wxi", 32 * L);
  const uint32_t* xp1 = xpowers(c, xi);
  const uint32_t* xp2 = xpowers(c, xiw);
  // two lanes: W_x's linear combination and division on lane 0 while W_xw's run on lane 1 (and its
  // commitment starts there right after); the commitments balance as W_x[0, h) on lane 0 and W_xw +
  // W_x[h, L - 1) on lane 1, h = half of all their points
  fork_lanes(c);
  run_lincomb(c.st, Pbuf, L, lw);
  const uint32_t dtiles = (uint32_t)((L + EVAL_TILE - 1) / EVAL_TILE);
  launch_divide(c.st, Wx, flags + FL_W, Pbuf, L, xp1, c.buf("div_part", 32 * (dtiles + 1)),
                c.buf("div_carry", 32 * (dtiles + 1)));
  // W_{xi w} = sum_j v^j (S_j - S_j(xi w)) / (X - xi w)
  LcTerms l2;
  Fr vp = Fr::one();
  for (int j = 0; j < m; j++) {
    l2.add(A[j].Sc, n, vp);
    l2.c0 = l2.c0 - vp * A[j].sxiw;
    vp = vp * v;
  }
  uint32_t* P2 = c.buf("Pw2", E);
  uint32_t* Wxw = c.buf("Wxiw", E);
  run_lincomb(s2, P2, n, l2);
  launch_divide(s2, Wxw, flags + FL_W + 1, P2, n, xp2, c.buf("div_part2", 32 * (ntiles + 1)),
                c.buf("div_carry2", 32 * (ntiles + 1)));
  check_launch();
  Commit cW2 = commit_launch(c, Wxw, n - 1, slot++, 1);
  lane_join(c, c.st, s2);  // W_x[h, L - 1) on lane 1 needs W_x
  Commit cW1 = commit_launch_split(c, Wx, L - 1, (L - 1 + n - 1) / 2, slot);
  slot += 2;
  HC(hipMemcpyAsync(h_flags, flags, 4 * FL_WORDS, hipMemcpyDeviceToHost, c.st));
  c.sync();
  if (h_flags[FL_W] || h_flags[FL_W + 1]) throw KgsError(KGS_E_DOES_NOT_DIVIDE, "Polynomial does not divide");
  commits_finish(c, {cW1, cW2}, {com_at(ci), com_at(ci + 1)});
  ci += 2;
  clock.lap(4);

  memcpy(com_out, com.data(), com.size());
  for (size_t i = 0; i < evals.size(); i++) evals[i].to_bytes(ev_out + 32 * i);
  c.reset_staging();
}

}  // namespace kgsi
