// Host orchestration of the MI355X-native grand-sum / grand-product KZG prover. One context = one
// device, one HIP stream, a device-resident SRS with its MSM window tables, NTT/coset tables, and a
// grow-only device buffer pool. Here: device allocation and the registries of the shared tables; the
// domain tables; the NTT, Horner, linear-combination and quotient helpers the round engine
// (prover_rounds.cpp) calls; round 5's terms; the single-argument prover (prove_impl); and the context's
// entry points of the C-ABI (include/kgs.h): create, destroy, setters, kgs_ctx_idle, kgs_last_timing,
// kgs_prove_device. kgs_prove is in host_boundary.cpp, the building blocks one by one in primitives.cpp.
//
// Round structure, transcript order and proof schema follow the reference provers exactly
// (src/grandsum/mset_eq_kzg_prover.js:12-434, src/grandproduct/mset_eq_kzg_prover.js:12-414).
// Every output is a unique field / group element, so the computation is re-planned for the GPU
// where that leaves the values unchanged (DESIGN.md §Hot path):
//  * evalsF = fft(sum beta^i F_i) = sum beta^i f_i (NTT linearity; prover.js:207-217)
//  * the quotient Q = N / Z_H is computed on a coset of size 2n (n for the unselected grand
//    product) instead of the 2n/4n `multiply` chain + `divZh` (prover.js:233-286); divisibility
//    (the "Polynomial is not divisible" check of divZh) is decided exactly by N(w^i) == 0 on H;
//  * S(wX) on the coset is a rotation of the coset evaluations (no shiftOmega NTT pair);
//  * L1(X)/Z_H(X) = 1/(n (X - 1)) on the coset (precomputed per domain);
//  * commitments skip zero top coefficients by degree bounds (zero scalars add nothing).
#include "context.hpp"

using namespace kgs;
using namespace kgsi;
using host::Fq;
using host::Fr;

namespace kgsi {

// Every device allocation goes through here. KGS_DEBUG_ALLOC_LIMIT=<bytes> (fault injection for the
// tests) makes any single request above that size fail as out-of-memory; with KGS_DEBUG_ALLOC_RANK=<r>
// only on the host thread that is proving as rank r of a rank group (a failure on ONE rank of an
// in-process group, whose ranks are threads of one process).
thread_local int tl_group_rank = -1;
hipError_t dev_malloc(void** p, size_t bytes) {
  if (const char* e = getenv("KGS_DEBUG_ALLOC_LIMIT")) {
    const unsigned long long lim = strtoull(e, nullptr, 10);
    const char* rk = getenv("KGS_DEBUG_ALLOC_RANK");
    if (lim && bytes > lim && (!rk || atoi(rk) == tl_group_rank)) {
      *p = nullptr;
      return hipErrorOutOfMemory;
    }
  }
  return hipMalloc(p, bytes);
}

std::mutex g_reg_mu;
std::vector<std::weak_ptr<SrsTables>> g_srs_reg;
std::vector<std::weak_ptr<DomainTables>> g_dom_reg;

// ------------------------------------------------------------------ domain tables
// The 29-bit twin of every table (stage twiddles, coset powers, 1/m), record i <-> element i, for the
// LDS passes' products (fr29.hpp): 40 B per element beside the 32 B words. Built with the domain for
// the proofs' own domains; a domain grown only for the reference-quirks replay (up to 2^26 points)
// gets none (its NTTs take the 8 x 32 products, the same values), and the first proof that runs on it
// builds the twin then (ensure_twin). Under g_reg_mu.
static void build_twin(kgs_ctx& c, DomainTables* d) {
  if (d->mem29) return;
  const uint64_t entries = 4 * (1ull << d->logM) + d->logM + 1;
  HC(dev_malloc((void**)&d->mem29, (size_t)4 * TW29_WORDS * entries));
  launch_tw29(c.st, d->mem29, d->mem, entries);
  check_launch();
  HC(hipStreamSynchronize(c.st));
  ntt_register_tw29(d->mem, entries, d->mem29);
}
void ensure_twin(kgs_ctx& c) {
  if (!c.dom) return;
  std::lock_guard<std::mutex> lk(g_reg_mu);  // mem29 is written under this lock (by any context)
  build_twin(c, c.dom.get());
}

// Shared per device: a context asking for 2^logM reuses any published table of at least that size.
void ensure_domain(kgs_ctx& c, int logM, bool twin) {
  if (c.logM >= logM) return;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (auto& w : g_dom_reg) {
    auto d = w.lock();
    if (d && d->device == c.device && d->logM >= logM) {
      if (twin) build_twin(c, d.get());
      // switching may drop the last reference to the old tables (freed at once): nothing of this
      // context may still read them. Every caller drains its streams first today; this keeps it so.
      c.sync();
      c.use_domain(d);
      c.nxm1.clear();
      return;
    }
  }
  const uint64_t M = 1ull << logM;
  auto d = std::make_shared<DomainTables>();
  d->device = c.device;
  // stage twiddle tables: tw[h + t] = w_{2h}^t for h = 2^l, l < logM (entries 1..M-1); coset powers
  // g^i, g^-i (g = KGS_NTT_COSET_GEN); 1/2^l for l <= logM
  const size_t words = (size_t)8 * (4 * M + logM + 1);
  HC(dev_malloc((void**)&d->mem, 4 * words));
  d->tw_fwd = d->mem;
  d->tw_inv = d->tw_fwd + 8 * M;
  d->coset_pow = d->tw_inv + 8 * M;
  d->coset_ipow = d->coset_pow + 8 * M;
  d->invm = d->coset_ipow + 8 * M;
  // This may run in the middle of a proof (the reference-quirks replay grows the domain,
  // ref_quirks.cpp need_domain): the scalars and pinned words the proof has staged so far must stay
  // intact, so the build stages above them and gives that space back once it has completed.
  c.sync();
  const size_t pin_mark = c.h_pin_off, scal_mark = c.d_scal_off;
  std::vector<Fr> consts;
  for (int l = 0; l < logM; l++) {
    Fr w = fr_w(l + 1);
    consts.push_back(w);
    consts.push_back(w.inverse());
  }
  Fr g = Fr::from_u64(KGS_NTT_COSET_GEN);
  consts.push_back(g);
  consts.push_back(g.inverse());
  uint32_t* dc = c.scal(consts.data(), (int)consts.size());
  for (int l = 0; l < logM; l++) {
    const uint64_t h = 1ull << l;
    launch_powers(c.st, d->tw_fwd + 8 * h, h, dc + 16 * l, nullptr);
    launch_powers(c.st, d->tw_inv + 8 * h, h, dc + 16 * l + 8, nullptr);
  }
  launch_powers(c.st, d->coset_pow, M, dc + 16 * logM, nullptr);
  launch_powers(c.st, d->coset_ipow, M, dc + 16 * logM + 8, nullptr);
  std::vector<Fr> im(logM + 1);
  for (int l = 0; l <= logM; l++) im[l] = Fr::from_u64(1ull << l).inverse();
  uint8_t* h = c.pin(32 * (logM + 1));
  for (int l = 0; l <= logM; l++) im[l].to_bytes(h + 32 * l);
  HC(hipMemcpyAsync(d->invm, h, 32 * (logM + 1), hipMemcpyHostToDevice, c.st));
  check_launch();
  c.sync();  // built
  c.h_pin_off = pin_mark;
  c.d_scal_off = scal_mark;
  d->logM = logM;
  if (twin) build_twin(c, d.get());  // then publish
  g_dom_reg.erase(std::remove_if(g_dom_reg.begin(), g_dom_reg.end(), [](auto& w) { return w.expired(); }),
                  g_dom_reg.end());
  g_dom_reg.push_back(d);
  c.use_domain(d);
  c.nxm1.clear();
}

uint32_t* get_nxm1(kgs_ctx& c, int nbits, int lcs) {
  auto key = std::make_pair(nbits, lcs);
  auto it = c.nxm1.find(key);
  if (it != c.nxm1.end()) return it->second;
  const uint64_t cs = 1ull << lcs;
  uint32_t* out = c.buf("nxm1_" + std::to_string(nbits) + "_" + std::to_string(lcs), 32 * cs);
  uint32_t* tmp = c.buf("nxm1_tmp", 32 * cs);
  // 1/(n (x - 1)) / cs: the coset inverse NTT of the quotient (coset_inv_prescaled) takes its 1/cs from here and
  // from the Z_H scalars of round 3 instead of a product per element
  Fr consts[2] = {Fr::from_u64(KGS_NTT_COSET_GEN), Fr::from_u64(1ull << nbits) * Fr::from_u64(cs)};
  uint32_t* d = c.scal(consts, 2);
  // w_M^j (j < M/2) is the last stage table, tw_fwd + 8 * (M/2)
  const uint64_t halfM = (1ull << c.logM) / 2;
  launch_nxm1(c.st, tmp, c.tw_fwd + 8 * halfM, halfM, d, d + 8, lcs, (1ull << c.logM) >> lcs);
  launch_fr_batch_inv(c.st, out, tmp, cs);
  check_launch();
  c.nxm1[key] = out;
  return out;
}

// ------------------------------------------------------------------ NTT helpers
// natural-order evaluations -> natural-order coefficients (out != in)
void intt_nat(kgs_ctx& c, uint32_t* out, const uint32_t* in, int logm, hipStream_t st) {
  ntt_dit(st ? st : c.st, out, in, 0, logm, c.tw_inv, c.logM, nullptr, c.invm + 8 * logm);
}
// coefficients (len <= 2^lcs, natural) -> coset evaluations p(g w^i), bit-reversed order
void coset_fwd(kgs_ctx& c, uint32_t* out, const uint32_t* in, uint64_t len, int lcs, hipStream_t st) {
  ntt_dif(st ? st : c.st, out, in, len, lcs, c.coset_pow, c.tw_fwd, c.logM);
}
// bit-reversed coset evaluations, already scaled by 1/cs -> natural coefficients (in place allowed)
void coset_inv_prescaled(kgs_ctx& c, uint32_t* out, const uint32_t* in, int lcs) {
  ntt_dit(c.st, out, in, 1, lcs, c.tw_inv, c.logM, c.coset_ipow, nullptr);
}

// ------------------------------------------------------------------ Horner evaluation
// returns p_j(x) for each poly of the batch

// The 29-bit product record of a constant (fr29.hpp mul29): x * 2^261 mod r (x's Montgomery form times
// 32) in 9 x 29-bit limbs + zero pad, as two 32-byte scalar slots; the per-element kernels multiply by
// a uniform constant with it (one mad per partial product, no carry words)
void fr29_record(const Fr& x, Fr out[2]) {
  const Fr y = x * Fr::from_u64(32);
  uint32_t w[16] = {0};
  for (int j = 0; j < 9; j++) {
    const int bit = 29 * j, i = bit >> 6, off = bit & 63;
    uint64_t l = y.v[i] >> off;
    if (off > 35 && i + 1 < 4) l |= y.v[i + 1] << (64 - off);
    w[j] = (uint32_t)(l & 0x1fffffffu);
  }
  memcpy(out[0].v, w, 32);
  memcpy(out[1].v, w + 8, 32);
}

// xp[l] = x^(8 * 2^l) (l < 8), xp[8] = x, xp[9] = x^2048, xp[10..11] = the 29-bit record of x,
// xp[12 + 2l .. 13 + 2l] = the record of xp[l] (l < 8)
uint32_t* xpowers(kgs_ctx& c, const Fr& x) {
  Fr p[28];
  Fr x8 = x.sqr().sqr().sqr();
  p[0] = x8;
  for (int l = 1; l < 8; l++) p[l] = p[l - 1].sqr();
  p[8] = x;
  p[9] = p[7].sqr();  // x^2048
  fr29_record(x, p + 10);
  for (int l = 0; l < 8; l++) fr29_record(p[l], p + 12 + 2 * l);
  return c.scal(p, 28);
}

EvalJob eval_launch(kgs_ctx& c, const std::vector<const uint32_t*>& src, const std::vector<uint64_t>& len, const Fr& x,
                    int slot) {
  EvalJob j;
  j.src = src;
  j.len = len;
  j.x = x;
  uint64_t maxlen = 1;
  for (auto l : len) maxlen = l > maxlen ? l : maxlen;
  j.ntiles = (uint32_t)((maxlen + EVAL_TILE - 1) / EVAL_TILE);
  const int np = (int)src.size();
  uint32_t* xp = xpowers(c, x);
  size_t bytes = (size_t)32 * j.ntiles * (np ? np : 1);
  uint32_t* dpart = c.buf("eval_part_" + std::to_string(slot), bytes);
  // batches of EB_MAX polynomials per launch (any number of multisets), partials contiguous per poly
  for (int p0 = 0; p0 < np; p0 += EB_MAX) {
    EvalBatch eb;
    eb.npolys = np - p0 < EB_MAX ? np - p0 : EB_MAX;
    for (int i = 0; i < eb.npolys; i++) {
      eb.src[i] = src[p0 + i];
      eb.len[i] = len[p0 + i];
    }
    launch_eval_tiles(c.st, dpart + (size_t)8 * j.ntiles * p0, eb, xp, j.ntiles);
    check_launch();
  }
  j.h_part = c.pin(bytes);
  HC(hipMemcpyAsync(j.h_part, dpart, bytes, hipMemcpyDeviceToHost, c.st));
  return j;
}

std::vector<Fr> eval_finish(const EvalJob& j) {
  Fr X = j.x;
  for (int i = 0; i < 11; i++) X = X.sqr();  // x^2048
  std::vector<Fr> out;
  for (size_t p = 0; p < j.src.size(); p++) {
    Fr v = Fr::zero();
    for (uint32_t b = j.ntiles; b-- > 0;) v = v * X + Fr::from_bytes(j.h_part + 32 * ((size_t)p * j.ntiles + b));
    out.push_back(v);
  }
  return out;
}

// ------------------------------------------------------------------ linear combinations
void run_lincomb(hipStream_t st, uint32_t* out, uint64_t n, const LcTerms& t) {
  size_t k = 0;
  bool first = true;
  do {
    LinComb lc{};
    if (!first) {
      lc.src[0] = out;
      lc.len[0] = n;
      Fr::one().to_bytes((uint8_t*)lc.coef[0]);
      Fr rec[2];
      fr29_record(Fr::one(), rec);
      memcpy(lc.coef29[0], rec, 4 * LC_W29);
      lc.nterms = 1;
    }
    for (; k < t.src.size() && lc.nterms < LC_MAX; k++) {
      lc.src[lc.nterms] = t.src[k];
      lc.len[lc.nterms] = t.len[k];
      t.coef[k].to_bytes((uint8_t*)lc.coef[lc.nterms]);
      Fr rec[2];
      fr29_record(t.coef[k], rec);
      memcpy(lc.coef29[lc.nterms], rec, 4 * LC_W29);
      lc.nterms++;
    }
    (first ? t.c0 : Fr::zero()).to_bytes((uint8_t*)lc.c0);
    launch_lincomb(st, out, n, lc);
    check_launch();
    first = false;
  } while (k < t.src.size());
}

// ------------------------------------------------------------------ round 3: divisibility and quotient
// One set of quotient scalars per argument: slot 4, the weight of the selT-binary term (none for a
// lookup, whose selT holds multiplicities), is the argument's own, the rest is shared; slots 2-3 are
// 1/Z_H on the two coset halves times 1/cs (the scaling of the inverse transform that follows; nxm1
// carries it too), slots 5-6 and 7-8 alpha / Z_H on each half as one 29-bit product record. The
// divisibility checks and k_quotient read the argument's set, the fused kernel set 0.
static const uint32_t* quot_scalars(kgs_ctx& c, int nbits, int lcs, bool lookup, const Fr& alpha, const Fr& gamma) {
  const Fr gn = Fr::from_u64(KGS_NTT_COSET_GEN).pow_u64(1ull << nbits);
  const Fr inv_cs = Fr::from_u64(1ull << lcs).inverse();
  Fr qs[9] = {alpha, gamma, (gn - Fr::one()).inverse() * inv_cs, (gn.neg() - Fr::one()).inverse() * inv_cs,
              lookup ? Fr::zero() : alpha};
  fr29_record(alpha * qs[2], qs + 5);
  fr29_record(alpha * qs[3], qs + 7);
  return c.scal(qs, 9);
}

const uint32_t* run_divcheck(kgs_ctx& c, int nbits, int lcs, const QuotIn& a, const Fr& alpha, const Fr& gamma, uint64_t n,
                             uint32_t* flag, const uint32_t* S_next, uint64_t gbase) {
  const uint32_t* d_qs = quot_scalars(c, nbits, lcs, a.lk(), alpha, gamma);
  launch_divcheck(c.st, !a.gs(), a.sel(), flag, a.S, a.F, a.T, a.SF, a.ST, d_qs, n, S_next, gbase);
  return d_qs;
}

void run_quotient(kgs_ctx& c, int nbits, int lcs, const std::vector<QuotIn>& args, const Fr& alpha, const Fr& gamma,
                  const std::vector<Fr>& dpow, uint32_t* Qc, bool fused, const uint32_t* qs0) {
  const int m = (int)args.size();
  const uint32_t rot = (uint32_t)((1ull << lcs) >> nbits);
  const uint32_t* nxm1 = get_nxm1(c, nbits, lcs);
  if (!qs0) qs0 = quot_scalars(c, nbits, lcs, args[0].lk(), alpha, gamma);
  if (!fused) {  // the templated kernel of the single proof
    if (m != 1) throw KgsError(KGS_E_ARG, "the single-argument quotient takes one argument");
    launch_quotient(c.st, !args[0].gs(), args[0].sel(), Qc, args[0].S, args[0].F, args[0].T, args[0].SF, args[0].ST, nxm1,
                    qs0, lcs, rot);
    return;
  }
  for (int j0 = 0; j0 < m; j0 += QM_MAX) {
    QuotMulti qm{};
    qm.nargs = m - j0 < QM_MAX ? m - j0 : QM_MAX;
    qm.accumulate = j0 > 0;
    for (int i = 0; i < qm.nargs; i++) {
      const int j = j0 + i;
      QuotArg& q = qm.a[i];
      q.S = args[j].S;
      q.F = args[j].F;
      q.T = args[j].T;
      q.SF = args[j].SF;
      q.ST = args[j].ST;
      q.prod = !args[j].gs();
      q.sel = args[j].sel();
      q.lookup = args[j].lk();
      dpow[j].to_bytes((uint8_t*)q.delta);
      Fr rec[2];
      fr29_record(dpow[j], rec);
      memcpy(q.delta29, rec, 4 * LC_W29);
    }
    launch_quotient_multi(c.st, Qc, qm, nxm1, qs0, lcs, rot);
  }
}

// Round 2: the four beta combinations of a vector argument (k > 1), sum_i beta^i of the f_i and t_i on H
// and of F_i and T_i in coefficient form, each over `len` elements. The callers launch them (run_lincomb)
// on the streams they choose.
BetaComb beta_combination(const std::vector<uint32_t*>& fm, const std::vector<uint32_t*>& tm,
                          const std::vector<uint32_t*>& Fc, const std::vector<uint32_t*>& Tc, int k, const Fr& beta,
                          uint64_t len) {
  BetaComb b;
  Fr bp = Fr::one();
  for (int i = 0; i < k; i++) {
    b.fcomb.add(fm[i], len, bp);
    b.tcomb.add(tm[i], len, bp);
    b.polF.add(Fc[i], len, bp);
    b.polT.add(Tc[i], len, bp);
    bp = bp * beta;
  }
  return b;
}

// Round 5 (prover.js:320-413): one argument's linearisation r(X) as sum_k coef_k P_k + c0 over S, polT and
// Q, from the challenges and round-4 evaluations. Z_H(xi), L1(xi) as polynomial_utils.js:1-19.
R5 round5_terms(bool gs, bool sel, int k, int nbits, const Fr& alpha, const Fr& beta, const Fr& gamma, const Fr& xi,
                const std::vector<Fr>& fx, const std::vector<Fr>& tx, const Fr& sFx, const Fr& sTx, const Fr& sxiw,
                bool lookup, const Fr* fxi_override) {
  const uint64_t n = 1ull << nbits;
  Fr xn = xi;
  for (int i = 0; i < nbits; i++) xn = xn.sqr();
  const Fr zh = xn - Fr::one();
  const Fr l1 = zh * (Fr::from_u64(n) * (xi - Fr::one())).inverse();
  Fr fxi = Fr::zero(), txi = Fr::zero();
  for (int i = k - 1; i >= 0; i--) {
    fxi = fxi * beta + fx[i];
    if (gs) txi = txi * beta + tx[i];
  }
  if (fxi_override) fxi = *fxi_override;
  const Fr one = Fr::one();
  Fr selBin = Fr::zero();  // alpha^3 selTBin + alpha^2 selFBin (a lookup has no selTBin term)
  if (sel) selBin = ((lookup ? Fr::zero() : (sTx - sTx.sqr()) * alpha) + (sFx - sFx.sqr())) * alpha * alpha;
  R5 r;
  Fr c0;
  if (gs) {
    const Fr fg = fxi + gamma, tg = txi + gamma;
    Fr rc = sxiw * fg * tg + (sel ? sTx * fg - sFx * tg : fxi - txi);
    c0 = selBin + alpha * rc;
    r.terms.push_back({R5_S, 0, l1 - alpha * fg * tg});
    r.terms.push_back({R5_Q, 0, zh.neg()});
  } else {
    const Fr fg = fxi + gamma;
    const Fr dF = sel ? sFx * (fg - one) + one : fg;
    c0 = selBin + alpha * sxiw * (sel ? sTx * (gamma - one) + one : gamma) - l1;
    r.terms.push_back({R5_POLT, 0, alpha * sxiw * (sel ? sTx : one)});
    r.terms.push_back({R5_S, 0, l1 - alpha * dF});
    r.terms.push_back({R5_Q, 0, zh.neg()});
  }
  r.c0 = c0;
  return r;
}

// W_xi's numerator (prover.js:320-413) of a proof of m >= 1 arguments, as the terms of one linear
// combination: sum_j dpow[j] r_j - Z_H(xi) Q, then every polynomial opened at xi minus its value there,
// one power of v each (ArgIn::each_xi by power). Round-1 polynomials, S and polT contribute `len`
// elements, Q `qlen`; c0 is the constant term (global coefficient 0). fxi_override: the reference-quirks
// replay's second value of polF (argument 0 only).
LcTerms wxi_numerator(const std::vector<OpenArg>& args, int nbits, const Fr& alpha, const Fr& beta, const Fr& gamma,
                      const std::vector<Fr>& dpow, const Fr& xi, const Fr& v, const uint32_t* Qc, uint64_t len,
                      uint64_t qlen, const Fr* fxi_override) {
  LcTerms lw;
  Fr c0 = Fr::zero();
  Fr zh_neg = Fr::zero();
  for (size_t j = 0; j < args.size(); j++) {
    const ArgIn& a = *args[j].in;
    const XiEvals& x = *args[j].x;
    const R5 r5 = round5_terms(a.gs(), a.sel(), a.k, nbits, alpha, beta, gamma, xi, x.fx, x.tx, x.sFx, x.sTx, args[j].sxiw,
                               a.lk(), fxi_override);
    for (const R5Term& t : r5.terms) {
      if (t.id == R5_Q) zh_neg = t.coef;
      else lw.add(args[j].polys->poly(t.id, t.idx), len, dpow[j] * t.coef);
    }
    c0 = c0 + dpow[j] * r5.c0;
  }
  lw.add(Qc, qlen, zh_neg);
  Fr vp = Fr::one();
  for (const OpenArg& o : args)
    o.in->each_xi(true, [&](R5Poly id, int i) {
      vp = vp * v;
      lw.add(o.polys->poly(id, i), len, vp);
      c0 = c0 - vp * o.x->at(id, i);
    });
  lw.c0 = c0;
  return lw;
}

// The single-argument prover: its own checks, the rank-group dispatch, then the rounds (prover_rounds.cpp)
// with what is special about it — kgs_prove's host-boundary hooks, round 1 piped over the two lanes when
// commitments are split, and the reference's behaviour on degenerate inputs (never for a lookup).
void prove_impl(kgs_ctx& c, const ProveIn& in, uint8_t* com_out, uint8_t* ev_out) {
  if (in.kind != KGS_GRANDSUM && in.kind != KGS_GRANDPRODUCT && in.kind != KGS_LOOKUP)
    throw KgsError(KGS_E_ARG, "unknown argument kind");
  if (in.kind == KGS_LOOKUP && !in.sel_f)
    throw KgsError(KGS_E_ARG, "a lookup needs both selectors (sel_t holds the multiplicities)");
  c.xs.reset();
  ensure_twin(c);  // a domain last grown by a quirks replay has no 29-bit twin yet
  if (c.group) {
    prove_dist_group(c, in, com_out, ev_out);
    return;
  }
  if (in.nbits < 1) throw KgsError(KGS_E_ARG, "nbits must be >= 1");
  check_srs(c, in.nbits);
  if (in.nbits > c.nbits_max) throw KgsError(KGS_E_SRS, "SRS loaded for a smaller maximum domain; reload with larger nbits_max");
  if (in.npols < 1) throw KgsError(KGS_E_ARG, "The number of multisets must be greater than 0.");
  if (in.npols > KGS_MAX_POLS) throw KgsError(KGS_E_ARG, "too many multisets");
  RoundOpts o;
  o.hooks = &in;
  o.piped_round1 = split_commits(c);
  o.ref_quirks = c.ref_quirks && in.kind != KGS_LOOKUP;
  prove_rounds(c, in.nbits, {in.arg()}, o, com_out, ev_out);
}

}  // namespace

// ================================================================== C-ABI
extern "C" {

int kgs_ctx_create(int device, kgs_ctx_t** out) {
  API_BEGIN
  if (!out) throw KgsError(KGS_E_ARG, "out is NULL");
  int ndev = 0;
  HC(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) throw KgsError(KGS_E_ARG, "no such HIP device");
  HC(hipSetDevice(device));
  auto* c = new kgs_ctx();
  c->device = device;
  HC(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
  // the second MSM lane and the copy stream are created on first use: contexts that never need
  // them keep one stream (several in-flight contexts share the device's few hardware queues)
  c->d_scal = c->buf("scalars", kgs_ctx::SCAL_BYTES);
  // reference-identical behaviour on degenerate inputs by default (kgs.h); KGS_REFERENCE_QUIRKS=0
  // selects the exact-math prover
  c->ref_quirks = true;
  if (const char* e = getenv("KGS_REFERENCE_QUIRKS")) c->ref_quirks = e[0] != '0';
  c->ensure_pin(8 << 20);
  *out = c;
  API_END
}

void kgs_ctx_destroy(kgs_ctx_t* ctx) {
  if (!ctx) return;
  { std::lock_guard<std::mutex> lk(ctx->mu); }  // wait for a call still running on another thread
  delete ctx;
}

int kgs_device_count(int* count) {
  API_BEGIN
  if (!count) throw KgsError(KGS_E_ARG, "NULL argument");
  int n = 0;
  HC(hipGetDeviceCount(&n));
  *count = n;
  API_END
}

int kgs_ctx_set_reference_quirks(kgs_ctx_t* ctx, int on) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  ctx->ref_quirks = on != 0;
  API_END
}

int kgs_ctx_idle(kgs_ctx_t* ctx) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  HC(hipSetDevice(ctx->device));
  for (const auto& s : ctx->streams()) {
    if (!s.st) continue;
    const hipError_t e = hipStreamQuery(s.st);
    if (e == hipErrorNotReady) return 0;
    HC(e);
  }
  return 1;
  API_END
}

int kgs_prove_device(kgs_ctx_t* ctx, int kind, int nbits, int npols, const void* const* d_evals_f,
                     const void* const* d_evals_t, const void* d_sel_f, const void* d_sel_t, uint8_t* commitments_out,
                     uint8_t* evaluations_out) {
  API_BEGIN
  if (!ctx || !d_evals_f || !d_evals_t || !commitments_out || !evaluations_out) throw KgsError(KGS_E_ARG, "NULL argument");
  CTX_LOCK(ctx);
  if ((d_sel_f == nullptr) != (d_sel_t == nullptr)) throw KgsError(KGS_E_ARG, "selectors must be both given or both NULL");
  if (npols < 1 || npols > KGS_MAX_POLS || nbits < 1 || nbits > 28) throw KgsError(KGS_E_ARG, "bad shape");
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);  // no kernel of a failed call still reads the caller's device buffers
  ProveIn in;
  in.kind = kind;
  in.nbits = nbits;
  in.npols = npols;
  for (int i = 0; i < npols; i++) {
    in.f_std.push_back((const uint32_t*)d_evals_f[i]);
    in.t_std.push_back((const uint32_t*)d_evals_t[i]);
  }
  in.sel_f = (const uint32_t*)d_sel_f;
  in.sel_t = (const uint32_t*)d_sel_t;
  prove_impl(*ctx, in, commitments_out, evaluations_out);
  API_END
}

int kgs_last_timing(kgs_ctx_t* ctx, double* rounds_ms, int max_rounds) {
  if (!ctx || !rounds_ms) return KGS_E_ARG;
  CTX_LOCK(ctx);
  int n = (int)ctx->timing.size() < max_rounds ? (int)ctx->timing.size() : max_rounds;
  for (int i = 0; i < n; i++) rounds_ms[i] = ctx->timing[i];
  return n;
}

int kgs_ctx_set_shard(kgs_ctx_t* ctx, int rank, int world, kgs_allgather_fn fn, void* user) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "ctx is NULL");
  CTX_LOCK(ctx);
  if (world < 1 || rank < 0 || rank >= world) throw KgsError(KGS_E_ARG, "bad shard rank/world");
  if (world > 1 && !fn) throw KgsError(KGS_E_ARG, "sharding needs an all-gather callback");
  ctx->shard_rank = world > 1 ? rank : 0;
  ctx->shard_world = world;
  ctx->shard_fn = world > 1 ? fn : nullptr;
  ctx->shard_user = world > 1 ? user : nullptr;
  API_END
}

int kgs_ctx_set_msm_lanes(kgs_ctx_t* ctx, int lanes) {
  API_BEGIN
  if (!ctx || lanes < 1 || lanes > 2) throw KgsError(KGS_E_ARG, "msm lanes must be 1 or 2");
  CTX_LOCK(ctx);
  ctx->msm_lanes = lanes;
  API_END
}

}  // extern "C"
