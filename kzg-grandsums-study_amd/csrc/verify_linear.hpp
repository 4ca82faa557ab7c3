// The verifiers' pairing equation as a linear form (host only, no GPU): shared by verifier.cpp
// (kgs_verify) and verify_batch.cpp (kgs_verify_batch, kgs_g1_lincomb).
//
// For a proof of ncom commitments C_0 .. C_{ncom-1} (fixed order of kgs_proof_shape) the check of
// src/{grandsum,grandproduct}/mset_eq_kzg_verifier.js is e(-A, [tau]2) * e(B, [1]2) == 1 with
//   A = 1 * Wxi + u * Wxiw
//   B = sum_j b_j * C_j + b_G * G1
// where every b_j and b_G is an element of Fr computed from the transcript challenges and the
// proof's evaluations alone. linear_form() does the structural checks, the transcript replay and
// that Fr arithmetic, and returns the scalars; no point is touched beyond the on-curve check.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "host_field.hpp"
#include "transcript.hpp"

namespace kgs {
namespace host {

inline bool lt_mod(const uint8_t* le, const uint64_t* p) {  // little-endian 256-bit value < p
  for (int i = 3; i >= 0; i--) {
    uint64_t w;
    memcpy(&w, le + 8 * i, 8);
    if (w != p[i]) return w < p[i];
  }
  return false;
}

// G1.isValid on an affine LEM point: infinity, or canonical coordinates on y^2 = x^3 + 3
inline bool g1_valid(const uint8_t* lem) {
  bool zero = true;
  for (int i = 0; i < 64; i++) zero &= lem[i] == 0;
  if (zero) return true;
  if (!lt_mod(lem, FQ_MOD.p) || !lt_mod(lem + 32, FQ_MOD.p)) return false;
  Fq x = Fq::from_bytes(lem), y = Fq::from_bytes(lem + 32);
  return y.sqr() == x.sqr() * x + Fq::from_u64(3);
}

inline void g1_gen_lem(uint8_t out[64]) {
  Fq::one().to_bytes(out);
  Fq::from_u64(2).to_bytes(out + 32);
}

struct Proof {
  int npols;
  bool sel, gs;
  const uint8_t* com;  // fixed order (kgs_proof_shape)
  const uint8_t* ev;
  bool lookup = false;  // KGS_LOOKUP: no binary constraint on selT
  // commitment indices
  int iF(int i) const { return 2 * i; }
  int iT(int i) const { return 2 * i + 1; }
  int iselF() const { return 2 * npols; }
  int iselT() const { return 2 * npols + 1; }
  int base() const { return 2 * npols + (sel ? 2 : 0); }
  int iS() const { return base(); }  // S (grand-sum) or Z (grand-product)
  int iQ() const { return base() + 1; }
  int iWxi() const { return base() + 2; }
  int iWxiw() const { return base() + 3; }
  int ncom() const { return base() + 4; }
  const uint8_t* C(int j) const { return com + 64 * (size_t)j; }
  const uint8_t* F(int i) const { return C(iF(i)); }
  const uint8_t* T(int i) const { return C(iT(i)); }
  const uint8_t* selF() const { return C(iselF()); }
  const uint8_t* selT() const { return C(iselT()); }
  const uint8_t* S() const { return C(iS()); }
  const uint8_t* Q() const { return C(iQ()); }
  const uint8_t* Wxi() const { return C(iWxi()); }
  const uint8_t* Wxiw() const { return C(iWxiw()); }
  // evaluation indices: per pol f (and t for grand-sum), then selF, selT, then S(xi w) / Z(xi w)
  int per() const { return gs ? 2 : 1; }
  const uint8_t* fxi_raw(int i) const { return ev + 32 * (size_t)(per() * i); }
  const uint8_t* txi_raw(int i) const { return ev + 32 * (size_t)(per() * i + 1); }
  const uint8_t* selFxi_raw() const { return ev + 32 * (size_t)(per() * npols); }
  const uint8_t* selTxi_raw() const { return ev + 32 * (size_t)(per() * npols + 1); }
  const uint8_t* sxiw_raw() const { return ev + 32 * (size_t)(per() * npols + (sel ? 2 : 0)); }
  int nev() const { return per() * npols + (sel ? 2 : 0) + 1; }
};

// validateCommitments / validateEvaluations (grandsum verifier.js:194-244, grandproduct :200-233)
inline bool proof_structure_ok(const Proof& p) {
  for (int i = 0; i < p.ncom(); i++)
    if (!g1_valid(p.C(i))) return false;
  for (int i = 0; i < p.nev(); i++)
    if (!lt_mod(p.ev + 32 * (size_t)i, FR_MOD.p)) return false;
  return true;
}

// fr_w(k) for k <= 28, computed once (fr_w raises 5 to a 226-bit power on every call)
inline const Fr& fr_w_cached(int k) {
  static const std::vector<Fr> tab = [] {
    std::vector<Fr> t(29);
    t[28] = fr_w(28);
    for (int s = 27; s >= 0; s--) t[s] = t[s + 1].sqr();
    return t;
  }();
  return tab[k];
}

// The challenges of a proof whose commitments lie in proof order (ncom1 round-1 commitments, m S, Q, Wxi,
// Wxiw) and whose nev evaluations lie in transcript order: the schedule's stages back to back
// (transcript.hpp; computeChallenges, grandsum verifier.js:246-312)
struct Challenges {
  Fr beta, gamma, alpha, delta, xi, v, u;
};
inline Challenges replay_schedule(const uint8_t* com, int ncom1, int m, const uint8_t* ev, int nev, bool any_vec) {
  const uint8_t *S = com + 64 * (size_t)ncom1, *Q = S + 64 * (size_t)m;
  std::vector<Fr> evals(nev);
  for (int i = 0; i < nev; i++) evals[i] = Fr::from_bytes(ev + 32 * (size_t)i);
  Schedule sch;
  Challenges c;
  const Schedule::BetaGamma bg = sch.after_round1(com, ncom1, any_vec);
  const Schedule::AlphaDelta ad = sch.after_round2(S, m);
  c.beta = bg.beta;
  c.gamma = bg.gamma;
  c.alpha = ad.alpha;
  c.delta = ad.delta;
  c.xi = sch.after_round3(Q);
  c.v = sch.after_round4(evals.data(), evals.size());
  c.u = sch.after_round5(Q + 64, Q + 128);
  return c;
}

struct LinearForm {
  Fr a_wxi, a_wxiw;   // A = a_wxi * Wxi + a_wxiw * Wxiw
  std::vector<Fr> b;  // B = sum_j b[j] * C_j + b_g * G1, j in the commitment order of the proof
  Fr b_g;
};

// The scalars of a structurally valid proof (proof_structure_ok). Follows verify_impl of verifier.cpp
// line by line; every point operation there becomes an addition into the coefficient of its point.
inline LinearForm linear_form(const Proof& p, int nbits) {
  const int k = p.npols;
  const bool vec = k > 1;
  auto fr_at = [](const uint8_t* b) { return Fr::from_bytes(b); };
  // computeChallenges (grandsum verifier.js:246-312)
  const Challenges ch = replay_schedule(p.com, p.base(), 1, p.ev, p.nev(), vec);
  const Fr &beta = ch.beta, &gamma = ch.gamma, &alpha = ch.alpha, &xi = ch.xi, &v = ch.v, &u = ch.u;
  const Fr sxiw = fr_at(p.sxiw_raw());

  // Z_H(xi), L1(xi) (polynomial_utils.js:1-19)
  Fr xn = xi;
  for (int i = 0; i < nbits; i++) xn = xn.sqr();
  const Fr zh = xn - Fr::one();
  const Fr l1 = zh * (Fr::from_u64(1ull << nbits) * (xi - Fr::one())).inverse();
  const Fr w = fr_w_cached(nbits);

  LinearForm lf;
  lf.b.assign(p.ncom(), Fr::zero());
  Fr r0 = Fr::zero();
  Fr selF = Fr::zero(), selT = Fr::zero();
  if (p.sel) {
    selF = fr_at(p.selFxi_raw());
    selT = fr_at(p.selTxi_raw());
    if (!p.lookup) r0 = r0 + (selT - selT.sqr());  // a lookup's selT holds multiplicities
    r0 = r0 * alpha;
    r0 = (r0 + (selF - selF.sqr())) * alpha;
  }
  Fr fxi = Fr::zero(), txi = Fr::zero();
  for (int i = k - 1; i >= 0; i--) {
    fxi = fxi * beta + fr_at(p.fxi_raw(i));
    if (p.gs) txi = txi * beta + fr_at(p.txi_raw(i));
  }
  // [D]1 = d11 * S - Z_H * Q (+ D12 for the grand-product), with coefficient v^0 in [F]1
  if (p.gs) {
    const Fr fg = fxi + gamma, tg = txi + gamma;
    Fr r01 = sxiw * (fg * tg);
    if (p.sel)
      r01 = r01 + selT * fg - selF * tg;
    else
      r01 = r01 + fxi - txi;
    r0 = (r0 + r01) * alpha;
    lf.b[p.iS()] = (l1 - alpha * fg * tg) + u;
  } else {
    Fr r01 = sxiw;
    r01 = p.sel ? r01 * ((gamma - Fr::one()) * selT + Fr::one()) : r01 * gamma;
    r0 = (r0 + r01) * alpha;
    r0 = r0 - l1;
    Fr fg = fxi + gamma;
    if (p.sel) fg = (fg - Fr::one()) * selF + Fr::one();
    lf.b[p.iS()] = (l1 - alpha * fg) + u;
    // D12 = alpha * sxiw * [selT(xi)] * sum_i beta^i T_i
    Fr c = sxiw * alpha;
    if (p.sel) c = c * selT;
    for (int i = 0; i < k; i++) {
      lf.b[p.iT(i)] = lf.b[p.iT(i)] + c;
      c = c * beta;
    }
  }
  lf.b[p.iQ()] = zh.neg();
  // [F]1 (grandsum verifier.js:125-142) and [E]1 (:146-167): v^(i+1) on F_i and f_i(xi), then the
  // T_i / t_i(xi) of a grand-sum, then selF, selT
  Fr E = u * sxiw - r0;
  Fr pw = v;
  for (int i = 0; i < k; i++) {
    lf.b[p.iF(i)] = lf.b[p.iF(i)] + pw;
    E = E + pw * fr_at(p.fxi_raw(i));
    pw = pw * v;
  }
  if (p.gs)
    for (int i = 0; i < k; i++) {
      lf.b[p.iT(i)] = lf.b[p.iT(i)] + pw;
      E = E + pw * fr_at(p.txi_raw(i));
      pw = pw * v;
    }
  if (p.sel) {
    lf.b[p.iselF()] = lf.b[p.iselF()] + pw;
    E = E + pw * selF;
    pw = pw * v;
    lf.b[p.iselT()] = lf.b[p.iselT()] + pw;
    E = E + pw * selT;
  }
  lf.b_g = E.neg();
  // pairing equation (:170-186)
  lf.a_wxi = Fr::one();
  lf.a_wxiw = u;
  lf.b[p.iWxi()] = xi;
  lf.b[p.iWxiw()] = u * xi * w;
  return lf;
}

// ---- multi-argument proofs (kgs_verify_multi; layout and transcript in include/kgs.h)
struct ArgShape {
  int npols;
  bool sel, gs, lookup;
  int ncom1() const { return 2 * npols + (sel ? 2 : 0); }           // round-1 commitments
  int nev() const { return (gs ? 2 : 1) * npols + (sel ? 2 : 0); }  // evaluations at xi
};
struct MultiProof {
  std::vector<ArgShape> args;
  const uint8_t* com;
  const uint8_t* ev;
  int m() const { return (int)args.size(); }
  int ncom1() const {
    int s = 0;
    for (const ArgShape& a : args) s += a.ncom1();
    return s;
  }
  int nev_xi() const {
    int s = 0;
    for (const ArgShape& a : args) s += a.nev();
    return s;
  }
  int iS(int j) const { return ncom1() + j; }
  int iQ() const { return ncom1() + m(); }
  int iWxi() const { return iQ() + 1; }
  int iWxiw() const { return iQ() + 2; }
  int ncom() const { return iQ() + 3; }
  int nev() const { return nev_xi() + m(); }
  const uint8_t* C(int i) const { return com + 64 * (size_t)i; }
  const uint8_t* E(int i) const { return ev + 32 * (size_t)i; }
};

inline bool multi_structure_ok(const MultiProof& p) {
  for (int i = 0; i < p.ncom(); i++)
    if (!g1_valid(p.C(i))) return false;
  for (int i = 0; i < p.nev(); i++)
    if (!lt_mod(p.E(i), FR_MOD.p)) return false;
  return true;
}

// The scalars of a structurally valid multi-argument proof: per argument exactly linear_form's terms
// under the shared challenges, weighted by delta^j; the openings' powers of v run over all arguments.
inline LinearForm linear_form_multi(const MultiProof& p, int nbits) {
  const int m = p.m();
  auto fr_at = [](const uint8_t* b) { return Fr::from_bytes(b); };
  bool any_vec = false;
  for (const ArgShape& a : p.args) any_vec |= a.npols > 1;
  const Challenges ch = replay_schedule(p.com, p.ncom1(), m, p.ev, p.nev(), any_vec);
  const Fr &beta = ch.beta, &gamma = ch.gamma, &alpha = ch.alpha, &delta = ch.delta, &xi = ch.xi, &v = ch.v, &u = ch.u;

  Fr xn = xi;
  for (int i = 0; i < nbits; i++) xn = xn.sqr();
  const Fr zh = xn - Fr::one();
  const Fr l1 = zh * (Fr::from_u64(1ull << nbits) * (xi - Fr::one())).inverse();
  const Fr w = fr_w_cached(nbits);

  LinearForm lf;
  lf.b.assign(p.ncom(), Fr::zero());
  Fr E = Fr::zero();  // b_g = -E
  Fr dj = Fr::one(), vj = Fr::one(), pw = v;
  int c0 = 0, e0 = 0;  // argument j's first commitment / evaluation
  for (int j = 0; j < m; j++) {
    const ArgShape& a = p.args[j];
    const int k = a.npols, per = a.gs ? 2 : 1;
    auto fx = [&](int i) { return fr_at(p.E(e0 + per * i)); };
    auto tx = [&](int i) { return fr_at(p.E(e0 + per * i + 1)); };
    const int iF0 = c0, iselF = c0 + 2 * k, eSel = e0 + per * k;
    const Fr sxiw = fr_at(p.E(p.nev_xi() + j));
    Fr r0 = Fr::zero();
    Fr selF = Fr::zero(), selT = Fr::zero();
    if (a.sel) {
      selF = fr_at(p.E(eSel));
      selT = fr_at(p.E(eSel + 1));
      if (!a.lookup) r0 = r0 + (selT - selT.sqr());
      r0 = r0 * alpha;
      r0 = (r0 + (selF - selF.sqr())) * alpha;
    }
    Fr fxi = Fr::zero(), txi = Fr::zero();
    for (int i = k - 1; i >= 0; i--) {
      fxi = fxi * beta + fx(i);
      if (a.gs) txi = txi * beta + tx(i);
    }
    Fr bS;
    if (a.gs) {
      const Fr fg = fxi + gamma, tg = txi + gamma;
      Fr r01 = sxiw * (fg * tg);
      if (a.sel)
        r01 = r01 + selT * fg - selF * tg;
      else
        r01 = r01 + fxi - txi;
      r0 = (r0 + r01) * alpha;
      bS = l1 - alpha * fg * tg;
    } else {
      Fr r01 = sxiw;
      r01 = a.sel ? r01 * ((gamma - Fr::one()) * selT + Fr::one()) : r01 * gamma;
      r0 = (r0 + r01) * alpha;
      r0 = r0 - l1;
      Fr fg = fxi + gamma;
      if (a.sel) fg = (fg - Fr::one()) * selF + Fr::one();
      bS = l1 - alpha * fg;
      Fr c = sxiw * alpha * dj;
      if (a.sel) c = c * selT;
      for (int i = 0; i < k; i++) {
        lf.b[iF0 + 2 * i + 1] = lf.b[iF0 + 2 * i + 1] + c;
        c = c * beta;
      }
    }
    lf.b[p.iS(j)] = dj * bS + u * vj;
    E = E + u * vj * sxiw - dj * r0;
    for (int i = 0; i < k; i++) {
      lf.b[iF0 + 2 * i] = lf.b[iF0 + 2 * i] + pw;
      E = E + pw * fx(i);
      pw = pw * v;
    }
    if (a.gs)
      for (int i = 0; i < k; i++) {
        lf.b[iF0 + 2 * i + 1] = lf.b[iF0 + 2 * i + 1] + pw;
        E = E + pw * tx(i);
        pw = pw * v;
      }
    if (a.sel) {
      lf.b[iselF] = lf.b[iselF] + pw;
      E = E + pw * selF;
      pw = pw * v;
      lf.b[iselF + 1] = lf.b[iselF + 1] + pw;
      E = E + pw * selT;
      pw = pw * v;
    }
    c0 += a.ncom1();
    e0 += a.nev();
    dj = dj * delta;
    vj = vj * v;
  }
  lf.b[p.iQ()] = zh.neg();
  lf.b_g = E.neg();
  lf.a_wxi = Fr::one();
  lf.a_wxiw = u;
  lf.b[p.iWxi()] = xi;
  lf.b[p.iWxiw()] = u * xi * w;
  return lf;
}

// sum_t s_t * P_t over one segment (Straus: the terms share the doublings). Points are affine LEM on
// the curve (or zero), scalars 32 B little-endian standard form, any 256-bit integer.
inline G1 g1_lincomb_segment(const uint8_t* points_lem, const uint8_t* scalars_std, size_t nterms) {
  std::vector<G1> pts(nterms);
  int top = -1;
  for (size_t t = 0; t < nterms; t++) {
    pts[t] = G1::from_affine_lem(points_lem + 64 * t);
    if (pts[t].is_inf()) continue;
    for (int i = 255; i > top; i--)
      if ((scalars_std[32 * t + (i >> 3)] >> (i & 7)) & 1) {
        top = i;
        break;
      }
  }
  G1 acc = G1::inf();
  for (int i = top; i >= 0; i--) {
    acc = acc.dbl();
    for (size_t t = 0; t < nterms; t++)
      if ((scalars_std[32 * t + (i >> 3)] >> (i & 7)) & 1) acc = acc.add(pts[t]);
  }
  return acc;
}

}  // namespace host
}  // namespace kgs
