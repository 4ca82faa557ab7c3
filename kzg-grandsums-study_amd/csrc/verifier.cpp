// Native verifiers for both arguments (host C++, no GPU): kgs_verify / kgs_verify_ptau.
//
// Restates src/grandsum/mset_eq_kzg_verifier.js:9-313 and
// src/grandproduct/mset_eq_kzg_verifier.js:9-299 step by step: validate the commitments (on G1)
// and the evaluations (< r), replay the Keccak transcript (beta only for vector arguments; an
// absent beta multiplies zero, Appendix C.4 of SURVEY.md), evaluate Z_H(xi) and L1(xi), build
// r0, [D]1, [F]1, [E]1, and decide e(-A, [tau]2) * e(B, [1]2) == 1 with the optimal-ate pairing.
// Inputs use the fixed C-ABI order of kgs_prove (include/kgs.h, kgs_proof_shape).
#include <stdio.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kgs.h"
#include "host_field.hpp"
#include "host_pairing.hpp"
#include "transcript.hpp"
#include "verify_linear.hpp"

using namespace kgs;
using host::Fq;
using host::Fr;
using host::G1;
using host::Proof;  // proof layout, lt_mod, g1_valid: verify_linear.hpp (shared with verify_batch.cpp)
using host::g1_valid;
using host::lt_mod;

namespace {

Fr fr_at(const uint8_t* b) { return Fr::from_bytes(b); }
G1 pt(const uint8_t* lem) { return G1::from_affine_lem(lem); }

bool verify_impl(const Proof& p, int nbits, const host::G2A& tau_g2) {
  const int k = p.npols;
  const bool vec = k > 1;
  // validateCommitments / validateEvaluations (grandsum verifier.js:194-244, grandproduct :200-233)
  for (int i = 0; i < p.ncom(); i++)
    if (!g1_valid(p.com + 64 * i)) return false;
  for (int i = 0; i < p.nev(); i++)
    if (!lt_mod(p.ev + 32 * i, host::FR_MOD.p)) return false;

  // computeChallenges (grandsum verifier.js:246-312)
  const host::Challenges ch = host::replay_schedule(p.com, p.base(), 1, p.ev, p.nev(), vec);
  const Fr &beta = ch.beta, &gamma = ch.gamma, &alpha = ch.alpha, &xi = ch.xi, &v = ch.v, &u = ch.u;
  const Fr sxiw = fr_at(p.sxiw_raw());

  // Z_H(xi), L1(xi) (polynomial_utils.js:1-19)
  Fr xn = xi;
  for (int i = 0; i < nbits; i++) xn = xn.sqr();
  const Fr zh = xn - Fr::one();
  const Fr l1 = zh * (Fr::from_u64(1ull << nbits) * (xi - Fr::one())).inverse();
  const Fr w = host::fr_w(nbits);

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
  G1 D1;
  if (p.gs) {
    const Fr fg = fxi + gamma, tg = txi + gamma;
    Fr r01 = sxiw * (fg * tg);
    if (p.sel)
      r01 = r01 + selT * fg - selF * tg;
    else
      r01 = r01 + fxi - txi;
    r0 = (r0 + r01) * alpha;
    const Fr d11 = (l1 - alpha * fg * tg) + u;
    D1 = pt(p.S()).mul(d11).add(pt(p.Q()).mul(zh).neg());
  } else {
    Fr r01 = sxiw;
    r01 = p.sel ? r01 * ((gamma - Fr::one()) * selT + Fr::one()) : r01 * gamma;
    r0 = (r0 + r01) * alpha;
    r0 = r0 - l1;
    Fr fg = fxi + gamma;
    if (p.sel) fg = (fg - Fr::one()) * selF + Fr::one();
    const Fr d11 = (l1 - alpha * fg) + u;
    G1 D12 = G1::inf();
    for (int i = k - 1; i >= 0; i--) D12 = D12.mul(beta).add(pt(p.T(i)));
    if (p.sel) D12 = D12.mul(selT);
    D12 = D12.mul(sxiw).mul(alpha);
    D1 = pt(p.S()).mul(d11).add(D12).add(pt(p.Q()).mul(zh).neg());
  }
  // [F]1 (grandsum verifier.js:125-142)
  G1 F1 = G1::inf();
  if (p.sel) {
    F1 = F1.add(pt(p.selT()));
    F1 = F1.mul(v).add(pt(p.selF()));
  }
  if (p.gs)
    for (int i = k - 1; i >= 0; i--) F1 = F1.mul(v).add(pt(p.T(i)));
  for (int i = k - 1; i >= 0; i--) F1 = F1.mul(v).add(pt(p.F(i)));
  F1 = F1.mul(v).add(D1);
  // [E]1 (:146-167)
  Fr E = Fr::zero();
  if (p.sel) {
    E = E + selT;
    E = E * v + selF;
  }
  if (p.gs)
    for (int i = k - 1; i >= 0; i--) E = E * v + fr_at(p.txi_raw(i));
  for (int i = k - 1; i >= 0; i--) E = E * v + fr_at(p.fxi_raw(i));
  E = E * v + u * sxiw - r0;
  uint8_t g1gen[64];
  Fq::one().to_bytes(g1gen);
  Fq::from_u64(2).to_bytes(g1gen + 32);
  const G1 E1 = pt(g1gen).mul(E);
  // pairing equation (:170-186)
  const G1 A = pt(p.Wxi()).add(pt(p.Wxiw()).mul(u));
  G1 Bp;
  if (p.gs)
    Bp = pt(p.Wxi()).add(pt(p.Wxiw()).mul(u * w)).mul(xi);
  else
    Bp = pt(p.Wxi()).mul(xi).add(pt(p.Wxiw()).mul(u * xi * w));
  Bp = Bp.add(F1).add(E1.neg());
  return host::pairing_eq2(A.neg(), tau_g2, Bp, host::g2_gen());
}

thread_local std::string v_err;

// kgs_verify_multi: the shapes as a MultiProof, or false for a bad count / kind / npols / lookup shape
bool multi_shape(const kgs_arg_shape_t* args, int count, host::MultiProof& p) {
  if (!args || count < 1 || count > KGS_MAX_ARGS) return false;
  for (int j = 0; j < count; j++) {
    const kgs_arg_shape_t& a = args[j];
    if (a.kind != KGS_GRANDSUM && a.kind != KGS_GRANDPRODUCT && a.kind != KGS_LOOKUP) return false;
    if (a.kind == KGS_LOOKUP && !a.selected) return false;
    if (a.npols < 1 || a.npols > (1 << 20)) return false;
    p.args.push_back({a.npols, a.selected != 0, a.kind != KGS_GRANDPRODUCT, a.kind == KGS_LOOKUP});
  }
  return true;
}

// e(-A, [tau]2) * e(B, [1]2) == 1 with A, B from the proof's linear form (verify_linear.hpp)
bool verify_multi_impl(const host::MultiProof& p, int nbits, const host::G2A& tau_g2) {
  if (!host::multi_structure_ok(p)) return false;
  const host::LinearForm lf = host::linear_form_multi(p, nbits);
  const G1 A = pt(p.C(p.iWxi())).mul(lf.a_wxi).add(pt(p.C(p.iWxiw())).mul(lf.a_wxiw));
  uint8_t g1gen[64];
  host::g1_gen_lem(g1gen);
  G1 B = pt(g1gen).mul(lf.b_g);
  for (int i = 0; i < p.ncom(); i++) B = B.add(pt(p.C(i)).mul(lf.b[i]));
  return host::pairing_eq2(A.neg(), tau_g2, B, host::g2_gen());
}

}  // namespace

extern "C" {

int kgs_proof_shape(int kind, int npols, int selected, int* n_commitments, int* n_evaluations) {
  if (npols < 1 || npols > (1 << 20)) return KGS_E_ARG;
  if (n_commitments) *n_commitments = 2 * npols + (selected ? 2 : 0) + 4;
  if (kind != KGS_GRANDSUM && kind != KGS_GRANDPRODUCT && kind != KGS_LOOKUP) return KGS_E_ARG;
  if (n_evaluations) *n_evaluations = (kind != KGS_GRANDPRODUCT ? 2 : 1) * npols + (selected ? 2 : 0) + 1;
  return KGS_OK;
}

int kgs_verify(int kind, int nbits, int npols, int selected, const uint8_t* commitments, const uint8_t* evaluations,
               const uint8_t tau_g2[128]) {
  if ((kind != KGS_GRANDSUM && kind != KGS_GRANDPRODUCT && kind != KGS_LOOKUP) || (kind == KGS_LOOKUP && !selected) ||
      nbits < 1 || nbits > 28 || npols < 1 || !commitments ||
      !evaluations || !tau_g2)
    return KGS_E_ARG;
  try {
    Proof p{npols, selected != 0, kind != KGS_GRANDPRODUCT, commitments, evaluations, kind == KGS_LOOKUP};
    host::G2A t2 = host::g2_from_lem(tau_g2);
    if (!host::g2_on_curve(t2)) return KGS_E_ARG;
    return verify_impl(p, nbits, t2) ? 1 : 0;
  } catch (const std::exception&) {
    return KGS_E_ARG;
  }
}

int kgs_multi_proof_shape(const kgs_arg_shape_t* args, int count, int* n_commitments, int* n_evaluations) {
  host::MultiProof p{{}, nullptr, nullptr};
  if (!multi_shape(args, count, p)) return KGS_E_ARG;
  if (n_commitments) *n_commitments = p.ncom();
  if (n_evaluations) *n_evaluations = p.nev();
  return KGS_OK;
}

int kgs_verify_multi(int nbits, const kgs_arg_shape_t* args, int count, const uint8_t* commitments,
                     const uint8_t* evaluations, const uint8_t tau_g2[128]) {
  if (nbits < 1 || nbits > 28 || !commitments || !evaluations || !tau_g2) return KGS_E_ARG;
  try {
    host::MultiProof p{{}, commitments, evaluations};
    if (!multi_shape(args, count, p)) return KGS_E_ARG;
    host::G2A t2 = host::g2_from_lem(tau_g2);
    if (!host::g2_on_curve(t2)) return KGS_E_ARG;
    return verify_multi_impl(p, nbits, t2) ? 1 : 0;
  } catch (const std::exception&) {
    return KGS_E_ARG;
  }
}

int kgs_verify_multi_ptau(const char* ptau_path, int nbits, const kgs_arg_shape_t* args, int count,
                          const uint8_t* commitments, const uint8_t* evaluations) {
  uint8_t t2[128];
  int rc = kgs_ptau_read_tau_g2(ptau_path, t2);
  if (rc < 0) return rc;
  return kgs_verify_multi(nbits, args, count, commitments, evaluations, t2);
}

int kgs_pairing_eq(int npairs, const uint8_t* g1_lem, const uint8_t* g2_lem) {
  if (npairs < 0 || npairs > 4096 || (npairs && (!g1_lem || !g2_lem))) return KGS_E_ARG;
  try {
    std::vector<host::G1> a(npairs);
    std::vector<host::G2A> b(npairs);
    std::vector<const host::G1*> pa(npairs);
    std::vector<const host::G2A*> pb(npairs);
    for (int k = 0; k < npairs; k++) {
      const uint8_t* p1 = g1_lem + 64 * (size_t)k;
      if (!host::g1_lem_on_curve(p1)) return KGS_E_ARG;
      a[k] = host::G1::from_affine_lem(p1);
      b[k] = host::g2_from_lem(g2_lem + 128 * (size_t)k);
      if (!host::g2_on_curve(b[k])) return KGS_E_ARG;
      pa[k] = &a[k];
      pb[k] = &b[k];
    }
    return host::pairing_eq(pa.data(), pb.data(), npairs) ? 1 : 0;
  } catch (const std::exception&) {
    return KGS_E_ARG;
  }
}

int kgs_kzg_verify(const uint8_t commit_lem[64], const uint8_t z_mont[32], const uint8_t y_mont[32],
                   const uint8_t proof_lem[64], const uint8_t tau_g2[128]) {
  if (!commit_lem || !z_mont || !y_mont || !proof_lem || !tau_g2) return KGS_E_ARG;
  try {
    const host::G2A t2 = host::g2_from_lem(tau_g2);
    if (!host::g2_on_curve(t2)) return KGS_E_ARG;
    if (!host::g1_valid(commit_lem) || !host::g1_valid(proof_lem) || !host::lt_mod(z_mont, host::FR_MOD.p) ||
        !host::lt_mod(y_mont, host::FR_MOD.p))
      return 0;
    const G1 W = pt(proof_lem);
    uint8_t g1gen[64];
    host::g1_gen_lem(g1gen);
    // e(-W, [tau]_2) e(C - y G + z W, [1]_2) == 1
    const G1 B = pt(commit_lem).add(pt(g1gen).mul(Fr::from_bytes(y_mont)).neg()).add(W.mul(Fr::from_bytes(z_mont)));
    return host::pairing_eq2(W.neg(), t2, B, host::g2_gen()) ? 1 : 0;
  } catch (const std::exception&) {
    return KGS_E_ARG;
  }
}

int kgs_kzg_verify_coset(const uint8_t commit_lem[64], int nbits, int lbits, uint64_t index, const uint8_t* ys_mont,
                         const uint8_t proof_lem[64], const uint8_t* srs_g1_lem, const uint8_t tau_l_g2[128]) {
  if (!commit_lem || !ys_mont || !proof_lem || !srs_g1_lem || !tau_l_g2) return KGS_E_ARG;
  if (nbits < 0 || nbits > 28 || lbits < 0 || lbits > nbits || (index >> (nbits - lbits))) return KGS_E_ARG;
  try {
    const host::G2A t2 = host::g2_from_lem(tau_l_g2);
    if (!host::g2_on_curve(t2)) return KGS_E_ARG;
    const size_t l = (size_t)1 << lbits;
    if (!host::g1_valid(commit_lem) || !host::g1_valid(proof_lem)) return 0;
    for (size_t k = 0; k < l; k++)
      if (!host::g1_valid(srs_g1_lem + 64 * k) || !host::lt_mod(ys_mont + 32 * k, host::FR_MOD.p)) return 0;
    // J = the inverse transform of size l of y (radix-2, decimation in time, root Fr.w[lbits]^-1, times 1 / l),
    // then d_k = w^(-i k) J_k: I(X) = sum_k d_k X^k takes the value y_j at w^i psi^j
    std::vector<Fr> J(l);
    for (size_t j = 0; j < l; j++) {
      size_t b = 0;
      for (int s = 0; s < lbits; s++) b |= ((j >> s) & 1) << (lbits - 1 - s);
      J[b] = Fr::from_bytes(ys_mont + 32 * j);
    }
    const Fr pinv = host::fr_w_cached(lbits).inverse();
    for (size_t h = 1; h < l; h *= 2) {
      Fr wh = pinv;
      for (size_t k = 2 * h; k < l; k *= 2) wh = wh.sqr();
      Fr tw = Fr::one();
      for (size_t t = 0; t < h; t++) {
        for (size_t g = 0; g < l; g += 2 * h) {
          const Fr a = J[g + t], b = J[g + t + h] * tw;
          J[g + t] = a + b;
          J[g + t + h] = a - b;
        }
        tw = tw * wh;
      }
    }
    const Fr w = host::fr_w_cached(nbits);
    const Fr step = w.pow_u64(index).inverse();  // w^(-i)
    Fr f = Fr::from_u64(l).inverse();
    std::vector<uint8_t> d(32 * l);
    for (size_t k = 0; k < l; k++) {
      uint64_t s[4];
      (J[k] * f).to_std(s);
      memcpy(d.data() + 32 * k, s, 32);
      f = f * step;
    }
    const G1 I = host::g1_lincomb_segment(srs_g1_lem, d.data(), l);
    const Fr a = host::fr_w_cached(nbits - lbits).pow_u64(index);  // a_i = w^(i l)
    const G1 W = pt(proof_lem);
    // e(-W, [tau^l]_2) e(C - [I(tau)]_1 + a_i W, [1]_2) == 1
    const G1 B = pt(commit_lem).add(I.neg()).add(W.mul(a));
    return host::pairing_eq2(W.neg(), t2, B, host::g2_gen()) ? 1 : 0;
  } catch (const std::exception&) {
    return KGS_E_ARG;
  }
}

int kgs_verify_ptau(int kind, const char* ptau_path, int nbits, int npols, int selected, const uint8_t* commitments,
                    const uint8_t* evaluations) {
  uint8_t t2[128];
  int rc = kgs_ptau_read_tau_g2(ptau_path, t2);
  if (rc < 0) return rc;
  return kgs_verify(kind, nbits, npols, selected, commitments, evaluations, t2);
}

}  // extern "C"
