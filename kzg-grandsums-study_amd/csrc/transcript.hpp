// Keccak-256 Fiat-Shamir transcript exactly as src/Keccak256Transcript.js:7-53: commitments enter
// as G1.toRprUncompressed (64 B, big-endian standard x||y), scalars as Fr.toRprBE (32 B); the
// challenge is the big-endian hash reduced mod r; the buffer is cumulative (never reset).
#pragma once
#include <vector>

#include "host_field.hpp"
#include "keccak.hpp"

namespace kgs {
namespace host {

struct Transcript {
  std::vector<uint8_t> buf;
  void add_commitment(const uint8_t lem[64]) {
    uint8_t rpr[64];
    host::g1_lem_to_rpr_uncompressed(lem, rpr);
    buf.insert(buf.end(), rpr, rpr + 64);
  }
  void add_scalar(const Fr& s) {
    uint8_t be[32];
    s.to_be_std(be);
    buf.insert(buf.end(), be, be + 32);
  }
  Fr challenge() const {
    uint8_t h[32];
    host::keccak256(buf.data(), buf.size(), h);
    return Fr::from_be_reduce(h);
  }
};

// The Fiat-Shamir schedule of a proof of m >= 1 arguments, written once: what enters the transcript, in
// what order, and where each challenge is drawn (grandsum verifier.js:246-312 computeChallenges, prover.js
// rounds 2-5; the multi-argument layout in include/kgs.h). The provers call the stages as their commitments
// appear, the verifiers back to back. Commitments are 64 B affine LEM, `n` of them contiguous. A challenge is
// absorbed at the start of the stage after the one that drew it, which is the same byte stream: the buffer
// is cumulative. For m = 1 no delta is drawn and the stream is the single-argument one.
struct Schedule {
  struct BetaGamma { Fr beta, gamma; };    // beta = 0 unless some argument has k > 1
  struct AlphaDelta { Fr alpha, delta; };  // delta = 1 for one argument

  BetaGamma after_round1(const uint8_t* coms, int ncom, bool any_vec) {
    absorb(coms, ncom);
    Fr beta = Fr::zero();
    if (any_vec) {
      beta = tr.challenge();
      tr.add_scalar(beta);
    }
    return {beta, draw()};
  }
  AlphaDelta after_round2(const uint8_t* S_coms, int m) {
    tr.add_scalar(last);
    absorb(S_coms, m);
    const Fr alpha = draw();
    if (m == 1) return {alpha, Fr::one()};
    tr.add_scalar(alpha);
    return {alpha, draw()};
  }
  Fr after_round3(const uint8_t* Q) {
    tr.add_scalar(last);
    absorb(Q, 1);
    return draw();
  }
  Fr after_round4(const Fr* evals, size_t nev) {
    tr.add_scalar(last);
    for (size_t i = 0; i < nev; i++) tr.add_scalar(evals[i]);
    return draw();
  }
  Fr after_round5(const uint8_t* Wxi, const uint8_t* Wxiw) {
    tr.add_scalar(last);
    absorb(Wxi, 1);
    absorb(Wxiw, 1);
    return draw();
  }

 private:
  Transcript tr;
  Fr last = Fr::zero();  // the challenge drawn last: the next stage absorbs it first
  void absorb(const uint8_t* coms, int n) {
    for (int i = 0; i < n; i++) tr.add_commitment(coms + 64 * (size_t)i);
  }
  Fr draw() { return last = tr.challenge(); }
};

}  // namespace host
}  // namespace kgs
