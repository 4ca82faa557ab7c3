// The cross-rank host arithmetic of the distributed prover (prover_dist.cpp): what each rank computes
// from all-gathered values between its kernel launches, and what decides whether W ranks produce the
// proof one GPU would. Host field only, so every rule is checked alone on a CPU
// (tests/native/dist_math_check.cpp). W ranks; rank r; gathered vectors are rank-major.
#pragma once
#include <stdint.h>
#include <vector>

#include "host_field.hpp"

namespace kgsi {
using kgs::host::Fr;

// Round 2: the builder scans each rank's BLOCK alone; tot[j] is rank j's local total (sum, or product for
// a grand-product: gs = false). off: what rank r's block starts from (the totals before it); next: S at the
// natural index following the block, the unit for the last rank (the wrap, index n -> 0); all: the total
// over all ranks, which must be the unit.
struct ScanOffsets {
  Fr off, next, all;
};
inline ScanOffsets scan_offsets(const std::vector<Fr>& tot, int r, bool gs) {
  const int W = (int)tot.size();
  const Fr unit = gs ? Fr::zero() : Fr::one();
  Fr off = unit, all = unit, next = unit;
  for (int j = 0; j < W; j++) {
    if (j < r) off = gs ? off + tot[j] : off * tot[j];
    if (j <= r) next = gs ? next + tot[j] : next * tot[j];
    all = gs ? all + tot[j] : all * tot[j];
  }
  if (r == W - 1) next = unit;  // S at the wrap (natural index n -> 0)
  return {off, next, all};
}

// Round 3's quotient halo. In the E layout rank r holds, for every k1 < W, block k1 of the coset
// evaluations; the global order of the blocks is (k1, r) -> k1 * W + r. The quotient at the end of block k1
// reads the head of the block that follows it: the same k1 on rank r + 1, or for the last rank block
// k1 + 1 (cyclically) on rank 0. blk is the block index on rank src.
struct HaloSource {
  int src, blk;
};
inline HaloSource halo_source(int r, int W, int k1) {
  return r + 1 < W ? HaloSource{r + 1, k1} : HaloSource{0, (k1 + 1) % W};
}

// Round 4: rank j evaluated its CYCLIC slices p_j(Y) = sum_i a_(j + W i) Y^i at Y = x^W, so
// p(x) = sum_j x^j p_j(x^W). allv holds np values per rank: np - 1 polynomials at xi^W, then S at (xi w)^W.
inline void horner_combine(const std::vector<Fr>& allv, size_t np, int W, const Fr& xi, const Fr& xiw, std::vector<Fr>& ev1,
                           Fr& sxiw) {
  ev1.assign(np - 1, Fr::zero());
  sxiw = Fr::zero();
  Fr xr = Fr::one(), xwr = Fr::one();
  for (int j = 0; j < W; j++) {
    for (size_t p = 0; p + 1 < np; p++) ev1[p] = ev1[p] + xr * allv[j * np + p];
    sxiw = sxiw + xwr * allv[j * np + np - 1];
    xr = xr * xi;
    xwr = xwr * xiw;
  }
}

// Round 5: each rank divides its BLOCK of `len` coefficients by (X - z) with a zero carry-in
// (Polynomial.divByXSubValue, polynomial.js:814-851, block by block); Rl[2 j + which] is block j's value
// at z. Carries from the top rank down: c_{W-1} = 0, c_{j-1} = R_lo(j) + z^len c_j. `mine` receives rank
// r's carry-in; returns r_0, the remainder, which must be zero.
inline Fr division_carries(const std::vector<Fr>& Rl, int which, const Fr& z, uint64_t len, int W, int r, Fr& mine) {
  const Fr zl = z.pow_u64(len);
  Fr cr = Fr::zero();
  for (int j = W - 1; j >= 0; j--) {
    if (j == r) mine = cr;
    cr = Rl[2 * j + which] + zl * cr;
  }
  return cr;
}

}  // namespace kgsi
