// Stand-alone check of the distributed prover's cross-rank host arithmetic (csrc/dist_math.hpp), built by
// tests/native/Makefile under -fsanitize=address,undefined and run by tests/test_host_sanitizers.py
// (TEST INFRASTRUCTURE). Every W in {1, 2, 4, 8}, seeded random Fr values:
//   scan_offsets      against a sequential prefix over the concatenated blocks, sum and product, with a
//                     total that is not the unit and with one that is; the last rank's wrap value
//   division_carries  a polynomial of W L coefficients (L in {1, 3, 8}) divided block by block with a zero
//                     carry-in, the carries applied as k_div_fix does, against the synthetic division of the
//                     whole polynomial by (X - z); r_0 zero exactly when z is a root ((X - z) g, and the
//                     same with one coefficient changed)
//   horner_combine    against direct evaluation of the interleaved polynomials
//   halo_source       against "the block following block k1 of rank r in the E layout", enumerated
// Exit status 0: every check held; 1: a mismatch (named on stderr).
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../kzg-grandsums-study_amd/csrc/dist_math.hpp"

using namespace kgsi;

namespace {

int g_failures = 0;
void fail(const char* what, int W, int a, int b) {
  fprintf(stderr, "dist_math_check: %s: W %d, case %d / %d\n", what, W, a, b);
  g_failures++;
}

uint64_t g_state = 20261020;
uint64_t rnd64() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
Fr rnd_fr() {
  uint64_t s[4] = {rnd64(), rnd64(), rnd64(), rnd64() >> 4};  // < 2^252 < r
  return Fr::from_std(s);
}
std::vector<Fr> rnd_vec(size_t n) {
  std::vector<Fr> v(n);
  for (Fr& x : v) x = rnd_fr();
  return v;
}
Fr eval(const std::vector<Fr>& p, const Fr& x) {
  Fr a = Fr::zero();
  for (size_t i = p.size(); i-- > 0;) a = a * x + p[i];
  return a;
}

void check_scan(int W) {
  const int L = 3;
  for (int gs = 0; gs < 2; gs++)
    for (int unit_total = 0; unit_total < 2; unit_total++) {
      const Fr unit = gs ? Fr::zero() : Fr::one();
      auto op = [&](const Fr& a, const Fr& b) { return gs ? a + b : a * b; };
      std::vector<Fr> v = rnd_vec((size_t)W * L);
      if (unit_total) {  // the last element makes the total the unit
        Fr rest = unit;
        for (size_t i = 0; i + 1 < v.size(); i++) rest = op(rest, v[i]);
        v.back() = gs ? rest.neg() : rest.inverse();
      }
      std::vector<Fr> tot(W, unit), prefix(1, unit);  // prefix[i]: the sequential scan before element i
      for (size_t i = 0; i < v.size(); i++) {
        tot[i / L] = op(tot[i / L], v[i]);
        prefix.push_back(op(prefix.back(), v[i]));
      }
      for (int r = 0; r < W; r++) {
        const ScanOffsets so = scan_offsets(tot, r, gs != 0);
        if (!(so.off == prefix[(size_t)r * L])) fail("scan_offsets off", W, gs, r);
        if (!(so.all == prefix.back()) || (so.all == unit) != (unit_total != 0)) fail("scan_offsets all", W, gs, r);
        // next: the scan at the first index past the block; past the last block that is index 0 again
        if (r + 1 < W ? !(so.next == prefix[(size_t)(r + 1) * L]) : !(so.next == unit)) fail("scan_offsets next", W, gs, r);
        if (unit_total && !(so.next == prefix[(size_t)(r + 1) * L])) fail("scan_offsets wrap", W, gs, r);
      }
    }
}

// synthetic division by (X - z) of a[0 .. len) with carry-in zero: q[i - 1] = r_i, q[len - 1] = 0,
// r_i = a_i + z r_(i + 1); returns r_0 (poly.hip k_div_finish)
Fr divide_block(const Fr* a, size_t len, const Fr& z, Fr* q) {
  Fr r = Fr::zero();
  q[len - 1] = Fr::zero();
  for (size_t i = len; i-- > 0;) {
    r = a[i] + z * r;
    if (i >= 1) q[i - 1] = r;
  }
  return r;
}

void check_division_of(int W, int L, const std::vector<Fr>& p, const Fr& z, bool root, int tag) {
  const size_t n = (size_t)W * L;
  std::vector<Fr> want(n), got(n), Rl(2 * W, Fr::zero());
  const Fr rem = divide_block(p.data(), n, z, want.data());
  for (int which = 0; which < 2; which++) {  // both slots of the gathered pair
    for (int j = 0; j < W; j++) Rl[2 * j + which] = divide_block(p.data() + (size_t)j * L, L, z, got.data() + (size_t)j * L);
    for (int r = 0; r < W; r++) {
      Fr carry = Fr::one();  // overwritten
      const Fr r0 = division_carries(Rl, which, z, (uint64_t)L, W, r, carry);
      if (!(r0 == rem) || r0.is_zero() != root) fail("division_carries r_0", W, L, tag);
      // dist.hip k_div_fix: q[j] += z^(L - 1 - j) c
      Fr zp = Fr::one();
      for (int j = L - 1; j >= 0; j--) {
        got[(size_t)r * L + j] = got[(size_t)r * L + j] + zp * carry;
        zp = zp * z;
      }
    }
    for (size_t i = 0; i < n; i++)
      if (!(got[i] == want[i])) {
        fail("division_carries quotient", W, L, tag);
        break;
      }
  }
}

void check_division(int W) {
  const int Ls[3] = {1, 3, 8};
  for (int L : Ls) {
    const size_t n = (size_t)W * L;
    const Fr z = rnd_fr();
    const std::vector<Fr> p = rnd_vec(n);
    check_division_of(W, L, p, z, eval(p, z).is_zero(), 0);
    // (X - z) g with deg g = n - 2, then one coefficient changed
    std::vector<Fr> g = rnd_vec(n - 1), m(n, Fr::zero());
    for (size_t i = 0; i + 1 < n; i++) {
      m[i + 1] = m[i + 1] + g[i];
      m[i] = m[i] - z * g[i];
    }
    check_division_of(W, L, m, z, true, 1);
    const size_t at = rnd64() % n;
    m[at] = m[at] + Fr::one();  // the value at z becomes z^at: never zero
    check_division_of(W, L, m, z, false, 2);
  }
}

void check_horner(int W) {
  const int L = 3;
  const size_t np = 4;
  const Fr xi = rnd_fr(), xiw = xi * rnd_fr();
  std::vector<std::vector<Fr>> polys;
  for (size_t p = 0; p < np; p++) polys.push_back(rnd_vec((size_t)W * L));
  const Fr xW = xi.pow_u64(W), xwW = xiw.pow_u64(W);
  std::vector<Fr> allv((size_t)W * np);
  for (int j = 0; j < W; j++)
    for (size_t p = 0; p < np; p++) {
      std::vector<Fr> slice(L);  // rank j's CYCLIC slice: coefficients j + W i
      for (int i = 0; i < L; i++) slice[i] = polys[p][(size_t)j + (size_t)W * i];
      allv[j * np + p] = eval(slice, p + 1 < np ? xW : xwW);
    }
  std::vector<Fr> ev1;
  Fr sxiw;
  horner_combine(allv, np, W, xi, xiw, ev1, sxiw);
  if (ev1.size() != np - 1) fail("horner_combine size", W, 0, 0);
  for (size_t p = 0; p + 1 < np && p < ev1.size(); p++)
    if (!(ev1[p] == eval(polys[p], xi))) fail("horner_combine at xi", W, (int)p, 0);
  if (!(sxiw == eval(polys[np - 1], xiw))) fail("horner_combine at xi w", W, 0, 0);
}

void check_halo(int W) {
  // E layout: block k1 of rank r is the (k1 W + r)-th of the W^2 blocks; the order is cyclic
  for (int r = 0; r < W; r++)
    for (int k1 = 0; k1 < W; k1++) {
      const int next = (k1 * W + r + 1) % (W * W);
      const HaloSource hs = halo_source(r, W, k1);
      if (hs.src != next % W || hs.blk != next / W) fail("halo_source", W, r, k1);
    }
}

}  // namespace

int main() {
  const int Ws[4] = {1, 2, 4, 8};
  for (int W : Ws) {
    check_scan(W);
    check_division(W);
    check_horner(W);
    check_halo(W);
  }
  printf("dist_math_check %s (%d mismatches)\n", g_failures ? "FAILED" : "ok", g_failures);
  return g_failures ? 1 : 0;
}
