// BN254 Fr products in 9 x 29-bit limbs for the NTT twiddle multiplications (device only).
//
// The NTT keeps its elements as 8 x 32-bit words (field.hpp `fr`, values in [0, 4p) lazily reduced,
// canonical at every pass boundary) and only its twiddle products go through this header. The 8 x 32
// product-scanning product (fr::mul_nored) is ONE dependent chain: every v_mad_u64_u32 reads the
// previous one's 64-bit sum and every mad needs a v_addc for the column's carry word (2 VALU per
// partial product). Here a CIOS product in 29-bit limbs takes one mad per partial product into 64-bit
// column accumulators with no carry words (a column's 9 products and 8 reduction terms stay below 2^64), and the 9
// columns are 9 independent chains: the same issue cycles for fewer instructions (~230 against ~300),
// and far more instruction-level parallelism for the NTT passes, which run at 2-3 waves per SIMD.
// The twiddle w comes pre-converted from the domain tables (ntt.hip k_tw29): w * 2^261 mod p,
// canonical, as 9 limbs in a 10-word record, so the product a * w * 2^261 * 2^-261 lands in the same
// Montgomery domain (R = 2^256) as a. Same reduction scheme as field29.hpp's fq29: rows 0..6 reduce by
// R* = k*r = -1 mod 2^32 (m is the column's low word, no multiply; r29::QSTAR_R), row 7 takes the
// 32-bit m = -t0/P[0] mod 2^32 (BN254's r is 1 + 2^28 mod 2^29, so -P[0]^-1 mod 2^32 is 2^28 - 1),
// row 8 the 29-bit m; one carry mad per row. Bounds (tests/test_fr29_qstar.py re-derives them and runs
// the exact row schedule on Python integers; tests/test_fr29.py does so for the rows without R*,
// KGS_QSTAR_ROWS_FR = 0: columns < 2^63.14): for a < 2^256 (unpacked limbs < 2^29, top limb < 2^24) and
// w < p, every column stays < 2^63.63 (the m * QSTAR_R[j] terms dominate) and the result is
// < a*w/2^261 + p(1 + 2^-22) < 1.04 p < 2p.
#pragma once
#include "field.hpp"

// Leading CIOS rows of mul29 that reduce by R* = k*r = -1 mod 2^32 (no multiply for m, see below); at
// most 7 (bounds: tests/test_fr29_qstar.py); 0 builds the parent's rows for A/B
#ifndef KGS_QSTAR_ROWS_FR
#define KGS_QSTAR_ROWS_FR 7
#endif
static_assert(KGS_QSTAR_ROWS_FR <= 7, "value and column bounds of mul29's R* rows");

namespace kgs {
namespace r29 {
constexpr uint32_t MASK = 0x1fffffffu;
constexpr uint32_t P[9] = {0x10000001u, 0x1f0fac9fu, 0x0e5c2450u, 0x07d090f3u, 0x1585d283u,
                           0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu};  // r, 29-bit limbs
constexpr uint32_t INV = 0x0fffffffu;    // -r^-1 mod 2^29
constexpr uint32_t INV32 = 0x0fffffffu;  // -P[0]^-1 mod 2^32
// R* = QSTAR_K * r = (2^32 - 1) + 2^29 * s with QSTAR_K = -r^-1 mod 2^32 (s a multiple of 8 below
// 2^257). QSTAR_R holds s's nine 29-bit limbs with 8 added to limb 0. A row that reduces by R* takes
// m = t0's low word as it is: t0 + m (2^32 - 1) = (hi32(t0) + m) 2^32, so column 0 vanishes, its carry
// into column 1 is 8 hi32(t0) + 8 m (the 8 m rides on m * QSTAR_R[0]), and m * s lands on columns
// 1..9: nine mads and the carry mad, 10 VOP3 against the 11 of a 32-bit-m row (same scheme as
// field29.hpp's fq29::reduce_row_qstar). Row i adds < 2^(32 + 29 i) R* / 2^261 to the result: rows
// 0..6 together < 2^-23 r.
constexpr uint32_t QSTAR_K = 0xefffffffu;
constexpr uint32_t QSTAR_R[9] = {0x08f05368u, 0x1a996a5bu, 0x13e27f6bu, 0x15166c9eu, 0x1e906a17u,
                                 0x04c58463u, 0x16877334u, 0x0b82ba37u, 0x016af04cu};
constexpr int W29_WORDS = 10;            // twiddle record: 9 limbs + 1 pad (kernels.hpp TW29_WORDS)
// 32 * 2^256 mod r in 8 x 32-bit words (Montgomery form of 32): x * C32 turns x * 2^256 into x * 2^261
constexpr uint32_t C32[8] = {0x8fffff57u, 0x2fd4e156u, 0xa494b01au, 0x75bba827u,
                             0x819caa80u, 0x5301fa84u, 0x563d4475u, 0x0dc83629u};
// record of R^2 (2^517 mod r, 29-bit limbs): mul29(x, TO_MONT) = x * 2^256 mod r, the Montgomery form
constexpr uint32_t TO_MONT[9] = {0x142db4dfu, 0x19d6990eu, 0x1472f48cu, 0x06dbe7e3u, 0x0b84d579u,
                                 0x10f9faf7u, 0x121f4380u, 0x17a112deu, 0x001275c7u};
}  // namespace r29

struct W29 {
  uint32_t l[9];
};

__device__ __forceinline__ W29 w29_load(const uint32_t* p) {
  const uint4 a = *reinterpret_cast<const uint4*>(p);
  const uint4 b = *reinterpret_cast<const uint4*>(p + 4);
  W29 w;
  w.l[0] = a.x; w.l[1] = a.y; w.l[2] = a.z; w.l[3] = a.w;
  w.l[4] = b.x; w.l[5] = b.y; w.l[6] = b.z; w.l[7] = b.w;
  w.l[8] = p[8];
  return w;
}

// 8 x 32-bit words (value < 2^256) -> 9 x 29-bit limbs, same value
__device__ __forceinline__ void unpack29(const fr& a, uint32_t (&l)[9]) {
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const int bit = 29 * j, i = bit >> 5, s = bit & 31;
    uint32_t x = a.v[i] >> s;
    if (s > 3 && i + 1 < 8) x |= a.v[i + 1] << (32 - s);
    l[j] = x & r29::MASK;
  }
}

// a * w * 2^-261 mod p, in [0, 2p), for a < 2^256 (any representative) and w = a twiddle record
__device__ __forceinline__ fr mul29(const fr& A, const W29& w) {
  uint32_t a[9];
  unpack29(A, a);
  // SGPR operands the compiler cannot fold: the row carry (x 8) and m * P[0] (P[0] = 2^28 + 1) stay
  // single v_mad_u64_u32s instead of 64-bit shift-and-add sequences
  uint32_t eight = 8, p0 = r29::P[0];
  asm volatile("" : "+s"(eight), "+s"(p0));
  uint64_t t[9];
#pragma unroll
  for (int j = 0; j < 9; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
#pragma unroll
    for (int j = 0; j < 9; j++) t[j] = (uint64_t)a[i] * w.l[j] + t[j];
    if (i < KGS_QSTAR_ROWS_FR) {  // reduce by R*: m = lo32(t0), no multiply
      const uint32_t m = (uint32_t)t[0], h = (uint32_t)(t[0] >> 32);
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = (uint64_t)m * r29::QSTAR_R[j] + t[j + 1];
      t[8] = (uint64_t)m * r29::QSTAR_R[8];
      t[0] = (uint64_t)h * eight + t[0];
    } else if (i < 8) {  // 32-bit m: t0 + m P0 has 32 zero low bits, its carry is 8 x its high word
      const uint32_t m = (uint32_t)t[0] * r29::INV32;
      const uint64_t u = (uint64_t)m * p0 + t[0];
#pragma unroll
      for (int j = 1; j < 9; j++) t[j] = (uint64_t)m * r29::P[j] + t[j];
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = t[j + 1];
      t[0] = (uint64_t)(uint32_t)(u >> 32) * eight + t[0];
      t[8] = 0;
    } else {  // 29-bit m in the last row
      const uint32_t m = ((uint32_t)t[0] * r29::INV) & r29::MASK;
      const uint64_t c = ((uint64_t)m * p0 + t[0]) >> 29;
#pragma unroll
      for (int j = 1; j < 9; j++) t[j] = (uint64_t)m * r29::P[j] + t[j];
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = t[j + 1];
      t[0] += c;
      t[8] = 0;
    }
  }
  uint32_t l[9];
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const uint64_t s = t[j] + c;
    l[j] = j < 8 ? ((uint32_t)s & r29::MASK) : (uint32_t)s;
    c = s >> 29;
  }
  fr r;  // value < 2p < 2^255: pack the limbs into 8 words
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int bit = 32 * i, j = bit / 29, s = bit % 29;
    uint32_t x = l[j] >> s;
    if (j + 1 < 9) x |= l[j + 1] << (29 - s);
    if (s > 26 && j + 2 < 9) x |= l[j + 2] << (58 - s);
    r.v[i] = x;
  }
  return r;
}

}  // namespace kgs
