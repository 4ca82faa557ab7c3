// Number-theoretic transform over G1 for gfx950 — [ffjs] `G1.fft` / `G1.ifft` (kgs.h kgs_g1_ntt; DESIGN.md §18;
// the entry points and the Lagrange-basis cache are in g1_ntt.cpp).
//
// Radix-2 decimation in time, natural order in and out: the first stage gathers its operands
// bit-reversed from the input, stage `h` (half-width 1, 2, .., n/2) computes
//   (a, b) -> (a + w b, a - w b),  w = omega_{2h}^t = omega_n^{t n / 2h},  t < h
// on the pairs (g 2h + t, g 2h + t + h) of its G = n / 2h groups. A butterfly is one 254-bit scalar
// multiplication and two additions for 256 B of traffic, so the stages are plain global-memory kernels,
// one butterfly per thread; all the time is in the (n/2) log2 n twiddle multiplications.
//   * The points are affine between the stages (launch_batch_affine after every stage: ~20 field
//     products per point against ~3000 per butterfly): the multiplication then adds an affine b
//     (madd, 10 products) instead of an XYZZ one (14), and so do the two additions to the affine a.
//   * The twiddles are signed digits (NAF, digits of 3k - k): a third of the bits carry an addition
//     instead of half. A record is 16 words, the masks of the +1 and of the -1 digits, built once per
//     call by k_g1ntt_twiddles; the double-and-add loop negates b's y for a -1.
//   * Twiddle index 0 (every stage; all of stage h = 1) is a copy, not a multiplication. With t < h no
//     twiddle is omega^(n/2) = -1: that negation is the `a - w b` output.
//   * Thread mapping. Per lane: thread i -> (g, t) = (i / h, i % h), adjacent lanes adjacent points, 64
//     twiddles per wave: the `if (digit) add` diverges and every lane pays every addition. Per wave:
//     (t, g) = (i / G, i % G), possible when G >= 64: the wave's 64 butterflies share t, the digits sit in
//     scalar registers and the schedule is uniform, as k_tab_scale's is for rho (msm.hip).
//   * The inverse transform's 1/n (kgs_srs_lagrange: 2^256 / n, which also takes rho = 2^-256 off the
//     table row) is one more multiplication per point by a launch-uniform constant, k_g1ntt_scale.
//   * Many transforms of one size side by side (kgs_kzg_open_cosets_many): k_g1ntt_stage_many runs
//     a stage of all of them in one launch; a wave then shares t across polynomials and groups (g1ntt_map.hpp), so
//     a small transform, whose stages have fewer than 64 groups, still gets a wave-uniform record.
#include "kernels.hpp"
#include "g1ntt_map.hpp"

namespace kgs {

static inline unsigned nb(uint64_t work, unsigned bs = 256) { return (unsigned)((work + bs - 1) / bs); }

struct G1NttWords {
  uint32_t w[8];
};

// the NAF of k < 2^254 as two masks: digit i is +1 if bit i of pos, -1 if bit i of neg (i <= 254)
__device__ __forceinline__ void naf_record(const uint32_t k[8], uint32_t* __restrict__ rec) {
  uint32_t k3[8];
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {  // 3k = 2k + k
    const uint32_t two = (k[i] << 1) | (i ? k[i - 1] >> 31 : 0u);
    const uint64_t s = (uint64_t)two + k[i] + carry;
    k3[i] = (uint32_t)s;
    carry = (uint32_t)(s >> 32);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t p = k3[i] & ~k[i], n = k[i] & ~k3[i];
    const uint32_t pn = i < 7 ? k3[i + 1] & ~k[i + 1] : 0u, nn = i < 7 ? k[i + 1] & ~k3[i + 1] : 0u;
    rec[i] = (p >> 1) | (pn << 31);
    rec[8 + i] = (n >> 1) | (nn << 31);
  }
}

// rec[i] = NAF record of the standard form of root^i, i < count; rec[count] = that of `scale`
// (standard form, < r). root: Montgomery words.
__global__ void __launch_bounds__(256) k_g1ntt_twiddles(uint32_t* __restrict__ rec, uint64_t count, G1NttWords root,
                                                        G1NttWords scale) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > count) return;
  uint32_t k[8];
  if (i == count) {
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = scale.w[j];
  } else {
    fr b, x = fr::one();
#pragma unroll
    for (int j = 0; j < 8; j++) b.v[j] = root.w[j];
    for (uint64_t e = i; e; e >>= 1) {
      if (e & 1) x = x * b;
      b = b.sqr();
    }
    x = x.from_mont();
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = x.v[j];
  }
  naf_record(k, rec + G1NTT_TW_WORDS * i);
}

// k * b for the record at rec. UNI: the record is the same for the whole wave.
template <bool UNI>
__device__ __forceinline__ g1_xyzz g1ntt_mul(const g1_aff& b, const uint32_t* __restrict__ rec) {
  g1_xyzz r = g1_xyzz::inf();
  if (b.is_inf()) return r;
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    uint32_t p = rec[w], n = rec[8 + w];
    if (UNI) {
      p = __builtin_amdgcn_readfirstlane(p);
      n = __builtin_amdgcn_readfirstlane(n);
    }
#pragma unroll 1
    for (int k = 31; k >= 0; k--) {
      r = r.dbl();
      const uint32_t m = 1u << k;
      if ((p | n) & m) {
        g1_aff s = b;
        if (n & m) s.y = s.y.neg();
        r.add_aff(s);
      }
    }
  }
  return r;
}

// One stage: out_xyzz[pa], out_xyzz[pb] = a + w b, a - w b. half_n = n / 2 butterflies, h = 2^logh.
// bitrev_in: the operands are read from in_aff at the bit-reversed positions (the first stage).
template <bool UNI>
__global__ void __launch_bounds__(64) k_g1ntt_stage(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ in_aff,
                                                    const uint32_t* __restrict__ tw, uint64_t half_n, int logh, int logn,
                                                    int bitrev_in) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= half_n) return;
  const int logG = logn - 1 - logh;
  uint32_t t, g;
  if (UNI) {  // logG >= 6 and 64-thread blocks: one t per wave
    t = __builtin_amdgcn_readfirstlane((uint32_t)(i >> logG));
    g = (uint32_t)i & ((1u << logG) - 1u);
  } else {
    g = (uint32_t)(i >> logh);
    t = (uint32_t)i & ((1u << logh) - 1u);
  }
  const uint64_t pa = ((uint64_t)g << (logh + 1)) + t, pb = pa + ((uint64_t)1 << logh);
  uint64_t sa = pa, sb = pb;
  if (bitrev_in) {
    sa = __brev((uint32_t)pa) >> (32 - logn);
    sb = __brev((uint32_t)pb) >> (32 - logn);
  }
  const g1_aff a = g1_aff::load(in_aff + 16 * sa), b = g1_aff::load(in_aff + 16 * sb);
  g1_xyzz T;
  if (t == 0)
    T = g1_xyzz::from_aff(b);
  else
    T = g1ntt_mul<UNI>(b, tw + G1NTT_TW_WORDS * ((uint64_t)t << logG));
  g1_xyzz U = T;
  U.Y = U.Y.neg();
  T.add_aff(a);
  U.add_aff(a);
  T.store(out_xyzz + 32 * pa);
  U.store(out_xyzz + 32 * pb);
}

// One stage of `polys` transforms of size 2^logn side by side, transform p over the points
// [p n, (p + 1) n) of in_aff / out_xyzz, all with the one twiddle table of their size. The butterfly is
// k_g1ntt_stage's; the lanes come from g1ntt_map.hpp. UNI: a block's 64 lanes share t across polynomials and
// groups (polys * G >= 64), the record is wave-uniform whatever G is. Grid: g1ntt_many_blocks.
template <bool UNI>
__global__ void __launch_bounds__(64) k_g1ntt_stage_many(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ in_aff,
                                                         const uint32_t* __restrict__ tw, uint64_t polys, int logh, int logn,
                                                         int bitrev_in) {
  KGS_AUX_PRIO();
  const G1NttBfly m = g1ntt_many_map(blockIdx.x, threadIdx.x, polys, logn, logh, UNI);
  if (!m.active) return;
  uint64_t sa = m.pa, sb = m.pb;
  if (bitrev_in) {  // within the polynomial's own block
    const uint64_t base = m.poly << logn;
    sa = base + (__brev((uint32_t)(m.pa - base)) >> (32 - logn));
    sb = base + (__brev((uint32_t)(m.pb - base)) >> (32 - logn));
  }
  const g1_aff a = g1_aff::load(in_aff + 16 * sa), b = g1_aff::load(in_aff + 16 * sb);
  g1_xyzz T;
  if (m.t == 0)
    T = g1_xyzz::from_aff(b);
  else
    T = g1ntt_mul<UNI>(b, tw + G1NTT_TW_WORDS * m.tw);
  g1_xyzz U = T;
  U.Y = U.Y.neg();
  T.add_aff(a);
  U.add_aff(a);
  T.store(out_xyzz + 32 * m.pa);
  U.store(out_xyzz + 32 * m.pb);
}

// out_xyzz[i] = k * in_aff[i] for the one record at rec
__global__ void __launch_bounds__(64) k_g1ntt_scale(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ in_aff,
                                                    const uint32_t* __restrict__ rec, uint64_t n) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1ntt_mul<true>(g1_aff::load(in_aff + 16 * i), rec).store(out_xyzz + 32 * i);
}

// out_xyzz[i] = k_i * in_aff[i], the scalar k_i = sc[8 i ..] another one in every lane (the pointwise
// product of kgs_kzg_open_all, kgs_g1_mul_each). REDUCE: k_i is any 256-bit integer and is
// taken mod r here (at most five subtractions); otherwise k_i < r as the Fr kernels leave it. The NAF
// record is made in registers and shifted up one digit per doubling, so no digit is indexed at run
// time and nothing goes to scratch or to a record buffer (130 VGPRs). The lanes of a wave share no digit:
// the wave pays an addition wherever one of its lanes has one, which with 64 independent scalars is
// nearly every one of the 254 positions, against ~85 for a shared record: 254 (9 + 10) field products
// against 254 * 9 + 85 * 10, a factor 1.54 (measured 1.57 at 2^21 points). The record in
// LDS instead (120 VGPRs, four waves per SIMD instead of three) measured the same time: the loop is bound
// by the VALU, not by latency.
// MANY (kgs_kzg_open_cosets_many): the n terms are rows of `cols` scalars, the points rows of
// pcols = 2^k <= cols: term (r, c) takes point (r, c mod pcols), the cached point every polynomial shares.
template <bool REDUCE, bool MANY = false>
__global__ void __launch_bounds__(64) k_g1_mul_each(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ in_aff,
                                                    const uint32_t* __restrict__ sc, uint64_t n, uint64_t cols,
                                                    uint64_t pcols) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t pi = i;
  if (MANY) {
    const uint64_t r = i / cols;
    pi = r * pcols + ((i - r * cols) & (pcols - 1));
  }
  fr k = fr::load(sc + 8 * i);
  if (REDUCE) {
#pragma unroll 1
    for (int t = 0; t < 5; t++) k = fr::reduce_once(k);  // 2^256 < 6 r
  }
  uint32_t rec[G1NTT_TW_WORDS];
  naf_record(k.v, rec);
  const g1_aff b = g1_aff::load(in_aff + 16 * pi);
  g1_xyzz r = g1_xyzz::inf();
  if (!b.is_inf()) {
#pragma unroll 1
    for (int d = 0; d < 256; d++) {
      r = r.dbl();
      const uint32_t p = rec[7] >> 31, m = rec[15] >> 31;
#pragma unroll
      for (int w = 7; w > 0; w--) {
        rec[w] = (rec[w] << 1) | (rec[w - 1] >> 31);
        rec[8 + w] = (rec[8 + w] << 1) | (rec[8 + w - 1] >> 31);
      }
      rec[0] <<= 1;
      rec[8] <<= 1;
      if (p | m) {
        g1_aff s = b;
        if (m) s.y = s.y.neg();
        r.add_aff(s);
      }
    }
  }
  r.store(out_xyzz + 32 * i);
}

// out_xyzz[g cols + i] = sum_{j < L} k[(g L + j) cols + i] * in_aff[(g L + j) cols + i]: L rows of a column per
// lane, sharing the 254 doublings (Straus): 254 (9 + 10 L) field products for L terms against
// 254 * 19 L. L records do not fit in registers beside the accumulator, so each lane keeps its records in a
// column of LDS of its own (word-major: lane = bank, no conflicts, no barrier) and reloads a base from global
// memory at each addition. The last group of a column may hold fewer than L rows. L = 2 ships: 99 VGPRs, 8 KiB
// of LDS per block, four waves per SIMD, no scratch; 62.4 ms against 79.8 ms for one row per lane at 2^21 terms
// in 64 rows. L = 4 (16 KiB, three waves) measured 63.6 ms and was dropped. Half the threads doing twice the
// work each lose where the launch is latency-bound (6.5 ms against 4.0 ms at 2^13 terms, 5.9 against 6.2 at
// 2^17): launch_g1_mul_sum takes this kernel from G1_MUL_GROUP_MIN_TERMS terms on.
// MANY: as k_g1_mul_each's, the point of term (r, i) is in_aff[r pcols + i mod pcols].
template <int L, bool REDUCE, bool MANY = false>
__global__ void __launch_bounds__(64) k_g1_mul_group(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ in_aff,
                                                     const uint32_t* __restrict__ sc, uint64_t rows, uint64_t cols,
                                                     uint64_t ngroups, uint64_t pcols) {
  KGS_AUX_PRIO();
  __shared__ uint32_t recs[L][G1NTT_TW_WORDS][64];
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ngroups * cols) return;
  const uint64_t g = t / cols, i = t - g * cols;
  const uint64_t pc = MANY ? pcols : cols, pi = MANY ? i & (pcols - 1) : i;  // the point rows' width, the column there
  const uint32_t lane = threadIdx.x;
  uint32_t live = 0;  // bit j: row g L + j exists and its point is not the identity
#pragma unroll 1
  for (int j = 0; j < L; j++) {
    const uint64_t r = g * L + j;
    if (r >= rows) break;
    fr k = fr::load(sc + 8 * (r * cols + i));
    if (REDUCE) {
#pragma unroll 1
      for (int s = 0; s < 5; s++) k = fr::reduce_once(k);  // 2^256 < 6 r
    }
    uint32_t rec[G1NTT_TW_WORDS];
    naf_record(k.v, rec);
#pragma unroll
    for (int w = 0; w < G1NTT_TW_WORDS; w++) recs[j][w][lane] = rec[w];
    if (!g1_aff::load(in_aff + 16 * (r * pc + pi)).is_inf()) live |= 1u << j;
  }
  g1_xyzz acc = g1_xyzz::inf();
  if (live) {
#pragma unroll 1
    for (int d = 255; d >= 0; d--) {
      acc = acc.dbl();
      const int w = d >> 5, bit = d & 31;
#pragma unroll 1
      for (int j = 0; j < L; j++) {
        if (!((live >> j) & 1u)) continue;
        const uint32_t p = (recs[j][w][lane] >> bit) & 1u, m = (recs[j][8 + w][lane] >> bit) & 1u;
        if (p | m) {
          g1_aff s = g1_aff::load(in_aff + 16 * ((g * L + j) * pc + pi));
          if (m) s.y = s.y.neg();
          acc.add_aff(s);
        }
      }
    }
  }
  acc.store(out_xyzz + 32 * (g * cols + i));
}

// The column sums of kgs_g1_mul_sum / kgs_kzg_open_cosets over the rows x cols products
// k_g1_mul_each left in xyzz, in place and by eights: of the rows that are still live (the multiples of
// `stride`) thread (g, i) adds rows (8 g + j) stride, j < 8, of column i into row 8 g stride, its group's
// first, which no other thread reads or writes; the next pass runs with 8 stride, and row 0 ends as the
// sum. Adjacent lanes take adjacent columns. The terms of a column may be equal (equal rows of the SRS side
// under equal coefficients), opposite or the identity: g1_xyzz::add branches on all three. Against the 254
// doublings and ~254 additions per term in k_g1_mul_each this is one addition per term, under 1 % of the
// products.
constexpr int G1_SUM_FAN = 8;
__global__ void __launch_bounds__(64) k_g1_col_sum(uint32_t* __restrict__ xyzz, uint64_t rows, uint64_t cols, uint64_t stride,
                                                   uint64_t ngroups) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ngroups * cols) return;
  const uint64_t g = t / cols, i = t - g * cols;
  const uint64_t r0 = g * G1_SUM_FAN * stride;
  g1_xyzz acc = g1_xyzz::load(xyzz + 32 * (r0 * cols + i));
#pragma unroll 1
  for (int j = 1; j < G1_SUM_FAN; j++) {
    const uint64_t r = r0 + (uint64_t)j * stride;
    if (r >= rows) break;
    acc.add(g1_xyzz::load(xyzz + 32 * (r * cols + i)));
  }
  acc.store(xyzz + 32 * (r0 * cols + i));
}

// out[b m + u] = in[u l + bitrev_l(b)] (8 words each), zero from index len on; m = 2^logm, l = 2^lbits >= 2
__global__ void __launch_bounds__(256) k_coset_rows(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint64_t len,
                                                    int logm, int lbits) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >> (logm + lbits)) return;
  const uint64_t b = t >> logm, u = t & ((1ull << logm) - 1);
  const uint64_t src = (u << lbits) | (__brev((uint32_t)b) >> (32 - lbits));
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (src < len) {
    const uint4* q = reinterpret_cast<const uint4*>(in + 8 * src);
    lo = q[0];
    hi = q[1];
  }
  uint4* o = reinterpret_cast<uint4*>(out + 8 * t);
  o[0] = lo;
  o[1] = hi;
}

// k_coset_rows for `polys` polynomials (polynomial p: len coefficients at in + 8 stride p), into blocks of
// 2^logblk >= m elements whose tail is zero: out[((b polys + p) << logblk) + u] = in_p[u l + bitrev_l(b)] for u < m,
// zero from index len on and for u >= m. Row-major over the polynomials: block b polys + p, so that the
// transformed rows are the rows x (polys 2^logblk) scalars of the multiply-sum pass. The blocks from l polys up
// to `nblocks` (the power of two the batched Fr transform wants) are zero. lbits = 0, logblk = logm: the
// zero-padded coefficients themselves, for the evaluations.
__global__ void __launch_bounds__(256) k_coset_rows_many(uint32_t* __restrict__ out, const uint32_t* __restrict__ in,
                                                         uint64_t polys, uint64_t stride, uint64_t len, int logm, int lbits,
                                                         int logblk, uint64_t nblocks) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t blk = t >> logblk, u = t & ((1ull << logblk) - 1);
  if (blk >= nblocks) return;
  const uint64_t b = blk / polys, p = blk - b * polys;
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if ((b >> lbits) == 0 && (u >> logm) == 0) {
    const uint64_t src = (u << lbits) | (lbits ? __brev((uint32_t)b) >> (32 - lbits) : 0u);
    if (src < len) {
      const uint4* q = reinterpret_cast<const uint4*>(in + 8 * (p * stride + src));
      lo = q[0];
      hi = q[1];
    }
  }
  uint4* o = reinterpret_cast<uint4*>(out + 8 * t);
  o[0] = lo;
  o[1] = hi;
}

// h[p m + k] = u[p 2m + m - 1 + k] for k < m - 1 and the identity for k = m - 1 (64 B points), p < polys, m = 2^logm
__global__ void __launch_bounds__(256) k_coset_slice_many(uint32_t* __restrict__ h, const uint32_t* __restrict__ u, int logm,
                                                          uint64_t total) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint64_t m = 1ull << logm, p = t >> logm, k = t & (m - 1);
  uint4 v[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  if (k < m - 1) {
    const uint4* q = reinterpret_cast<const uint4*>(u + 16 * (2 * m * p + m - 1 + k));
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = q[j];
  }
  uint4* o = reinterpret_cast<uint4*>(h + 16 * t);
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = v[j];
}

// out[b 2^logm + j] = in[b 2^logm + bitrev(j)] (8 words each), logm >= 1
__global__ void __launch_bounds__(256) k_bitrev_blocks(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, int logm,
                                                       uint64_t total) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint64_t j = t & ((1ull << logm) - 1);
  const uint64_t src = (t - j) | (__brev((uint32_t)j) >> (32 - logm));
  const uint4* q = reinterpret_cast<const uint4*>(in + 8 * src);
  uint4* o = reinterpret_cast<uint4*>(out + 8 * t);
  o[0] = q[0];
  o[1] = q[1];
}

// coordinates x * 2^261 (a table row, k_tab_to29) -> x * 2^256, out of place; nelem = 2 npts coordinates.
// flip = nblocks - 1 writes the blocks of 2^lb points in reverse order, each in its own order (lb = 0: the
// points in reverse order); flip = 0: in order
__global__ void __launch_bounds__(256) k_g1ntt_from29(uint32_t* __restrict__ out, const uint32_t* __restrict__ in,
                                                      uint64_t nelem, G1NttWords c251, uint64_t flip, int lb) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nelem) return;
  fq c;
#pragma unroll
  for (int k = 0; k < 8; k++) c.v[k] = c251.w[k];
  const uint64_t p = i >> 1;
  const uint64_t o = flip ? (((((flip - (p >> lb)) << lb) | (p & ((1ull << lb) - 1))) << 1) | (i & 1)) : i;
  (fq::load(in + 8 * i) * c).store(out + 8 * o);
}

G1NttSizes g1_ntt_sizes(int logn) {
  const uint64_t n = 1ull << logn;
  G1NttSizes z;
  z.xyzz = 128 * n;
  z.aff = 64 * n;
  z.scratch = 32 * n;
  z.tw = 4 * (uint64_t)G1NTT_TW_WORDS * (n / 2 + 1);
  return z;
}

void launch_g1_from29(hipStream_t st, uint32_t* out_aff, const uint32_t* in29, uint64_t npts, bool reversed,
                      int block_log) {
  G1NttWords c{};
  c.w[7] = 1u << 27;  // 2^251: (x 2^261)(2^251) / 2^256 = x 2^256 in the Montgomery product
  if (npts)
    hipLaunchKernelGGL(k_g1ntt_from29, dim3(nb(2 * npts)), dim3(256), 0, st, out_aff, in29, 2 * npts, c,
                       reversed ? (npts >> block_log) - 1 : (uint64_t)0, block_log);
}

// pcols: 0, every term has a point of its own; else the points are rows of pcols = 2^k columns that the cols / pcols
// polynomials of a row share (k_g1_mul_each / k_g1_mul_group, MANY; no reduction there)
template <int L>
static void launch_g1_mul_group(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars,
                                uint64_t rows, uint64_t cols, uint64_t ngroups, bool reduce, uint64_t pcols) {
  auto* kern = pcols ? k_g1_mul_group<L, false, true> : reduce ? k_g1_mul_group<L, true> : k_g1_mul_group<L, false>;
  hipLaunchKernelGGL(kern, dim3(nb(ngroups * cols, 64)), dim3(64), 0, st, out_xyzz, in_aff, scalars, rows, cols, ngroups,
                     pcols);
}

static void g1_mul_sum(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars, uint64_t rows,
                       uint64_t cols, uint64_t pcols, bool reduce, int group) {
  if (!rows || !cols) return;
  if (group == 2 && rows > 1 && rows * cols >= G1_MUL_GROUP_MIN_TERMS) {  // two rows per lane, then their sums
    const uint64_t ngroups = (rows + 1) / 2;
    launch_g1_mul_group<2>(st, out_xyzz, in_aff, scalars, rows, cols, ngroups, reduce, pcols);
    rows = ngroups;
  } else if (pcols) {
    hipLaunchKernelGGL((k_g1_mul_each<false, true>), dim3(nb(rows * cols, 64)), dim3(64), 0, st, out_xyzz, in_aff, scalars,
                       rows * cols, cols, pcols);
  } else {
    launch_g1_mul_each(st, out_xyzz, in_aff, scalars, rows * cols, reduce);
  }
  for (uint64_t stride = 1; stride < rows; stride *= G1_SUM_FAN) {
    const uint64_t live = (rows + stride - 1) / stride, ngroups = (live + G1_SUM_FAN - 1) / G1_SUM_FAN;
    hipLaunchKernelGGL(k_g1_col_sum, dim3(nb(ngroups * cols, 64)), dim3(64), 0, st, out_xyzz, rows, cols, stride, ngroups);
  }
}

void launch_g1_mul_sum(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars, uint64_t rows,
                       uint64_t cols, bool reduce, int group) {
  g1_mul_sum(st, out_xyzz, in_aff, scalars, rows, cols, 0, reduce, group);
}

void launch_g1_mul_sum_many(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars,
                            uint64_t rows, uint64_t polys, uint64_t pcols, int group) {
  g1_mul_sum(st, out_xyzz, in_aff, scalars, rows, polys * pcols, pcols, false, group);
}

void launch_coset_rows_many(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t polys, uint64_t stride, uint64_t len,
                            int logm, int lbits, int logblk, uint64_t nblocks) {
  hipLaunchKernelGGL(k_coset_rows_many, dim3(nb(nblocks << logblk)), dim3(256), 0, st, out, in, polys, stride, len, logm,
                     lbits, logblk, nblocks);
}

void launch_coset_slice_many(hipStream_t st, uint32_t* h, const uint32_t* u, int logm, uint64_t polys) {
  hipLaunchKernelGGL(k_coset_slice_many, dim3(nb(polys << logm)), dim3(256), 0, st, h, u, logm, polys << logm);
}

void launch_coset_rows(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t len, int logm, int lbits) {
  hipLaunchKernelGGL(k_coset_rows, dim3(nb(1ull << (logm + lbits))), dim3(256), 0, st, out, in, len, logm, lbits);
}

void launch_bitrev_blocks(hipStream_t st, uint32_t* out, const uint32_t* in, int logm, uint64_t nblocks) {
  const uint64_t total = nblocks << logm;
  hipLaunchKernelGGL(k_bitrev_blocks, dim3(nb(total)), dim3(256), 0, st, out, in, logm, total);
}

void launch_g1_scale(hipStream_t st, const G1NttWork& w, uint32_t* out_aff, const uint32_t* in_aff, uint64_t n,
                     const uint32_t scale_std[8]) {
  G1NttWords one{}, scale;
  for (int j = 0; j < 8; j++) scale.w[j] = scale_std[j];
  hipLaunchKernelGGL(k_g1ntt_twiddles, dim3(1), dim3(256), 0, st, w.tw, (uint64_t)0, one, scale);
  hipLaunchKernelGGL(k_g1ntt_scale, dim3(nb(n, 64)), dim3(64), 0, st, w.xyzz, in_aff, w.tw, n);
  launch_batch_affine(st, out_aff, w.xyzz, w.scratch, n);
}

void launch_g1_mul_each(hipStream_t st, uint32_t* out_xyzz, const uint32_t* in_aff, const uint32_t* scalars, uint64_t n,
                        bool reduce) {
  if (!n) return;
  auto* kern = reduce ? k_g1_mul_each<true> : k_g1_mul_each<false>;
  hipLaunchKernelGGL(kern, dim3(nb(n, 64)), dim3(64), 0, st, out_xyzz, in_aff, scalars, n, (uint64_t)0, (uint64_t)0);
}

void g1_ntt_run(hipStream_t st, const G1NttWork& w, uint32_t* out_aff, const uint32_t* in_aff, int logn,
                const uint32_t root_mont[8], const uint32_t* scale_std, int mapping, int stages) {
  const uint64_t n = 1ull << logn, half = n / 2;
  const int nstages = stages < 0 ? logn : stages;  // fewer: the transforms of the strided subsequences, side by side
  G1NttWords root, scale{};
  for (int j = 0; j < 8; j++) root.w[j] = root_mont[j];
  bool scaled = false;
  if (scale_std) {
    for (int j = 0; j < 8; j++) {
      scale.w[j] = scale_std[j];
      scaled |= scale_std[j] != (j == 0 ? 1u : 0u);
    }
  }
  hipLaunchKernelGGL(k_g1ntt_twiddles, dim3(nb(half + 1)), dim3(256), 0, st, w.tw, half, root, scale);
  const uint32_t* src = in_aff;
  for (int logh = 0; logh < nstages; logh++) {
    const bool last = logh == nstages - 1;
    const bool uni = mapping == G1NTT_MAP_WAVE || (mapping == G1NTT_MAP_AUTO && logh > 0);
    if (uni && logn - 1 - logh >= 6)
      hipLaunchKernelGGL(k_g1ntt_stage<true>, dim3(nb(half, 64)), dim3(64), 0, st, w.xyzz, src, w.tw, half, logh, logn,
                         logh == 0);
    else
      hipLaunchKernelGGL(k_g1ntt_stage<false>, dim3(nb(half, 64)), dim3(64), 0, st, w.xyzz, src, w.tw, half, logh, logn,
                         logh == 0);
    uint32_t* dst = last && !scaled ? out_aff : w.aff;
    launch_batch_affine(st, dst, w.xyzz, w.scratch, n);
    src = dst;
  }
  if (scaled) {
    hipLaunchKernelGGL(k_g1ntt_scale, dim3(nb(n, 64)), dim3(64), 0, st, w.xyzz, src, w.tw + G1NTT_TW_WORDS * half, n);
    launch_batch_affine(st, out_aff, w.xyzz, w.scratch, n);
  } else if (logn == 0 && out_aff != in_aff) {
    hipMemcpyAsync(out_aff, in_aff, 64, hipMemcpyDeviceToDevice, st);
  }
}

void g1_ntt_many_run(hipStream_t st, const G1NttWork& w, uint32_t* out_aff, const uint32_t* in_aff, uint64_t polys,
                     int logn, const uint32_t root_mont[8], int mapping) {
  const uint64_t n = 1ull << logn, total = polys << logn;
  if (!polys) return;
  if (logn == 0) {
    if (out_aff != in_aff) hipMemcpyAsync(out_aff, in_aff, 64 * total, hipMemcpyDeviceToDevice, st);
    return;
  }
  G1NttWords root, scale{};
  for (int j = 0; j < 8; j++) root.w[j] = root_mont[j];
  hipLaunchKernelGGL(k_g1ntt_twiddles, dim3(nb(n / 2 + 1)), dim3(256), 0, st, w.tw, n / 2, root, scale);
  const uint32_t* src = in_aff;
  for (int logh = 0; logh < logn; logh++) {
    const bool uni = mapping != G1NTT_MAP_LANE && g1ntt_many_uniform(polys, logn, logh);
    const dim3 grid((unsigned)g1ntt_many_blocks(polys, logn, logh, uni));
    if (uni)
      hipLaunchKernelGGL(k_g1ntt_stage_many<true>, grid, dim3(G1NTT_MANY_BLOCK), 0, st, w.xyzz, src, w.tw, polys, logh, logn,
                         logh == 0);
    else
      hipLaunchKernelGGL(k_g1ntt_stage_many<false>, grid, dim3(G1NTT_MANY_BLOCK), 0, st, w.xyzz, src, w.tw, polys, logh, logn,
                         logh == 0);
    uint32_t* dst = logh == logn - 1 ? out_aff : w.aff;
    launch_batch_affine(st, dst, w.xyzz, w.scratch, total);
    src = dst;
  }
}

}  // namespace kgs
