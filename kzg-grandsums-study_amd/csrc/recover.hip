// The Fr kernels of kgs_kzg_recover_cosets (include/kgs.h), for gfx950: a polynomial of known
// length back from a subset of its cosets. n = 2^nbits, l = 2^lbits, m = n / l, a_i = w^(i l) = Fr.w[logm]^i.
//
//   k_rc_mark      row_of[i] = the lowest input row that names coset i (RC_NONE: the coset is missing); flags an
//                  index >= m and a coset named twice
//   k_rc_leaf      the product tree's leaves: B consecutive coset slots -> Y^(B - d) prod (Y - a_i) over the slot's d
//                  missing cosets, monic of degree B whatever d is, built in LDS
//   k_rc_pad, k_rc_pointmul   one level of the tree around the batched transforms (ntt_dif_blocks / ntt_dit_blocks):
//                  (Y^d + a)(Y^d + b) as a cyclic product of size 2d of the monic polynomials whole
//   k_rc_zcoef     z's coefficients out of the root, and again scaled by (g^l)^t for the shifted set
//   k_rc_batch_inv the m inversions, one binary-Euclid inversion per block of 1024 elements
//   k_rc_scatter   E Z on the domain, natural order: y_{k,j} z(a_i) at i + m j, zero on a missing coset
//   k_rc_divide    times 1 / z(g^l a_i) in the forward transform's bit-reversed order
//   k_rc_check_copy   the first len coefficients out; flags a nonzero one from len on
// and, further down, the k_rcm_* kernels of kgs_kzg_recover_cosets_many.
//
// Every product is field.hpp's canonical Montgomery product and every stored value is canonical: the kernels
// here are bound by their HBM traffic (or, the leaves, by LDS round trips), not by the multiplier.
#include "kernels.hpp"

namespace kgs {

static inline unsigned rc_nb(uint64_t work, unsigned bs = 256) { return (unsigned)((work + bs - 1) / bs); }

__device__ __forceinline__ bool rc_canonical(const fr& x) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)__builtin_subc(x.v[i], FrP::p[i], borrow, &borrow);
  return borrow != 0;
}

__global__ void __launch_bounds__(256)
    k_rc_mark(uint32_t* __restrict__ row_of, uint32_t* __restrict__ flags, const uint64_t* __restrict__ index,
              uint64_t count, uint64_t m) {
  KGS_AUX_PRIO();
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint64_t i = index[k];
  if (i >= m) {
    atomicMin(flags + RC_FLAG_INDEX, (uint32_t)k);
    return;
  }
  // the previous mark of the coset: set already = named twice. The later of the two rows is the offender; the
  // minimum kept in row_of makes the lowest offender the one reported whatever order the rows arrive in
  const uint32_t prev = atomicMin(row_of + i, (uint32_t)k);
  if (prev != RC_NONE) atomicMin(flags + RC_FLAG_DUP, prev > (uint32_t)k ? prev : (uint32_t)k);
}

// LDS of a leaf block of B = blockDim.x threads: the running coefficients twice (double-buffered: one barrier per
// step) and the slots' a_i, each as two planes of 16-byte halves (lanes on consecutive 16-byte slots, as the NTT
// tile: a 32-byte element stride would put two lanes of every 16-lane phase on the same banks), then B flags.
__device__ __forceinline__ fr rc_lds_get(const uint4* base, int B, int e) {
  const uint4 a = base[e], b = base[B + e];
  fr r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void rc_lds_put(uint4* base, int B, int e, const fr& x) {
  base[e] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  base[B + e] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// Block b: slots [b B, (b + 1) B) of the m = 2^logm cosets (B divides m). Thread t keeps coefficient t of the
// running monic product in registers; a step multiplies by (Y - a): c'_t = c_{t-1} - a c_t, with the leading 1
// taken as c_deg. A present slot takes no step: its factor Y is the shift of the final store. tw: the forward
// stage table, w_m^t = tw[m / 2 + t] for t < m / 2 and its negation m / 2 further on.
__global__ void __launch_bounds__(RC_LEAF_MAX)
    k_rc_leaf(uint32_t* __restrict__ T, const uint32_t* __restrict__ row_of, const uint32_t* __restrict__ tw, int logm) {
  KGS_AUX_PRIO();
  extern __shared__ __attribute__((aligned(16))) uint4 rc_sh[];
  const int B = blockDim.x, t = threadIdx.x;
  uint4* cbuf = rc_sh;              // 2 buffers x 2 planes x B
  uint4* abuf = rc_sh + 4 * B;      // 2 planes x B
  uint32_t* miss = reinterpret_cast<uint32_t*>(rc_sh + 6 * B);
  const uint64_t slot = (uint64_t)blockIdx.x * B + t, half = (1ull << logm) >> 1;
  const bool missing = row_of[slot] == RC_NONE;
  miss[t] = missing;
  if (missing) {
    fr a = fr::one();
    if (logm) {
      const bool hi = slot >= half;
      a = fr::load(tw + 8 * (half + (hi ? slot - half : slot)));
      if (hi) a = a.neg();
    }
    rc_lds_put(abuf, B, t, a);
  }
  __syncthreads();
  fr c = fr::zero();
  int deg = 0, buf = 0;
  for (int i = 0; i < B; i++) {
    if (!miss[i]) continue;  // uniform over the block
    const fr cur = t == deg ? fr::one() : c;
    uint4* cb = cbuf + 2 * B * buf;
    rc_lds_put(cb, B, t, cur);
    __syncthreads();
    if (t <= deg + 1) {  // coefficients above deg + 1 stay zero
      const fr prev = t ? rc_lds_get(cb, B, t - 1) : fr::zero();
      c = prev - rc_lds_get(abuf, B, i) * cur;
    }
    deg++;
    buf ^= 1;
  }
  // Y^(B - deg) times the product; its leading 1 (index B) stays implicit
  uint32_t* out = T + 8 * ((uint64_t)blockIdx.x * B);
  if (t < deg) c.store(out + 8 * (B - deg + t));
  if (t < B - deg) fr::zero().store(out + 8 * t);
}

// W (2m elements) = the m / d polynomials of T (d = 2^logd low coefficients each) zero-padded to 2d
__global__ void __launch_bounds__(256) k_rc_pad(uint32_t* __restrict__ W, const uint32_t* __restrict__ T, int logd, uint64_t m) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2 * m) return;
  const uint64_t d = 1ull << logd, p = x & (2 * d - 1), q = x >> (logd + 1);
  (p < d ? fr::load(T + 8 * (q * d + p)) : fr::zero()).store(W + 8 * x);
}

// W: the transforms of size 2d of the padded polynomials, each in bit-reversed order. Pair P (blocks 2P, 2P + 1):
// the monic polynomials whole take +1 at the even powers of w_2d and -1 at the odd ones (Y^d there), i.e. by
// the position's top bit; the product's Y^2d wraps to 1 at every point. T[2d P + p] = (A_p + s)(B_p + s) - 1.
__global__ void __launch_bounds__(256)
    k_rc_pointmul(uint32_t* __restrict__ T, const uint32_t* __restrict__ W, int logd, uint64_t m) {
  KGS_AUX_PRIO();
  const uint64_t y = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= m) return;
  const uint64_t d = 1ull << logd, p = y & (2 * d - 1), P = y >> (logd + 1);
  const fr one = fr::one();
  fr a = fr::load(W + 8 * (4 * d * P + p)), b = fr::load(W + 8 * (4 * d * P + 2 * d + p));
  if (p < d) {
    a = a + one;
    b = b + one;
  } else {
    a = a - one;
    b = b - one;
  }
  (a * b - one).store(T + 8 * y);
}

// The root is Y^count z(Y): zc[t] = z_t (t < m; z's leading 1 at m - count included, zeros above), zs[t] = z_t g^(l t)
// with g^(l t) read from the domain's coset powers
__global__ void __launch_bounds__(256)
    k_rc_zcoef(uint32_t* __restrict__ zc, uint32_t* __restrict__ zs, const uint32_t* __restrict__ T, uint64_t count,
               uint64_t m, const uint32_t* __restrict__ coset_pow, int lbits) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  const uint64_t dz = m - count;
  const fr v = t < dz ? fr::load(T + 8 * (count + t)) : t == dz ? fr::one() : fr::zero();
  v.store(zc + 8 * t);
  (v * fr::load(coset_pow + 8 * (t << lbits))).store(zs + 8 * t);
}

// zev: z(a_i) at position bitrev(i) (the size-m forward transform's own order)
__global__ void __launch_bounds__(256)
    k_rc_scatter(uint32_t* __restrict__ out, const uint32_t* __restrict__ ys, const uint32_t* __restrict__ row_of,
                 const uint32_t* __restrict__ zev, uint32_t* __restrict__ flags, int logm, int lbits) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= (1ull << (logm + lbits))) return;
  const uint32_t i = (uint32_t)(x & ((1ull << logm) - 1));
  const uint64_t j = x >> logm;
  const uint32_t k = row_of[i];
  fr v = fr::zero();
  if (k != RC_NONE) {
    const uint64_t e = ((uint64_t)k << lbits) + j;
    const fr y = fr::load(ys + 8 * e);
    if (!rc_canonical(y)) {
      atomicMin(flags + RC_FLAG_VALUE, (uint32_t)e);
    } else {
      const uint32_t ib = logm ? __brev(i) >> (32 - logm) : 0;
      v = y * fr::load(zev + 8 * (uint64_t)ib);
    }
  }
  v.store(out + 8 * x);
}

// data: n values at the bit-reversed positions of the size-n forward transform; position x belongs to coset
// bitrev_n(x) mod m, whose inverse sits at x >> lbits of inv (the size-m transform's bit-reversed order)
__global__ void __launch_bounds__(256)
    k_rc_divide(uint32_t* __restrict__ data, const uint32_t* __restrict__ inv, int lbits, uint64_t n) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  (fr::load(data + 8 * x) * fr::load(inv + 8 * (x >> lbits))).store(data + 8 * x);
}

// out[i] = 1 / in[i], i < n (0 -> 0). A block inverts RC_INV_TILE elements with ONE inversion: products per thread,
// prefix and suffix products over the block's threads in LDS, the binary-Euclid inverse of the block's product on
// one lane (launch_fr_batch_inv's per-thread Fermat inverse is a chain of ~320 dependent products, 0.35 ms however
// few elements there are; this one is ~0.05 ms), then back down by Montgomery's trick.
constexpr int RC_INV_PER = 4, RC_INV_NT = 256, RC_INV_TILE = RC_INV_PER * RC_INV_NT;
__global__ void __launch_bounds__(RC_INV_NT)
    k_rc_batch_inv(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint64_t n) {
  KGS_AUX_PRIO();
  __shared__ __attribute__((aligned(16))) uint32_t lds[RC_INV_NT * 8];
  __shared__ __attribute__((aligned(16))) uint32_t tot[8];
  const uint32_t t = threadIdx.x;
  const uint64_t base = ((uint64_t)blockIdx.x * RC_INV_NT + t) * RC_INV_PER;
  fr v[RC_INV_PER], before[RC_INV_PER];
  bool zero[RC_INV_PER];
  fr p = fr::one();
#pragma unroll
  for (int r = 0; r < RC_INV_PER; r++) {
    v[r] = base + r < n ? fr::load(in + 8 * (base + r)) : fr::one();
    zero[r] = v[r].is_zero();
    if (zero[r]) v[r] = fr::one();
    before[r] = p;
    p = p * v[r];
  }
  fr pre = p, suf = p;  // inclusive prefix / suffix products over the threads
  for (uint32_t off = 1; off < RC_INV_NT; off <<= 1) {
    pre.store(lds + 8 * t);
    __syncthreads();
    if (t >= off) pre = fr::load(lds + 8 * (t - off)) * pre;
    __syncthreads();
  }
  for (uint32_t off = 1; off < RC_INV_NT; off <<= 1) {
    suf.store(lds + 8 * t);
    __syncthreads();
    if (t + off < RC_INV_NT) suf = suf * fr::load(lds + 8 * (t + off));
    __syncthreads();
  }
  if (t == RC_INV_NT - 1) pre.inverse_bgcd().store(tot);
  pre.store(lds + 8 * t);
  __syncthreads();
  const fr total_inv = fr::load(tot);
  const fr pex = t ? fr::load(lds + 8 * (t - 1)) : fr::one();
  __syncthreads();
  suf.store(lds + 8 * t);
  __syncthreads();
  const fr sex = t < RC_INV_NT - 1 ? fr::load(lds + 8 * (t + 1)) : fr::one();
  fr acc = total_inv * pex * sex;  // the inverse of this thread's product
#pragma unroll
  for (int r = RC_INV_PER - 1; r >= 0; r--) {
    if (base + r < n) (zero[r] ? fr::zero() : acc * before[r]).store(out + 8 * (base + r));
    acc = acc * v[r];
  }
}

__global__ void __launch_bounds__(256)
    k_rc_check_copy(uint32_t* __restrict__ coef, const uint32_t* __restrict__ q, uint64_t len, uint64_t n,
                    uint32_t* __restrict__ flags) {
  KGS_AUX_PRIO();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const fr v = fr::load(q + 8 * j);
  if (j < len)
    v.store(coef + 8 * j);
  else if (!v.is_zero())
    flags[RC_FLAG_HIGH] = 1;
}

// ---------------------------------------------------------------- kgs_kzg_recover_cosets_many
// P = polys rounded up to a power of two polynomials side by side: row_of, T, zc / zs / inv hold P blocks of m, the
// size-n array P blocks of n. The levels (launch_rc_level), the batch inversion and the division (inv[x >> lbits] is
// block b's inverse at (x mod n) >> lbits) are the single call's launches over the longer arrays; the kernels below
// are the ones that need to know where a polynomial ends.
//
//   k_rcm_mark        row_of[b m + i] = the lowest cell naming (b, i); cnt[b] = its distinct cosets; the two flags
//   k_rcm_leaf        k_rc_leaf with a_i from the slot's index mod m: a leaf (min(B, m) slots) never spans two polynomials
//   k_rcm_zcoef       k_rc_zcoef per block, each root with its own count
//   k_rcm_scatter     E_b Z_b into block b of the size-n array at the bit-reversed position within the block
//   k_rcm_twist       times g^j, j the position within the block
//   k_rcm_check_copy  times g^-j, the first len coefficients to the strided output, one flag per polynomial

__global__ void __launch_bounds__(256)
    k_rcm_mark(uint32_t* __restrict__ row_of, uint32_t* __restrict__ flags, uint32_t* __restrict__ cnt,
               const uint32_t* __restrict__ poly_of, const uint64_t* __restrict__ index, uint64_t count, uint64_t polys,
               uint64_t m) {
  KGS_AUX_PRIO();
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint64_t b = poly_of[k], i = index[k];
  if (b >= polys || i >= m) {
    atomicMin(flags + RC_FLAG_INDEX, (uint32_t)k);
    return;
  }
  // as k_rc_mark: the later of two cells that name a pair is the offender, the minimum the one reported. Only the
  // first cell to arrive at a pair counts it, so cnt[b] <= m whatever the input holds
  const uint32_t prev = atomicMin(row_of + b * m + i, (uint32_t)k);
  if (prev != RC_NONE)
    atomicMin(flags + RC_FLAG_DUP, prev > (uint32_t)k ? prev : (uint32_t)k);
  else
    atomicAdd(cnt + b, 1u);
}

// Block b: slots [b B, (b + 1) B) of the P m slots, B = blockDim.x a power of two that divides m. k_rc_leaf's body
// with one expression changed, a_i = w_m^(slot mod m): the single call's kernel stays the code DESIGN.md §22 measured,
// so the two bodies are kept in step by hand. A change to the steps of one belongs in the other too.
__global__ void __launch_bounds__(RC_LEAF_MAX)
    k_rcm_leaf(uint32_t* __restrict__ T, const uint32_t* __restrict__ row_of, const uint32_t* __restrict__ tw, int logm) {
  KGS_AUX_PRIO();
  extern __shared__ __attribute__((aligned(16))) uint4 rc_sh[];
  const int B = blockDim.x, t = threadIdx.x;
  uint4* cbuf = rc_sh;              // 2 buffers x 2 planes x B
  uint4* abuf = rc_sh + 4 * B;      // 2 planes x B
  uint32_t* miss = reinterpret_cast<uint32_t*>(rc_sh + 6 * B);
  const uint64_t slot = (uint64_t)blockIdx.x * B + t, half = (1ull << logm) >> 1;
  const bool missing = row_of[slot] == RC_NONE;
  miss[t] = missing;
  if (missing) {
    fr a = fr::one();
    if (logm) {
      const uint64_t i = slot & ((1ull << logm) - 1);
      const bool hi = i >= half;
      a = fr::load(tw + 8 * (half + (hi ? i - half : i)));
      if (hi) a = a.neg();
    }
    rc_lds_put(abuf, B, t, a);
  }
  __syncthreads();
  fr c = fr::zero();
  int deg = 0, buf = 0;
  for (int i = 0; i < B; i++) {
    if (!miss[i]) continue;  // uniform over the block
    const fr cur = t == deg ? fr::one() : c;
    uint4* cb = cbuf + 2 * B * buf;
    rc_lds_put(cb, B, t, cur);
    __syncthreads();
    if (t <= deg + 1) {
      const fr prev = t ? rc_lds_get(cb, B, t - 1) : fr::zero();
      c = prev - rc_lds_get(abuf, B, i) * cur;
    }
    deg++;
    buf ^= 1;
  }
  uint32_t* out = T + 8 * ((uint64_t)blockIdx.x * B);
  if (t < deg) c.store(out + 8 * (B - deg + t));
  if (t < B - deg) fr::zero().store(out + 8 * t);
}

// Block b of T is Y^cnt[b] z_b(Y) without its leading 1. cnt[b] = 0 (a polynomial with no cell, and the padding up to
// P) leaves no z of degree < m: its m low coefficients are stored as they are, and the status comes from the count.
__global__ void __launch_bounds__(256)
    k_rcm_zcoef(uint32_t* __restrict__ zc, uint32_t* __restrict__ zs, const uint32_t* __restrict__ T,
                const uint32_t* __restrict__ cnt, int logm, uint64_t total, const uint32_t* __restrict__ coset_pow,
                int lbits) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= total) return;
  const uint64_t m = 1ull << logm, b = x >> logm, t = x & (m - 1);
  uint64_t have = cnt[b];
  if (have > m) have = m;
  const uint64_t dz = m - have;
  const fr v = t < dz ? fr::load(T + 8 * ((b << logm) + have + t)) : t == dz ? fr::one() : fr::zero();
  v.store(zc + 8 * x);
  (v * fr::load(coset_pow + 8 * (t << lbits))).store(zs + 8 * x);
}

// Output position o of block b is domain point x = bitrev_n(o): coset i = x mod m = bitrev_m(o >> lbits), value
// j = x / m = bitrev_l(o mod l). So the l consecutive outputs o share one cell, whose row they read whole (permuted),
// and z_b(a_i) sits at (o >> lbits) of the size-m transform's own order: the writes are coalesced.
__global__ void __launch_bounds__(256)
    k_rcm_scatter(uint32_t* __restrict__ out, const uint32_t* __restrict__ ys, const uint32_t* __restrict__ row_of,
                  const uint32_t* __restrict__ zev, uint32_t* __restrict__ flags, int logm, int lbits, uint64_t total) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= total) return;
  const uint64_t u = x >> lbits;  // b m + (o >> lbits)
  const uint32_t ub = (uint32_t)(u & ((1ull << logm) - 1));
  const uint32_t i = logm ? __brev(ub) >> (32 - logm) : 0;
  const uint32_t jb = (uint32_t)(x & ((1ull << lbits) - 1));
  const uint32_t j = lbits ? __brev(jb) >> (32 - lbits) : 0;
  const uint32_t k = row_of[u - ub + i];
  fr v = fr::zero();
  if (k != RC_NONE) {
    const uint64_t e = ((uint64_t)k << lbits) + j;
    const fr y = fr::load(ys + 8 * e);
    if (!rc_canonical(y))
      atomicMin(flags + RC_FLAG_VALUE, (uint32_t)e);
    else
      v = y * fr::load(zev + 8 * u);
  }
  v.store(out + 8 * x);
}

__global__ void __launch_bounds__(256)
    k_rcm_twist(uint32_t* __restrict__ data, const uint32_t* __restrict__ tab, int nbits, uint64_t total) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= total) return;
  (fr::load(data + 8 * x) * fr::load(tab + 8 * (x & ((1ull << nbits) - 1)))).store(data + 8 * x);
}

// q: polys blocks of n coefficients of q_b(g X). g^-j is not zero, so the check from len on needs no product.
__global__ void __launch_bounds__(256)
    k_rcm_check_copy(uint32_t* __restrict__ coef, const uint32_t* __restrict__ q, const uint32_t* __restrict__ ipow,
                     uint64_t len, uint64_t stride, int nbits, uint64_t total, uint32_t* __restrict__ high) {
  KGS_AUX_PRIO();
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= total) return;
  const uint64_t b = x >> nbits, j = x & ((1ull << nbits) - 1);
  const fr v = fr::load(q + 8 * x);
  if (j < len)
    (v * fr::load(ipow + 8 * j)).store(coef + 8 * (b * stride + j));
  else if (!v.is_zero())
    high[b] = 1;
}

void launch_rc_mark(hipStream_t st, uint32_t* row_of, uint32_t* flags, const uint64_t* index, uint64_t count, uint64_t m) {
  hipLaunchKernelGGL(k_rc_mark, dim3(rc_nb(count)), dim3(256), 0, st, row_of, flags, index, count, m);
}

void launch_rc_leaves(hipStream_t st, uint32_t* T, const uint32_t* row_of, const uint32_t* tw_fwd, int logm, int leaf_log) {
  const unsigned B = 1u << leaf_log;
  hipLaunchKernelGGL(k_rc_leaf, dim3((unsigned)((1ull << logm) >> leaf_log)), dim3(B), rc_leaf_lds_bytes(leaf_log), st, T,
                     row_of, tw_fwd, logm);
}

void launch_rc_level(hipStream_t st, uint32_t* T, uint32_t* W, int logm, int logd, const uint32_t* tw_fwd,
                     const uint32_t* tw_inv, const uint32_t* invm) {
  const uint64_t m = 1ull << logm;
  hipLaunchKernelGGL(k_rc_pad, dim3(rc_nb(2 * m)), dim3(256), 0, st, W, T, logd, m);
  ntt_dif_blocks(st, W, logm + 1, logd + 1, tw_fwd);
  hipLaunchKernelGGL(k_rc_pointmul, dim3(rc_nb(m)), dim3(256), 0, st, T, W, logd, m);
  ntt_dit_blocks(st, T, logm, logd + 1, tw_inv, invm + 8 * (logd + 1));
}

void launch_rc_zcoef(hipStream_t st, uint32_t* zc, uint32_t* zs, const uint32_t* T, uint64_t count, uint64_t m,
                     const uint32_t* coset_pow, int lbits) {
  hipLaunchKernelGGL(k_rc_zcoef, dim3(rc_nb(m)), dim3(256), 0, st, zc, zs, T, count, m, coset_pow, lbits);
}

void launch_rc_scatter(hipStream_t st, uint32_t* out, const uint32_t* ys, const uint32_t* row_of, const uint32_t* zev,
                       uint32_t* flags, int logm, int lbits) {
  hipLaunchKernelGGL(k_rc_scatter, dim3(rc_nb(1ull << (logm + lbits))), dim3(256), 0, st, out, ys, row_of, zev, flags, logm,
                     lbits);
}

void launch_rc_divide(hipStream_t st, uint32_t* data, const uint32_t* inv, int lbits, uint64_t n) {
  hipLaunchKernelGGL(k_rc_divide, dim3(rc_nb(n)), dim3(256), 0, st, data, inv, lbits, n);
}

void launch_rc_batch_inv(hipStream_t st, uint32_t* out, const uint32_t* in, uint64_t n) {
  hipLaunchKernelGGL(k_rc_batch_inv, dim3(rc_nb(n, RC_INV_TILE)), dim3(RC_INV_NT), 0, st, out, in, n);
}

void launch_rc_check_copy(hipStream_t st, uint32_t* coef, const uint32_t* q, uint64_t len, uint64_t n, uint32_t* flags) {
  hipLaunchKernelGGL(k_rc_check_copy, dim3(rc_nb(n)), dim3(256), 0, st, coef, q, len, n, flags);
}

void launch_rcm_mark(hipStream_t st, uint32_t* row_of, uint32_t* flags, uint32_t* cnt, const uint32_t* poly_of,
                     const uint64_t* index, uint64_t count, uint64_t polys, uint64_t m) {
  if (!count) return;
  hipLaunchKernelGGL(k_rcm_mark, dim3(rc_nb(count)), dim3(256), 0, st, row_of, flags, cnt, poly_of, index, count, polys, m);
}

void launch_rcm_leaves(hipStream_t st, uint32_t* T, const uint32_t* row_of, const uint32_t* tw_fwd, int logtotal, int logm,
                       int leaf_log) {
  const unsigned B = 1u << leaf_log;
  hipLaunchKernelGGL(k_rcm_leaf, dim3((unsigned)((1ull << logtotal) >> leaf_log)), dim3(B), rc_leaf_lds_bytes(leaf_log), st, T,
                     row_of, tw_fwd, logm);
}

void launch_rcm_zcoef(hipStream_t st, uint32_t* zc, uint32_t* zs, const uint32_t* T, const uint32_t* cnt, int logtotal,
                      int logm, const uint32_t* coset_pow, int lbits) {
  const uint64_t total = 1ull << logtotal;
  hipLaunchKernelGGL(k_rcm_zcoef, dim3(rc_nb(total)), dim3(256), 0, st, zc, zs, T, cnt, logm, total, coset_pow, lbits);
}

void launch_rcm_scatter(hipStream_t st, uint32_t* out, const uint32_t* ys, const uint32_t* row_of, const uint32_t* zev,
                        uint32_t* flags, int logtotal, int logm, int lbits) {
  const uint64_t total = 1ull << logtotal;
  hipLaunchKernelGGL(k_rcm_scatter, dim3(rc_nb(total)), dim3(256), 0, st, out, ys, row_of, zev, flags, logm, lbits, total);
}

void launch_rcm_twist(hipStream_t st, uint32_t* data, const uint32_t* tab, int logtotal, int nbits) {
  const uint64_t total = 1ull << logtotal;
  hipLaunchKernelGGL(k_rcm_twist, dim3(rc_nb(total)), dim3(256), 0, st, data, tab, nbits, total);
}

void launch_rcm_check_copy(hipStream_t st, uint32_t* coef, const uint32_t* q, const uint32_t* ipow, uint64_t len,
                           uint64_t stride, int nbits, uint64_t polys, uint32_t* high) {
  const uint64_t total = polys << nbits;
  hipLaunchKernelGGL(k_rcm_check_copy, dim3(rc_nb(total)), dim3(256), 0, st, coef, q, ipow, len, stride, nbits, total, high);
}

}  // namespace kgs
