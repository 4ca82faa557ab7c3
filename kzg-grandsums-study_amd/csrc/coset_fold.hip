// The Fr side of the batch verifier for coset openings (kgs.h kgs_kzg_verify_cosets_batch,
// kgs_coset_interp_fold), for gfx950.
//
//   k_coset_interp_fold  D_j = sum_k w_k * w^(-i_k j) * J_{k,j}, j < l, in one pass over the count * l values:
//                        J_k is the inverse transform of size l of row k (kgs_ntt's convention), done in
//                        LDS; every block keeps its column sums in registers and writes them once
//   k_coset_fold_reduce  the blocks' partial sums -> D, times 1 / l
//   k_g1_on_curve        one byte per point: the identity, or canonical coordinates on y^2 = x^3 + 3
//   k_coset_screen       the structural verdict of every opening (its proof, its commitment, its index)
//   k_coset_terms, k_coset_terms_srs   the (scalar, point) terms of A and B of a range of openings
//
// A tile is CF_TILE = max(l, 512) consecutive values, max(1, 512 / l) whole rows, held in LDS as eight planes
// of one 32-bit limb each (a wave's reads of a limb then fall on consecutive banks). 256 threads: thread t owns
// the elements t + 256 q of every tile, whose column (t + 256 q) mod l does not depend on the tile, so its
// column sums stay in registers over all the tiles of the block: one accumulator for l <= 256, l / 256 above.
// w^(-i j) is one read of the domain's inverse stage table: i < m and j < l give i j < n, so w^(-i j) is
// tw_inv[n / 2 + i j] for i j < n / 2 and its negation at i j - n / 2 otherwise. The products are field.hpp's
// 32-bit Montgomery products: a row's l log2(l) / 2 + 2 l products are nothing beside its 32 l bytes of HBM
// traffic, so the 29-bit records of the NTT passes would buy nothing here.
#include "kernels.hpp"

namespace kgs {

static inline unsigned cf_nb(uint64_t work, unsigned bs = 256) { return (unsigned)((work + bs - 1) / bs); }

constexpr int CF_THREADS = 256;

template <class P>
__device__ __forceinline__ bool fe_canonical(const Fe<P>& x) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)__builtin_subc(x.v[i], P::p[i], borrow, &borrow);
  return borrow != 0;
}

struct CfPlanes {  // eight planes of E limbs
  uint32_t* sh;
  int E;
  __device__ __forceinline__ fr get(int e) const {
    fr x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = sh[w * E + e];
    return x;
  }
  __device__ __forceinline__ void put(int e, const fr& x) const {
#pragma unroll
    for (int w = 0; w < 8; w++) sh[w * E + e] = x.v[w];
  }
};

// part: gridDim.x x max(l, 256) partial sums (Montgomery), slot s of a block belonging to column s mod l.
// valid: NULL, or one byte per row: a row with 0 is skipped; a row with a value or a weight >= r or an index >= m
// is skipped, gets 0 there and sets *bad. weights / index / ys are only read. nbits >= LB; tw_inv covers 2^nbits.
template <int LB>
__global__ void __launch_bounds__(CF_THREADS)
    k_coset_interp_fold(uint32_t* __restrict__ part, uint8_t* __restrict__ valid, uint32_t* __restrict__ bad,
                        const uint32_t* __restrict__ ys, const uint64_t* __restrict__ index,
                        const uint32_t* __restrict__ weights, uint64_t count, const uint32_t* __restrict__ tw_inv,
                        int nbits) {
  KGS_AUX_PRIO();
  constexpr int L = 1 << LB;
  constexpr int E = L > 512 ? L : 512;      // values of a tile
  constexpr int RT = E / L;                 // its rows
  constexpr int EPT = E / CF_THREADS;       // values of a thread
  constexpr int NACC = L > 256 ? L / 256 : 1;
  __shared__ uint32_t sh_v[8 * E];
  __shared__ uint32_t sh_w[8 * RT];
  __shared__ uint32_t sh_idx[RT];
  __shared__ uint32_t sh_ok[RT];
  const CfPlanes V{sh_v, E}, W{sh_w, RT};
  const int tid = threadIdx.x;
  const uint64_t m = 1ull << (nbits - LB), half_n = (1ull << nbits) >> 1;
  const uint64_t ntiles = (count + RT - 1) / RT;

  fr acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = fr::zero();

  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t row0 = tile * RT;
    // the rows' weights and indices
    for (int r = tid; r < RT; r += CF_THREADS) {
      const uint64_t row = row0 + r;
      uint32_t ok = 0, idx = 0;
      fr w = fr::zero();
      if (row < count && (!valid || valid[row])) {
        w = fr::load(weights + 8 * row);
        const uint64_t i = index[row];
        if (i >= m || !fe_canonical(w)) {
          *bad = 1;
          if (valid) valid[row] = 0;
        } else if (!w.is_zero()) {
          ok = 1;
          idx = (uint32_t)i;
        }
      }
      W.put(r, w);
      sh_idx[r] = idx;
      sh_ok[r] = ok;
    }
    __syncthreads();
    // the values, each row in bit-reversed order; a value >= r switches its row off
#pragma unroll
    for (int q = 0; q < EPT; q++) {
      const int e = tid + CF_THREADS * q, r = e >> LB, j = e & (L - 1);
      fr y = fr::zero();
      if (sh_ok[r]) {
        y = fr::load(ys + 8 * (row0 * L + e));
        if (!fe_canonical(y)) {
          sh_ok[r] = 2;  // every writer writes the same value
          y = fr::zero();
        }
      }
      const int jr = LB ? (int)(__brev((uint32_t)j) >> (32 - (LB ? LB : 1))) : 0;
      V.put((e - j) + jr, y);
    }
    __syncthreads();
    for (int r = tid; r < RT; r += CF_THREADS)
      if (sh_ok[r] == 2) {
        *bad = 1;
        if (valid) valid[row0 + r] = 0;
      }
    // radix-2, decimation in time, root Fr.w[LB]^-1: stage h reads tw_inv[h + t] = w_{2h}^(-t)
#pragma unroll 1
    for (int s = 0; s < LB; s++) {
      const int h = 1 << s;
#pragma unroll
      for (int b = 0; b < E / 512; b++) {
        const int bi = tid + CF_THREADS * b;                   // butterfly of the tile
        const int rowbase = LB ? (bi >> (LB ? LB - 1 : 0)) << LB : 0;
        const int k = bi & ((L >> 1) - 1);
        const int t = k & (h - 1);
        const int i0 = rowbase + ((k >> s) << (s + 1)) + t, i1 = i0 + h;
        const fr x = V.get(i0);
        fr y = V.get(i1);
        if (s) y = y * fr::load(tw_inv + 8 * (h + t));
        V.put(i0, x + y);
        V.put(i1, x - y);
      }
      __syncthreads();
    }
    // element j of row k, times w_k w^(-i_k j), into the thread's sum of column j
#pragma unroll
    for (int q = 0; q < EPT; q++) {
      const int e = tid + CF_THREADS * q, r = e >> LB, j = e & (L - 1);
      if (sh_ok[r] == 1) {
        const uint64_t ex = (uint64_t)sh_idx[r] * (uint64_t)j;  // < n
        fr f = W.get(r);
        bool negate = false;
        if (ex) {
          negate = ex >= half_n;
          f = f * fr::load(tw_inv + 8 * (half_n + (negate ? ex - half_n : ex)));
        }
        const fr v = V.get(e) * f;
        fr& a = acc[NACC > 1 ? q : 0];
        a = negate ? a - v : a + v;
      }
    }
    __syncthreads();
  }
  constexpr int S = L > 256 ? L : 256;
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a].store(part + 8 * ((uint64_t)blockIdx.x * S + tid + CF_THREADS * a));
}

// out[j] (Montgomery) = invl * sum over the blocks b < nblocks and the slots s < S, s mod l == j, of part[b S + s];
// one block per column
__global__ void __launch_bounds__(CF_THREADS)
    k_coset_fold_reduce(uint32_t* __restrict__ out, const uint32_t* __restrict__ part, uint32_t nblocks, int lbits,
                        const uint32_t* __restrict__ invl) {
  KGS_AUX_PRIO();
  __shared__ uint32_t sh[8 * CF_THREADS];
  const CfPlanes V{sh, CF_THREADS};
  const uint32_t l = 1u << lbits, S = l > 256 ? l : 256, per = S >> lbits, j = blockIdx.x;
  const uint64_t entries = (uint64_t)nblocks * per;
  fr acc = fr::zero();
  for (uint64_t t = threadIdx.x; t < entries; t += CF_THREADS) {
    const uint64_t b = t / per, s = (t % per) * l + j;
    acc = acc + fr::load(part + 8 * (b * S + s));
  }
  V.put(threadIdx.x, acc);
  __syncthreads();
  for (int step = CF_THREADS / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) V.put(threadIdx.x, V.get(threadIdx.x) + V.get(threadIdx.x + step));
    __syncthreads();
  }
  if (threadIdx.x == 0) (V.get(0) * fr::load(invl)).store(out + 8 * j);
}

bool launch_coset_interp_fold(hipStream_t st, uint32_t* out, uint32_t* part, uint8_t* valid, uint32_t* bad,
                              const uint32_t* ys, const uint64_t* index, const uint32_t* weights, uint64_t count,
                              const uint32_t* tw_inv, const uint32_t* invm, int nbits, int lbits) {
  if (lbits < 0 || lbits > COSET_FOLD_LBITS_MAX || lbits > nbits) return false;
  const unsigned nblocks = coset_fold_blocks(count, lbits);
#define KGS_CF_CASE(LB)                                                                                              \
  case LB:                                                                                                           \
    hipLaunchKernelGGL(k_coset_interp_fold<LB>, dim3(nblocks), dim3(CF_THREADS), 0, st, part, valid, bad, ys, index, \
                       weights, count, tw_inv, nbits);                                                               \
    break;
  switch (lbits) {
    KGS_CF_CASE(0) KGS_CF_CASE(1) KGS_CF_CASE(2) KGS_CF_CASE(3) KGS_CF_CASE(4) KGS_CF_CASE(5) KGS_CF_CASE(6)
    KGS_CF_CASE(7) KGS_CF_CASE(8) KGS_CF_CASE(9) KGS_CF_CASE(10)
  }
#undef KGS_CF_CASE
  hipLaunchKernelGGL(k_coset_fold_reduce, dim3(1u << lbits), dim3(CF_THREADS), 0, st, out, part, nblocks, lbits,
                     invm + 8 * lbits);
  return true;
}

// ok[i] = 1 if point i (64 B affine LEM) is the identity or has canonical coordinates on the curve, else 0
__global__ void __launch_bounds__(256) k_g1_on_curve(uint8_t* __restrict__ ok, const uint32_t* __restrict__ points,
                                                     uint64_t n) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const g1_aff p = g1_aff::load(points + 16 * i);
  bool good = true;
  if (!p.is_inf()) {
    const fq three = fq::one() + fq::one() + fq::one();
    good = fe_canonical(p.x) && fe_canonical(p.y) && p.y.sqr() == p.x.sqr() * p.x + three;
  }
  ok[i] = good ? 1 : 0;
}

void launch_g1_on_curve(hipStream_t st, uint8_t* ok, const uint32_t* points, uint64_t n) {
  if (n) hipLaunchKernelGGL(k_g1_on_curve, dim3(cf_nb(n)), dim3(256), 0, st, ok, points, n);
}

// valid[k] = the proof of opening k and its commitment are points of the curve, commit_of[k] < ncommits and
// index[k] < m. proof_ok: count bytes, commit_ok: ncommits bytes (k_g1_on_curve)
__global__ void __launch_bounds__(256)
    k_coset_screen(uint8_t* __restrict__ valid, const uint8_t* __restrict__ proof_ok, const uint8_t* __restrict__ commit_ok,
                   const uint32_t* __restrict__ commit_of, const uint64_t* __restrict__ index, uint64_t count,
                   uint64_t ncommits, uint64_t m) {
  KGS_AUX_PRIO();
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t c = commit_of[k];
  valid[k] = proof_ok[k] && c < ncommits && commit_ok[c] && index[k] < m;
}

void launch_coset_screen(hipStream_t st, uint8_t* valid, const uint8_t* proof_ok, const uint8_t* commit_ok,
                         const uint32_t* commit_of, const uint64_t* index, uint64_t count, uint64_t ncommits,
                         uint64_t m) {
  if (count)
    hipLaunchKernelGGL(k_coset_screen, dim3(cf_nb(count)), dim3(256), 0, st, valid, proof_ok, commit_ok, commit_of,
                       index, count, ncommits, m);
}

// Montgomery -> standard form: the Montgomery product with the integer 1
__device__ __forceinline__ fr cf_to_std(const fr& x) {
  fr one = fr::zero();
  one.v[0] = 1;
  return x * one;
}

// The terms of the openings lo <= k < hi, cnt = hi - lo, standard-form scalars and 64 B points:
//   t < cnt            w_k         proof_k          (A)
//   cnt + t            w_k         commitment c(k)  (B from here on)
//   2 cnt + t          w_k a_{i_k} proof_k
//   3 cnt + j, j < l   -D_j        srs_j            (k_coset_terms_srs)
// An opening with valid[k] == 0 gets zero scalars and identities. a_i = w^(i l) = Fr.w[nbits - lbits]^i is read
// from the forward stage table: tw_fwd[m / 2 + i] below m / 2, the negation of tw_fwd[i] from there on.
__global__ void __launch_bounds__(256)
    k_coset_terms(uint32_t* __restrict__ scal, uint32_t* __restrict__ pts, const uint8_t* __restrict__ valid,
                  const uint32_t* __restrict__ weights, const uint64_t* __restrict__ index,
                  const uint32_t* __restrict__ commit_of, const uint32_t* __restrict__ commits,
                  const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ tw_fwd, uint64_t lo, uint64_t cnt,
                  int nbits, int lbits) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cnt) return;
  const uint64_t k = lo + t;
  uint4* p0 = reinterpret_cast<uint4*>(pts + 16 * t);
  uint4* p1 = reinterpret_cast<uint4*>(pts + 16 * (cnt + t));
  uint4* p2 = reinterpret_cast<uint4*>(pts + 16 * (2 * cnt + t));
  if (!valid[k]) {
    const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) p0[i] = p1[i] = p2[i] = z;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      reinterpret_cast<uint4*>(scal + 8 * t)[i] = z;
      reinterpret_cast<uint4*>(scal + 8 * (cnt + t))[i] = z;
      reinterpret_cast<uint4*>(scal + 8 * (2 * cnt + t))[i] = z;
    }
    return;
  }
  const fr w = fr::load(weights + 8 * k);
  const uint64_t i = index[k], half_m = (1ull << (nbits - lbits)) >> 1;
  fr wa = w;
  if (i) {
    const fr wp = w * fr::load(tw_fwd + 8 * (i < half_m ? half_m + i : i));
    wa = i < half_m ? wp : fr::zero() - wp;  // wp != 0
  }
  const fr ws = cf_to_std(w), was = cf_to_std(wa);
  ws.store(scal + 8 * t);
  ws.store(scal + 8 * (cnt + t));
  was.store(scal + 8 * (2 * cnt + t));
  const uint4* proof = reinterpret_cast<const uint4*>(proofs + 16 * k);
  const uint4* commit = reinterpret_cast<const uint4*>(commits + 16 * (uint64_t)commit_of[k]);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint4 a = proof[q];
    p0[q] = a;
    p2[q] = a;
    p1[q] = commit[q];
  }
}

// the l terms -D_j srs_j of B, behind the 3 cnt terms of the openings
__global__ void __launch_bounds__(256)
    k_coset_terms_srs(uint32_t* __restrict__ scal, uint32_t* __restrict__ pts, const uint32_t* __restrict__ D,
                      const uint32_t* __restrict__ srs, uint64_t cnt, uint64_t l) {
  KGS_AUX_PRIO();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= l) return;
  const fr ds = cf_to_std(fr::zero() - fr::load(D + 8 * j));
  ds.store(scal + 8 * (3 * cnt + j));
#pragma unroll
  for (int q = 0; q < 4; q++)
    reinterpret_cast<uint4*>(pts + 16 * (3 * cnt + j))[q] = reinterpret_cast<const uint4*>(srs + 16 * j)[q];
}

void launch_coset_terms(hipStream_t st, uint32_t* scal, uint32_t* pts, const uint8_t* valid, const uint32_t* weights,
                        const uint64_t* index, const uint32_t* commit_of, const uint32_t* commits,
                        const uint32_t* proofs, const uint32_t* D, const uint32_t* srs, const uint32_t* tw_fwd,
                        uint64_t lo, uint64_t cnt, int nbits, int lbits) {
  if (cnt)
    hipLaunchKernelGGL(k_coset_terms, dim3(cf_nb(cnt)), dim3(256), 0, st, scal, pts, valid, weights, index, commit_of,
                       commits, proofs, tw_fwd, lo, cnt, nbits, lbits);
  hipLaunchKernelGGL(k_coset_terms_srs, dim3(cf_nb(1ull << lbits)), dim3(256), 0, st, scal, pts, D, srs, cnt,
                     1ull << lbits);
}

}  // namespace kgs
