// Table multiplicities of a lookup (kgs.h kgs_lookup_multiplicities): m[j] = number of selected rows
// of F equal to table row j, all of a repeated table row's count on its first occurrence. A hash
// join on the GPU (gfx950):
//   * k_lk_insert  one thread per table row: open addressing over uint32 row indices, linear probing,
//                  capacity the power of two >= 2n. A slot goes EMPTY -> j once (atomicCAS) and then
//                  only to a smaller index of an EQUAL row (atomicMin), so every distinct row ends in
//                  exactly one slot, holding its lowest table index, whatever the interleaving.
//   * k_lk_probe   one thread per row of F: selector check, probe, atomicAdd on the matched row's
//                  counter (equal targets inside a wave are summed first); the lowest missing row
//                  and the lowest row with a non-binary selector go to two atomicMin flags.
//   * k_lk_write   counter -> 32 B Montgomery element.
// Rows are compared as elements of Fr: every 256-bit word is reduced mod r before it is hashed or
// compared (the prover accepts inputs >= r). The kernels read each input once for the hash and again
// (cache-resident for the probing thread's own row) for the compares; nothing but the index table
// and the counters is written. Integer atomics only: the result does not depend on arrival order.
#include "kernels.hpp"

namespace kgs {

static inline unsigned nb(uint64_t work, unsigned bs = 256) { return (unsigned)((work + bs - 1) / bs); }

constexpr uint32_t LK_EMPTY = 0xFFFFFFFFu;

// limb i of r << SH (4r < 2^256)
template <int SH>
__device__ __forceinline__ constexpr uint32_t lk_rsh(int i) {
  return SH == 0 ? FrP::p[i] : (FrP::p[i] << SH) | (i ? FrP::p[i - 1] >> (32 - SH) : 0u);
}
template <int SH>
__device__ __forceinline__ fr lk_cond_sub(const fr& a) {  // a - (r << SH) if that is not negative
  fr d, o;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d.v[i] = __builtin_subc(a.v[i], lk_rsh<SH>(i), borrow, &borrow);
#pragma unroll
  for (int i = 0; i < 8; i++) o.v[i] = borrow ? a.v[i] : d.v[i];
  return o;
}
// any 256-bit word (< 2^256 < 6r) -> its canonical residue: < 4r + (2^256 - 4r < 2r), < 2r, < r
__device__ __forceinline__ fr lk_canon(const uint32_t* p) {
  return lk_cond_sub<0>(lk_cond_sub<1>(lk_cond_sub<2>(fr::load(p))));
}

// One multiply-xorshift round per 32-bit word and the murmur3 64-bit finaliser at the end: every word
// of every column reaches every bit of the slot index (range tables, rows that differ in one high limb
// or in the last column only do not cluster).
__device__ __forceinline__ uint64_t lk_mix(uint64_t h, uint32_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
__device__ __forceinline__ uint64_t lk_hash_row(const LookupCols& cols, uint64_t i) {
  uint64_t h = 0x2545F4914F6CDD1Dull;
  for (int c = 0; c < cols.k; c++) {
    const fr x = lk_canon(cols.col[c] + 8 * i);
#pragma unroll
    for (int w = 0; w < 8; w++) h = lk_mix(h, x.v[w]);
  }
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}
__device__ __forceinline__ bool lk_rows_equal(const LookupCols& A, uint64_t ia, const LookupCols& B, uint64_t ib) {
  for (int c = 0; c < A.k; c++)
    if (lk_canon(A.col[c] + 8 * ia) != lk_canon(B.col[c] + 8 * ib)) return false;
  return true;
}

__global__ void __launch_bounds__(256) k_lk_insert(uint32_t* __restrict__ table, uint32_t mask, LookupCols T, uint64_t n) {
  KGS_AUX_PRIO();
  const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j64 >= n) return;
  const uint32_t j = (uint32_t)j64;
  uint32_t slot = (uint32_t)lk_hash_row(T, j) & mask;
  // at most n slots are ever occupied and the capacity is >= 2n: the walk ends
  for (;;) {
    // look before the CAS: a value read here was in the slot at some time, and a slot keeps its key, so
    // a row that finds an equal row of a lower index there is done without an atomic (a table of equal
    // rows would otherwise send every row's CAS and atomicMin to one address)
    uint32_t cur = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == LK_EMPTY) {
      cur = atomicCAS(table + slot, LK_EMPTY, j);
      if (cur == LK_EMPTY) return;
    }
    if (lk_rows_equal(T, cur, T, j)) {
      if (cur > j) atomicMin(table + slot, j);
      return;
    }
    slot = (slot + 1) & mask;
  }
}

// flags[0] = lowest selected row of F that is not in the table, flags[1] = lowest row whose selector
// is neither zero nor Montgomery one (both start at LK_EMPTY)
__global__ void __launch_bounds__(256) k_lk_probe(const uint32_t* __restrict__ table, uint32_t mask, LookupCols T,
                                                   LookupCols F, const uint32_t* __restrict__ sel_f, uint64_t n,
                                                   uint32_t* __restrict__ count, uint32_t* __restrict__ flags) {
  KGS_AUX_PRIO();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool pending = false;  // this lane found its row at table index idx and still owes the counter its 1
  uint32_t idx = 0;
  if (i < n) {
    bool selected = true;
    if (sel_f) {
      const fr s = fr::load(sel_f + 8 * i);
      selected = s == fr::one();
      if (!selected && !s.is_zero()) atomicMin(flags + 1, (uint32_t)i);
    }
    if (selected) {
      uint32_t slot = (uint32_t)lk_hash_row(F, i) & mask;
      for (;;) {  // the table has at least n empty slots: the walk ends
        idx = table[slot];
        if (idx == LK_EMPTY) {
          atomicMin(flags, (uint32_t)i);
          break;
        }
        if (lk_rows_equal(T, idx, F, i)) {
          pending = true;
          break;
        }
        slot = (slot + 1) & mask;
      }
    }
  }
  // Two rounds of "the first pending lane collects every lane with its target": one atomic per wave
  // when all rows of F are equal, and the hot row of a skewed F leaves in one of the rounds more often
  // than not. Whoever is left adds its own 1.
  const uint32_t lane = threadIdx.x & 63;
  for (int r = 0; r < 2; r++) {
    const unsigned long long pend = __ballot(pending);
    if (!pend) break;
    const int leader = __ffsll(pend) - 1;
    const uint32_t lidx = (uint32_t)__shfl((int)idx, leader);
    const bool same = pending && idx == lidx;
    const unsigned long long m = __ballot(same);
    if (lane == (uint32_t)leader) atomicAdd(count + lidx, (uint32_t)__popcll(m));
    if (same) pending = false;
  }
  if (pending) atomicAdd(count + idx, 1u);
}

__global__ void __launch_bounds__(256) k_lk_write(uint32_t* __restrict__ out, const uint32_t* __restrict__ count, uint64_t n) {
  KGS_AUX_PRIO();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  fr c = fr::zero();
  c.v[0] = count[j];
  c.to_mont().store(out + 8 * j);
}

void launch_lookup_multiplicities(hipStream_t st, uint32_t* out, uint32_t* table, uint64_t capacity, uint32_t* count,
                                  uint32_t* flags, const LookupCols& F, const LookupCols& T, const uint32_t* sel_f,
                                  uint64_t n) {
  const uint32_t mask = (uint32_t)(capacity - 1);
  hipLaunchKernelGGL(k_lk_insert, dim3(nb(n)), dim3(256), 0, st, table, mask, T, n);
  hipLaunchKernelGGL(k_lk_probe, dim3(nb(n)), dim3(256), 0, st, table, mask, T, F, sel_f, n, count, flags);
  hipLaunchKernelGGL(k_lk_write, dim3(nb(n)), dim3(256), 0, st, out, count, n);
}

}  // namespace kgs
