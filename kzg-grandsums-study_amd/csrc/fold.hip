// Segmented G1 linear combination for gfx950 (kgs.h kgs_g1_lincomb; the per-proof fold of
// kgs_verify_batch): out[s] = sum over the terms t of segment s of scalar_t * P_t.
//
// The points are used once (a proof's own commitments), so there are no window tables to read and
// nothing of msm.hip's Pippenger applies: a segment has a dozen terms.
//   k_fold_mul   one thread per term: double-and-add over the scalar's bits with the affine base
//                (madd, no per-thread table), XYZZ result per term;
//   k_fold_sum   one thread per segment adds its terms' results in order;
// then launch_batch_affine (msm.hip). One thread per SEGMENT sharing the doublings between its terms
// (Straus) does half the field products on a twelfth of the threads: measured 10x slower at 4096
// proofs and never faster below (DESIGN.md "Batch verifier"), so it is not built.
// Scalars are 32 B little-endian STANDARD form and may be any 256-bit integer (the group has prime
// order r, so s and s mod r give the same point); points are affine LEM on the curve, the zero point
// included. add / add_aff branch on the identity, on equal and on opposite operands, so equal
// summands and sums that cancel give the right point.
#include "kernels.hpp"

namespace kgs {

static inline unsigned nb(uint64_t work, unsigned bs = 256) { return (unsigned)((work + bs - 1) / bs); }

__global__ void __launch_bounds__(256) k_fold_mul(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ points,
                                                  const uint32_t* __restrict__ scalars, uint64_t nterms) {
  KGS_AUX_PRIO();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nterms) return;
  const g1_aff P = g1_aff::load(points + 16 * t);
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = scalars[8 * t + i];
  g1_xyzz acc = g1_xyzz::inf();
  if (!P.is_inf()) {
    int top = -1;
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (s[i]) top = 32 * i + 31 - __clz(s[i]);
    for (int i = top; i >= 0; i--) {
      acc = acc.dbl();
      uint32_t w = s[0];
#pragma unroll
      for (int k = 1; k < 8; k++)
        if ((i >> 5) == k) w = s[k];
      if ((w >> (i & 31)) & 1u) acc.add_aff(P);
    }
  }
  acc.store(out_xyzz + 32 * t);
}

__global__ void __launch_bounds__(256) k_fold_sum(uint32_t* __restrict__ out_xyzz, const uint32_t* __restrict__ term_xyzz,
                                                  const uint32_t* __restrict__ seg_off, uint64_t nseg) {
  KGS_AUX_PRIO();
  const uint64_t sgm = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sgm >= nseg) return;
  const uint32_t lo = seg_off[sgm], hi = seg_off[sgm + 1];
  g1_xyzz acc = g1_xyzz::inf();
  for (uint32_t t = lo; t < hi; t++) acc.add(g1_xyzz::load(term_xyzz + 32 * (uint64_t)t));
  acc.store(out_xyzz + 32 * sgm);
}

void launch_g1_fold(hipStream_t st, uint32_t* out_aff, const uint32_t* points, const uint32_t* scalars,
                    const uint32_t* seg_off, uint64_t nterms, uint64_t nseg, uint32_t* term_xyzz, uint32_t* seg_xyzz,
                    uint32_t* scratch) {
  if (!nseg) return;
  // one wave per workgroup: a few thousand terms spread over all CUs instead of filling a few
  if (nterms) hipLaunchKernelGGL(k_fold_mul, dim3(nb(nterms, 64)), dim3(64), 0, st, term_xyzz, points, scalars, nterms);
  hipLaunchKernelGGL(k_fold_sum, dim3(nb(nseg, 64)), dim3(64), 0, st, seg_xyzz, term_xyzz, seg_off, nseg);
  launch_batch_affine(st, out_aff, seg_xyzz, scratch, nseg);
}

}  // namespace kgs
