// The thread mapping of the batched G1 transform stage (g1ntt.hip k_g1ntt_stage_many): `polys`
// transforms of size n = 2^logn side by side, transform p over the points [p n, (p + 1) n), all at stage
// h = 2^logh with G = n / 2h groups each. No HIP header needed: the kernel and the host launch code index with
// these functions, and tests/native/g1ntt_map_dump.cpp enumerates them without a GPU.
//
// Uniform mapping: a block of 64 lanes holds one t. The polys * G butterflies that share t are numbered
// q = p G + g and cut into chunks of 64; block = t * chunks + chunk, the last chunk of a t may have idle lanes.
// The wave's twiddle record is then one (g1ntt_mul<true>), whatever G is: a small transform gets from the
// polynomial dimension what a large one gets from its groups. Taken when polys * G >= 64 and t is not always 0.
// Per-lane mapping: butterfly i -> (p, g, t) = (i / (n/2), (i % (n/2)) / h, i % h), adjacent lanes adjacent
// points, as k_g1ntt_stage's; only the last block has idle lanes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KGS_HD __host__ __device__
#else
#define KGS_HD
#endif

namespace kgs {

constexpr uint32_t G1NTT_MANY_BLOCK = 64;  // lanes per block: one wave

struct G1NttBfly {
  bool active;    // false: an idle lane, nothing below is in range
  uint64_t poly;  // which transform
  uint32_t g, t;  // group and twiddle exponent within it: t < h
  uint64_t pa, pb;  // the points of the butterfly, of polys * n: poly n + g 2h + t, and h above
  uint64_t tw;    // the twiddle's index in the table of the transform's n / 2 powers of its root: t G
};

KGS_HD inline bool g1ntt_many_uniform(uint64_t polys, int logn, int logh) {
  return logh > 0 && (polys << (logn - 1 - logh)) >= G1NTT_MANY_BLOCK;
}

// blocks of 64 lanes of one stage
KGS_HD inline uint64_t g1ntt_many_blocks(uint64_t polys, int logn, int logh, bool uniform) {
  if (uniform) {
    const uint64_t per_t = polys << (logn - 1 - logh);
    return ((per_t + G1NTT_MANY_BLOCK - 1) / G1NTT_MANY_BLOCK) << logh;
  }
  return ((polys << (logn - 1)) + G1NTT_MANY_BLOCK - 1) / G1NTT_MANY_BLOCK;
}

KGS_HD inline G1NttBfly g1ntt_many_map(uint64_t block, uint32_t lane, uint64_t polys, int logn, int logh, bool uniform) {
  const int logG = logn - 1 - logh;
  G1NttBfly b;
  if (uniform) {
    const uint64_t per_t = polys << logG, chunks = (per_t + G1NTT_MANY_BLOCK - 1) / G1NTT_MANY_BLOCK;
    const uint64_t q = (block % chunks) * G1NTT_MANY_BLOCK + lane;
    b.t = (uint32_t)(block / chunks);
    b.active = q < per_t && b.t < (1u << logh);
    b.poly = q >> logG;
    b.g = (uint32_t)(q & ((1ull << logG) - 1));
  } else {
    const uint64_t i = block * G1NTT_MANY_BLOCK + lane, within = i & ((1ull << (logn - 1)) - 1);
    b.poly = i >> (logn - 1);
    b.active = b.poly < polys;
    b.g = (uint32_t)(within >> logh);
    b.t = (uint32_t)(within & ((1ull << logh) - 1));
  }
  b.pa = (b.poly << logn) + ((uint64_t)b.g << (logh + 1)) + b.t;
  b.pb = b.pa + (1ull << logh);
  b.tw = (uint64_t)b.t << logG;
  return b;
}

}  // namespace kgs
