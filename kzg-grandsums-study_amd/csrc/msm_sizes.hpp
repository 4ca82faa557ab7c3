// The constants of the MSM kernels (msm.hip) that decide how large the work buffers are, and the one
// function that sizes them for both drivers (msm_run, msm_points_run). No HIP header needed. The kernels
// index with these constants and the host allocates with them, so a variant build (-DKGS_SL_CHUNK,
// -DKGS_SL_G, -DKGS_SORT_SPT) resizes both sides together.
#pragma once
#include <stdint.h>

namespace kgs {

#ifndef KGS_SORT_SPT
#define KGS_SORT_SPT 2
#endif
#ifndef KGS_SL_CHUNK
#define KGS_SL_CHUNK 16384
#endif
#ifndef KGS_SL_G
#define KGS_SL_G 64
#endif
constexpr int SORT_SPT = KGS_SORT_SPT;       // scalars per thread in the histogram / partition passes
constexpr uint32_t SL_CHUNK = KGS_SL_CHUNK;  // lo pass: entries per chunk (= its LDS tile)
constexpr int SL_G = KGS_SL_G;               // lo pass: most chunks per partition
constexpr uint32_t CB_T = 16;                // partials per thread per combine level
constexpr int CB_LEVELS = 3;
constexpr int RAW29_WORDS = 40;              // g1_acc29::store_raw / load_raw record (field29.hpp)
constexpr int NH_MAX = 2048;                 // most bucket-sort partitions
constexpr uint64_t MSM_SEG_MAX = 1ull << 18;  // most segments of the bucket accumulation (msm_buckets)
constexpr uint64_t MSM_SEG_MIN_LEN = 4;       // fewest sorted entries per segment

// Bucket sort with window c: LOB low bits of key - 1 are sorted inside a partition (<= 8: the lo pass
// keeps them in a byte), the other c - 1 - LOB bits select one of NH = 2^(c-1-LOB) partitions: 256 for
// 16 <= c <= 17, 512 / 1024 / 2048 = NH_MAX for c = 18 / 19 / 20
inline int msm_lob(int c) {
  int lob = c - 1 < 7 ? c - 1 : 7;
  if (c - 9 > lob) lob = c - 9 > 8 ? 8 : c - 9;
  return lob;
}
inline int msm_nh(int c) { return (1 << (c - 1)) >> msm_lob(c); }
inline int msm_windows(int c) { return (255 + c - 1) / c; }
// window of the sort that holds the variable-base key space [1, W * 2^(c-1)]: 2^(cs-1) >= W * 2^(c-1)
inline int msm_points_c_sort(int c) {
  const uint64_t keys = (uint64_t)msm_windows(c) << (c - 1);
  int lg = 0;
  while ((1ull << lg) < keys) lg++;
  return lg + 1 < 7 ? 7 : lg + 1;
}
// blocks of the histogram / partition passes over N scalars
inline uint32_t msm_sort_blocks(uint64_t N) { return (uint32_t)((N + 256 * SORT_SPT - 1) / (256 * SORT_SPT)); }
// dynamic LDS of k_sort_part: 256 * SORT_SPT * W staged entries (4 B value, 2 B partition, 1 B lo)
// and the block's base / offset / cursor per partition
inline uint64_t msm_part_lds(int W, int NH) { return (uint64_t)256 * SORT_SPT * W * 7 + (uint64_t)12 * NH; }
// lo-pass grid: an upper bound of sum_p clamp(ceil(size_p / SL_CHUNK), 1, SL_G) over NH partitions
// that hold E entries together (blocks past the real count exit)
inline uint64_t msm_chunk_bound(uint64_t E, int NH) {
  const uint64_t a = (uint64_t)NH * SL_G, b = NH + E / SL_CHUNK;
  return a < b ? a : b;
}
// row and column sums of one window's 2^(c-1) buckets: 2^h + 2^l lines, l = c / 2, h = c - 1 - l
inline uint32_t msm_tail_lines(int c) { return (1u << (c - 1 - c / 2)) + (1u << (c / 2)); }
// entries per segment of the bucket accumulation: one segment per resident accumulate thread, within the two limits
inline uint64_t msm_seg_len(uint64_t E, uint64_t resident) {
  uint64_t L = (E + resident - 1) / resident;
  if (L < MSM_SEG_MIN_LEN) L = MSM_SEG_MIN_LEN;
  if ((E + L - 1) / L > MSM_SEG_MAX) L = (E + MSM_SEG_MAX - 1) / MSM_SEG_MAX;
  return L;
}

// Bytes of the MsmWork buffers and of the T output for MSMs of up to N scalars. c: the digit window,
// W = ceil(255 / c) digits per scalar; cs: the sort's window (c for fixed base, msm_points_c_sort(c) for
// variable base); keys: buckets (2^(c-1), or W * 2^(c-1)); windows: bucket sets the tail reduces (1, or
// W). E = N * W bounds the sorted entries. Monotone in N: buffers for N serve every smaller MSM.
struct MsmSizes {
  uint64_t digit;      // k_sort_part tval[g], g < E
  uint64_t sorted;     // k_lo_scatter sorted[d0 + i] < E; k_sort_hist<VAR> std_out[8 i + k], i < N (W >= 8)
  uint64_t lo;         // k_sort_part tlo[g], g < E, and the 16-byte loads of k_lo_count
  uint64_t blockhist;  // k_sort_hist bh[p * nblk + block], p < NH, block < nblk
  uint64_t counts;     // k_sort_scan_blocks ptot[p], p < NH
  uint64_t offsets;    // k_lo_scatter offsets[(p << lob) + lo + 1] <= 2^(cs-1); k_sort_scan offsets[keys + 1]
  uint64_t cursor;     // hi_off and cpre at NH_MAX + 8 words each, then k_sort_scan bpart[b], b < msm_chunk_bound
  uint64_t segowner;   // k_accumulate segowner[s], s < nseg
  uint64_t locnt;      // k_lo_count locnt[((p << lob) + lo) * SL_G + g], g < SL_G
  uint64_t chunklist;  // combine_enqueue list j at j * lcap, lcap = nseg / CB_T + keys + 16, j < CB_LEVELS
  uint64_t raw29;      // k_accumulate run_rec(raw, keys + 1 + s), s < nseg
  uint64_t part;       // k_rowcol rc[RAW29_WORDS * (win * lines + line)]
  uint64_t T;          // k_bitsum_rc T[32 * (win * c + k)], k < c
  uint64_t total() const {
    return digit + sorted + lo + blockhist + counts + offsets + cursor + segowner + locnt + chunklist + raw29 + part;
  }
};
inline MsmSizes msm_work_sizes(uint64_t N, int c, int cs, uint64_t keys, int windows) {
  MsmSizes z;
  const uint64_t E = N * (uint64_t)msm_windows(c), NH = (uint64_t)msm_nh(cs), bsort = 1ull << (cs - 1);
  // msm_seg_len: L >= MSM_SEG_MIN_LEN and ceil(E / L) <= MSM_SEG_MAX, whatever the chip holds
  uint64_t nseg = (E + MSM_SEG_MIN_LEN - 1) / MSM_SEG_MIN_LEN;
  if (nseg > MSM_SEG_MAX) nseg = MSM_SEG_MAX;
  nseg += 2;
  z.digit = 4 * E;
  z.sorted = 4 * E;
  z.lo = E + 16;
  z.blockhist = 4 * NH * ((uint64_t)msm_sort_blocks(N) + 1);
  z.counts = 4 * (NH + 8);
  z.offsets = 4 * (bsort + 4);
  z.cursor = 4 * (2 * ((uint64_t)NH_MAX + 8) + msm_chunk_bound(E, (int)NH) + 64);
  z.segowner = 4 * nseg;
  z.locnt = 4 * bsort * SL_G;
  z.chunklist = 4 * (uint64_t)CB_LEVELS * (nseg / CB_T + keys + 16);
  z.raw29 = 4 * (uint64_t)RAW29_WORDS * (keys + 2 + nseg);
  z.part = 4 * (uint64_t)RAW29_WORDS * windows * msm_tail_lines(c);
  z.T = 128 * (uint64_t)windows * c;
  return z;
}

}  // namespace kgs
