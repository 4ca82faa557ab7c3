// Prints the MSM sizing header's constants and msm_work_sizes for the shapes named on the command
// line, as one JSON document (tests/test_msm_sizes.py). Host-only: plain g++, no HIP.
// usage: msm_sizes_dump (f|v):<N>:<c> ...   f: fixed base, v: variable base
#include <stdio.h>
#include <stdlib.h>

#include "msm_sizes.hpp"

using namespace kgs;

int main(int argc, char** argv) {
  printf("{\"constants\": {\"SORT_SPT\": %d, \"SL_CHUNK\": %u, \"SL_G\": %d, \"CB_T\": %u, \"CB_LEVELS\": %d, "
         "\"RAW29_WORDS\": %d, \"NH_MAX\": %d, \"SEG_MAX\": %llu, \"SEG_MIN_LEN\": %llu},\n \"shapes\": [",
         SORT_SPT, SL_CHUNK, SL_G, CB_T, CB_LEVELS, RAW29_WORDS, NH_MAX, (unsigned long long)MSM_SEG_MAX,
         (unsigned long long)MSM_SEG_MIN_LEN);
  for (int i = 1; i < argc; i++) {
    char kind = 0;
    unsigned long long N = 0;
    int c = 0;
    if (sscanf(argv[i], "%c:%llu:%d", &kind, &N, &c) != 3 || (kind != 'f' && kind != 'v')) return 2;
    const bool var = kind == 'v';
    const int W = msm_windows(c), cs = var ? msm_points_c_sort(c) : c;
    const uint64_t keys = var ? (uint64_t)W << (c - 1) : 1ull << (c - 1);
    const MsmSizes z = msm_work_sizes(N, c, cs, keys, var ? W : 1);
    printf("%s\n  {\"var\": %s, \"N\": %llu, \"c\": %d, \"cs\": %d, \"lob\": %d, \"NH\": %d, \"total\": %llu, \"sizes\": {"
           "\"digit\": %llu, \"sorted\": %llu, \"lo\": %llu, \"blockhist\": %llu, \"counts\": %llu, \"offsets\": %llu, "
           "\"cursor\": %llu, \"segowner\": %llu, \"locnt\": %llu, \"chunklist\": %llu, \"raw29\": %llu, \"part\": %llu, "
           "\"T\": %llu}}",
           i > 1 ? "," : "", var ? "true" : "false", N, c, cs, msm_lob(cs), msm_nh(cs), (unsigned long long)z.total(),
           (unsigned long long)z.digit, (unsigned long long)z.sorted, (unsigned long long)z.lo,
           (unsigned long long)z.blockhist, (unsigned long long)z.counts, (unsigned long long)z.offsets,
           (unsigned long long)z.cursor, (unsigned long long)z.segowner, (unsigned long long)z.locnt,
           (unsigned long long)z.chunklist, (unsigned long long)z.raw29, (unsigned long long)z.part,
           (unsigned long long)z.T);
  }
  printf("\n]}\n");
  return 0;
}
