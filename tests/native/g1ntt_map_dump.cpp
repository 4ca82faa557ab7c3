// Enumerates the thread mapping of the batched G1 transform stage (csrc/g1ntt_map.hpp) for the shapes named on
// the command line, every block and lane as the kernel launch forms them (tests/test_kzg_cosets_many_refs.py).
// Host-only: plain g++, no HIP.
// usage: g1ntt_map_dump <logn>:<logh>:<polys>:<a|l> ...   a: the mapping the library takes, l: per lane forced
// output, per shape: "S logn logh polys uniform blocks", then one line per block: its 64 lanes, space separated,
// each "poly,g,t,pa,pb,tw" or "-" for an idle lane
#include <stdio.h>
#include <stdlib.h>

#include "g1ntt_map.hpp"

using namespace kgs;

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    int logn = 0, logh = 0;
    unsigned long long polys = 0;
    char kind = 0;
    if (sscanf(argv[i], "%d:%d:%llu:%c", &logn, &logh, &polys, &kind) != 4 || (kind != 'a' && kind != 'l')) return 2;
    const bool uni = kind == 'a' && g1ntt_many_uniform(polys, logn, logh);
    const uint64_t blocks = g1ntt_many_blocks(polys, logn, logh, uni);
    printf("S %d %d %llu %d %llu\n", logn, logh, polys, uni ? 1 : 0, (unsigned long long)blocks);
    for (uint64_t b = 0; b < blocks; b++) {
      for (uint32_t lane = 0; lane < G1NTT_MANY_BLOCK; lane++) {
        const G1NttBfly m = g1ntt_many_map(b, lane, polys, logn, logh, uni);
        if (!m.active)
          printf("- ");
        else
          printf("%llu,%u,%u,%llu,%llu,%llu ", (unsigned long long)m.poly, m.g, m.t, (unsigned long long)m.pa,
                 (unsigned long long)m.pb, (unsigned long long)m.tw);
      }
      printf("\n");
    }
  }
  return 0;
}
