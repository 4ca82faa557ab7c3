// Stand-alone driver of the host copy engine (csrc/host_copy.cpp: par_copy, stream_copy and the pool
// behind them), built by tests/native/Makefile under -fsanitize=thread and under
// -fsanitize=address,undefined and run by tests/test_host_sanitizers.py (TEST INFRASTRUCTURE).
//
// Four threads run concurrently, so their copies share the pool's helpers and helpers wake after the
// task they were queued for has finished. Each thread goes through the lengths that reach every branch
// (no piece, one partial piece, either side of the 256 KiB piece, several DMA spans with a ragged tail),
// each at destination offset 0 and 1 (the unaligned head of the non-temporal store loop), and checks
// what kgs_prove relies on. Exit status 0: every check held; 1: a mismatch (named on stderr).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../kzg-grandsums-study_amd/csrc/host_copy.hpp"

using kgsi::par_copy;
using kgsi::stream_copy;

namespace {

const size_t PIECE = (size_t)256 << 10;
const uint8_t GUARD = 0xA5;
std::atomic<int> g_failures{0};

void fail(int thread, size_t len, size_t off, const char* what) {
  fprintf(stderr, "host_copy_check: thread %d len %zu offset %zu: %s\n", thread, len, off, what);
  g_failures.fetch_add(1);
}

struct Case {
  int thread;
  size_t len, off;
  std::vector<uint8_t> src, buf;  // buf: `off` bytes, the destination, one guard byte
  Case(int t, size_t l, size_t o) : thread(t), len(l), off(o), src(l), buf(o + l + 1) {
    uint32_t x = 0x9E3779B9u * (uint32_t)(t + 1) + (uint32_t)l;
    for (size_t i = 0; i < l; i++) {
      x = x * 1664525u + 1013904223u;
      src[i] = (uint8_t)(x >> 24);
    }
  }
  uint8_t* dst() { return buf.data() + off; }
  void clear() {
    memset(buf.data(), 0, buf.size());
    buf[off + len] = GUARD;
  }
  void check_whole(const char* what) {
    if (len && memcmp(dst(), src.data(), len)) fail(thread, len, off, what);
    if (buf[off + len] != GUARD) fail(thread, len, off, "the byte after the destination was written");
  }

  // spans of `span` bytes asked for, `dma` bytes expected (the span in whole pieces, at least one); the
  // ready callback throws at its call number `throw_at` (-1: never)
  void stream(size_t span, size_t dma, int throw_at) {
    clear();
    size_t next = 0;
    int calls = 0;
    bool thrown = false;
    try {
      stream_copy(dst(), src.data(), len, span, [&](size_t o, size_t l) {
        const int call = calls++;
        if (call == throw_at) throw std::runtime_error("injected");
        if (o != next) fail(thread, len, off, "spans are not contiguous and ascending");
        if (o >= len || l != (len - o < dma ? len - o : dma)) fail(thread, len, off, "span of the wrong length");
        else if (memcmp(dst() + o, src.data() + o, l)) fail(thread, len, off, "span reported before it was copied");
        next = o + l;
      });
    } catch (const std::runtime_error&) {
      thrown = true;
    }
    const size_t nspans = (len + dma - 1) / dma;
    if (throw_at < 0) {
      if (thrown) fail(thread, len, off, "exception without a throwing callback");
      if (next != len || (size_t)calls != nspans) fail(thread, len, off, "spans do not cover [0, len) exactly");
    } else {
      const size_t want_calls = nspans < (size_t)throw_at + 1 ? nspans : (size_t)throw_at + 1;
      if (thrown != (nspans > (size_t)throw_at)) fail(thread, len, off, "exception did not reach the caller exactly when thrown");
      if ((size_t)calls != want_calls) fail(thread, len, off, "a span was reported after the callback threw");
    }
    check_whole("stream_copy left bytes uncopied");
  }

  void par() {
    clear();
    const size_t h = len / 2;
    par_copy({{dst(), src.data(), h}, {dst() + h, src.data() + h, len - h}});
    check_whole("par_copy: destination differs from the source");
  }
};

void run_thread(int t) {
  const size_t lens[] = {0, 1, 15, PIECE - 1, PIECE + 1, ((size_t)3 << 20) + 17};
  for (size_t len : lens)
    for (size_t off = 0; off < 2; off++) {
      Case c(t, len, off);
      c.stream(2 * PIECE, 2 * PIECE, -1);
      c.stream(4096, PIECE, -1);  // clamped up to one piece
      c.stream(2 * PIECE, 2 * PIECE, 1);
      c.par();
    }
}

}  // namespace

int main() {
  std::vector<std::thread> th;
  for (int t = 0; t < 4; t++) th.emplace_back(run_thread, t);
  for (auto& x : th) x.join();
  const int f = g_failures.load();
  printf("host_copy_check %s (%d mismatches)\n", f ? "FAILED" : "ok", f);
  return f ? 1 : 0;
}
