// The host copy engine (host_copy.hpp): par_copy and stream_copy over a persistent pool of threads.
// Standard C++ and SSE2 only: no HIP call is made here, on any thread.
#include "host_copy.hpp"

#include <immintrin.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>

namespace kgsi {
// host copies between pageable caller buffers and the pinned staging area, split over threads; the
// 16 threads (a GPU's host share) are divided among the contexts copying at the same time, so that
// several proofs in flight through the host-buffer boundary do not oversubscribe the cores. The
// helpers are a persistent pool (spawning 8-16 threads per call cost ~0.1 ms, paid several times per
// proof once inputs are fed in pieces); the calling thread copies too, so a busy pool never stalls it.
static std::atomic<int> g_copy_active{0};
// host threads for the staging copies of all contexts together (KGS_COPY_THREADS, default 16: a GPU's
// share of the host's cores)
static unsigned copy_threads() {
  static const unsigned n = [] {
    const char* e = getenv("KGS_COPY_THREADS");
    const int v = e ? atoi(e) : 16;
    return (unsigned)(v >= 1 && v <= 64 ? v : 16);
  }();
  return n;
}
namespace {
// The staging copy's stores: cached (memcpy) or 16 B non-temporal. NT stores bypass the caches and
// copy a 32 MiB vector into pinned staging in 0.26 ms with 4 threads against 0.44 ms for memcpy
// (profiles/ubench/host_copy_bw.cpp, profiles/r06/host_copy_bw.txt), but then the H2D DMA reads the
// staging from DRAM instead of the host's L3, and F's DMA, not its copy, is what a lone proof waits
// for. Measured (same boxes, interleaved): a lone proof through the JavaScript module is faster with
// cached stores, median 15.1-16.1 vs 16.8-17.8 ms (4 x 15 samples, profiles/r06/js_lat_ab.txt; again
// 15.7-16.6 vs 16.9-17.9, profiles/r06/copy_final_ab/). Four proofs in flight are faster with NT
// stores, 0.9727 vs 0.9664 of device-resident (12 samples each, profiles/r06/inflight_store_ab/). So by
// default (KGS_COPY_NT unset) a copy uses NT stores when another proof of the process is in progress,
// cached stores when its proof is alone; KGS_COPY_NT=0 / 1 forces one kind. With NT stores the sfence
// makes the lines globally visible before the piece is counted done, i.e. before its DMA is enqueued.
std::atomic<int> g_proofs_active{0};  // kgs_prove calls in progress in the process (ProofInProgress)
bool copy_nt_now() {
  static const int mode = [] {
    const char* e = getenv("KGS_COPY_NT");
    return e && e[0] == '1' ? 1 : e && e[0] == '0' ? 0 : -1;
  }();
  return mode == 1 || (mode < 0 && g_proofs_active.load(std::memory_order_relaxed) > 1);
}
void copy_stores(uint8_t* d, const uint8_t* s, size_t n, bool nt) {
  if (!nt) {
    memcpy(d, s, n);
    return;
  }
  size_t i = 0;
  const size_t head = (16 - ((uintptr_t)d & 15)) & 15;
  if (head) {
    const size_t h = std::min(head, n);
    memcpy(d, s, h);
    i = h;
  }
  for (; i + 64 <= n; i += 64) {
    const __m128i a = _mm_loadu_si128((const __m128i*)(s + i)), b = _mm_loadu_si128((const __m128i*)(s + i + 16));
    const __m128i c = _mm_loadu_si128((const __m128i*)(s + i + 32)), e = _mm_loadu_si128((const __m128i*)(s + i + 48));
    _mm_stream_si128((__m128i*)(d + i), a);
    _mm_stream_si128((__m128i*)(d + i + 16), b);
    _mm_stream_si128((__m128i*)(d + i + 32), c);
    _mm_stream_si128((__m128i*)(d + i + 48), e);
  }
  if (i < n) memcpy(d + i, s + i, n - i);
  _mm_sfence();
}

// Invariants (DESIGN.md §13 "The round-5 illegal-address fault"): a piece is claimed exactly once,
// before par_copy / stream_copy returns, and pool threads make no HIP call (every DMA is enqueued by
// the thread that owns the call). Queue entries outlive their task (a helper that wakes late pops a
// finished task): such a late `work()` must claim nothing, which `closed` checks.
struct CopyTask {
  std::vector<CopyJob> pieces;
  std::atomic<size_t> next{0}, done{0};
  std::atomic<bool> closed{false};  // set once the owner has seen every piece done
  // stream_copy: pieces left to copy per DMA piece (piece i belongs to DMA piece i / per_dma)
  std::unique_ptr<std::atomic<uint32_t>[]> left;
  size_t per_dma = 0;
  bool nt = false;  // non-temporal stores (decided once per copy: copy_nt_now)
  std::mutex mu;
  std::condition_variable cv;
  bool copy_one(size_t i) {  // false: nothing left to claim
    if (i >= pieces.size()) return false;
    if (closed.load(std::memory_order_acquire)) {
      fprintf(stderr, "kgs: copy piece %zu claimed after its task completed\n", i);
      abort();
    }
    copy_stores(pieces[i].dst, pieces[i].src, pieces[i].len, nt);
    if (left) left[i / per_dma].fetch_sub(1, std::memory_order_release);
    return true;
  }
  void work() {
    size_t mine = 0;
    while (copy_one(next.fetch_add(1))) mine++;
    if (mine && done.fetch_add(mine) + mine == pieces.size()) {
      std::lock_guard<std::mutex> lk(mu);
      cv.notify_all();
    }
  }
};
struct CopyPool {  // leaked on purpose: its detached threads outlive static destruction
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::shared_ptr<CopyTask>> q;
  explicit CopyPool(unsigned n) {
    for (unsigned t = 0; t < n; t++)
      std::thread([this] {
        for (;;) {
          std::shared_ptr<CopyTask> task;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !q.empty(); });
            task = std::move(q.back());
            q.pop_back();
          }
          task->work();
        }
      }).detach();
  }
  static CopyPool& get() {
    static CopyPool* p = new CopyPool(copy_threads());
    return *p;
  }
};
struct Active {  // copies running at once in the process: they share the copy threads
  int n;
  Active() : n(g_copy_active.fetch_add(1) + 1) {}
  ~Active() { g_copy_active.fetch_sub(1); }
};
// threads (this one included) for one copy: KGS_COPY_TASK_THREADS (default 2), within the share of
// the copy threads left by the other copies running. The host copy bandwidth of the GPU box peaks at
// 2-4 threads (profiles/r06/host_copy_bw.txt), but the proof does not get faster with it: F_0's DMA,
// not its copy, sets its arrival. Same-box A/Bs (profiles/r06/copy_ab*, f0_ab): single-proof median
// 14.43 ms with 2 threads, 14.82 with 4, 14.54 for round 5's span-by-span copy; in flight all within
// the run-to-run spread (87.7-90.8 proofs/s against 92.7-93.1 device-resident)
unsigned task_threads(const Active& a, size_t pieces) {
  static const unsigned per = [] {
    const char* e = getenv("KGS_COPY_TASK_THREADS");
    const int v = e ? atoi(e) : 2;
    return (unsigned)(v >= 1 && v <= 64 ? v : 2);
  }();
  unsigned nth = std::min(per, std::max(1u, copy_threads() / (unsigned)std::max(1, a.n)));
  return std::max(1u, std::min<unsigned>(nth, (unsigned)pieces));
}
void start_helpers(const std::shared_ptr<CopyTask>& task, unsigned nth) {
  if (nth <= 1) return;
  CopyPool& pool = CopyPool::get();
  {
    std::lock_guard<std::mutex> lk(pool.mu);
    for (unsigned t = 1; t < nth; t++) pool.q.push_back(task);  // helpers; the calling thread is the nth
  }
  pool.cv.notify_all();
}
}  // namespace

ProofInProgress::ProofInProgress() { g_proofs_active.fetch_add(1, std::memory_order_relaxed); }
ProofInProgress::~ProofInProgress() { g_proofs_active.fetch_sub(1, std::memory_order_relaxed); }

void par_copy(const std::vector<CopyJob>& jobs) {
  const size_t piece = 1u << 20;
  auto task = std::make_shared<CopyTask>();
  task->nt = copy_nt_now();
  for (const auto& j : jobs)
    for (size_t o = 0; o < j.len; o += piece) task->pieces.push_back({j.dst + o, j.src + o, std::min(piece, j.len - o)});
  Active active;
  start_helpers(task, task_threads(active, task->pieces.size()));
  task->work();
  std::unique_lock<std::mutex> lk(task->mu);
  task->cv.wait(lk, [&] { return task->done.load() == task->pieces.size(); });
  task->closed.store(true, std::memory_order_release);
}

// One vector into pinned staging, copied in 256 KiB pieces claimed in address order by this thread
// and the pool's helpers; `ready(offset, len)` runs on THIS thread for each `dma`-byte span, in order,
// as soon as every piece of it is copied (it enqueues that span's DMA). So the first DMA starts after
// one span's copy and the link is fed while the rest is still being copied, at the copy bandwidth of
// several threads (round 5 copied span by span with two threads each, ~1.2 ms for a 32 MiB vector).
// An exception from `ready` is held until every piece is copied (helpers never outlive the call's
// writes into the staging), then rethrown; later spans are not enqueued.
void stream_copy(uint8_t* dst, const uint8_t* src, size_t len, size_t dma, const std::function<void(size_t, size_t)>& ready) {
  const size_t sub = (size_t)256 << 10;
  dma = std::max(sub, dma / sub * sub);
  auto task = std::make_shared<CopyTask>();
  task->nt = copy_nt_now();
  for (size_t o = 0; o < len; o += sub) task->pieces.push_back({dst + o, src + o, std::min(sub, len - o)});
  const size_t ndma = (len + dma - 1) / dma;
  task->per_dma = dma / sub;
  task->left.reset(new std::atomic<uint32_t>[ndma]);
  for (size_t k = 0; k < ndma; k++)
    task->left[k].store((uint32_t)std::min(task->per_dma, task->pieces.size() - k * task->per_dma));
  Active active;
  start_helpers(task, task_threads(active, task->pieces.size()));
  size_t issued = 0, mine = 0;
  std::exception_ptr err;
  auto flush = [&] {
    while (issued < ndma && task->left[issued].load(std::memory_order_acquire) == 0) {
      const size_t o = issued * dma;
      if (!err) {
        try {
          ready(o, std::min(dma, len - o));
        } catch (...) {
          err = std::current_exception();
        }
      }
      issued++;
    }
  };
  while (task->copy_one(task->next.fetch_add(1))) {
    mine++;
    flush();
  }
  if (mine) task->done.fetch_add(mine);
  while (issued < ndma) {  // the helpers' last pieces (each at most one 256 KiB copy away)
    flush();
    if (issued < ndma) _mm_pause();
  }
  task->closed.store(true, std::memory_order_release);
  if (err) std::rethrow_exception(err);
}

}  // namespace kgsi
