// The host rendezvous of an in-process rank group (dist_group.cpp LocalGroup: several contexts of one
// process, one host thread per rank): a generation barrier with a time-out, the broken / abort state and
// the published-pointer table with the host all-gather built on it. No HIP here, so that this protocol —
// with host_copy.cpp the only hand-written concurrent code of the library — builds and runs alone under
// the thread and address sanitizers (tests/native/rank_rendezvous_check.cpp).
//
// Once a rank has timed out in a barrier or called abort(), the object is broken for good: every rank
// waiting in it leaves with KGS_E_COMM ("rank group barrier timed out" or "rank group aborted"), and every
// later call fails with "rank group aborted" at once.
#pragma once
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "../../include/kgs.h"
#include "host_error.hpp"

namespace kgsi {

struct RankRendezvous {
  const int world;
  const double timeout_s;  // what a rank waits for its peers in one barrier
  // what each rank published for the exchange in progress: written by its rank before a barrier, read
  // by the others after it
  std::vector<const void*> sp;

  RankRendezvous(int w, double timeout) : world(w), timeout_s(timeout), sp(w) {}

  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    if (broken) throw kgs::KgsError(KGS_E_COMM, "rank group aborted");
    const uint64_t g = gen;
    if (++arrived == world) {
      arrived = 0;
      gen++;
      cv.notify_all();
      return;
    }
    if (!cv.wait_for(lk, std::chrono::duration<double>(timeout_s), [&] { return gen != g || broken; })) {
      broken = timed_out = true;
      cv.notify_all();
    }
    // a rank that a peer's time-out released waited for the same missing rank: it reports the time-out too
    if (broken) throw kgs::KgsError(KGS_E_COMM, timed_out ? "rank group barrier timed out" : "rank group aborted");
  }
  void abort() {
    std::lock_guard<std::mutex> lk(mu);
    broken = true;
    cv.notify_all();
  }
  // blocking host all-gather: recv = world x bytes, rank-major
  void allgather(int rank, const void* send, void* recv, size_t bytes) {
    sp[rank] = send;
    barrier();
    for (int j = 0; j < world; j++) memcpy((uint8_t*)recv + (size_t)j * bytes, sp[j], bytes);
    barrier();  // the senders' buffers stay valid until every rank has copied
  }

 private:
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool broken = false, timed_out = false;
};

}  // namespace kgsi
