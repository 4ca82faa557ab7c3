// Stand-alone driver of the in-process rank group's host rendezvous (csrc/rank_rendezvous.hpp: the
// generation barrier with its time-out, abort, and the host all-gather over published pointers), built by
// tests/native/Makefile under -fsanitize=thread and under -fsanitize=address,undefined and run by
// tests/test_host_sanitizers.py (TEST INFRASTRUCTURE).
//
// W = 4 threads, one per rank, through four phases:
//   all-gather  2,000 rounds with per-round, per-rank payloads of 1, 4 and 252 bytes (252: the verdict
//               record of dist_preconditions); every rank checks every byte it received
//   abort       rank 3 calls abort() instead of arriving at round 1,000: the other three leave with
//               KGS_E_COMM "rank group aborted", and every later call on the object fails the same way at once
//   time-out    0.2 s, rank 3 never arrives: the others leave with "rank group barrier timed out" within a
//               few time-outs, and the object stays broken
//   W = 1       every call returns at once
// Only the time-out phase waits on the clock. Exit status 0: every check held; 1: a mismatch (on stderr).
//
// Under the thread sanitizer only: libstdc++ implements condition_variable::wait_for on the steady clock
// with pthread_cond_clockwait, which GCC 11's sanitizer runtime does not intercept, so it never sees the
// wait release the mutex and reports a "double lock" at the next barrier. Without the macro below the same
// wait_for goes through pthread_cond_timedwait, which it does intercept. The barrier's own code is the same.
#if defined(__SANITIZE_THREAD__) && __has_include(<bits/c++config.h>)
#include <bits/c++config.h>
#undef _GLIBCXX_USE_PTHREAD_COND_CLOCKWAIT
#endif
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../kzg-grandsums-study_amd/csrc/rank_rendezvous.hpp"

using kgs::KgsError;
using kgsi::RankRendezvous;

namespace {

const int W = 4;
const size_t SIZES[3] = {1, 4, 252};
std::atomic<int> g_failures{0};

void fail(const char* phase, int rank, int round, const std::string& what) {
  fprintf(stderr, "rank_rendezvous_check: %s, rank %d, round %d: %s\n", phase, rank, round, what.c_str());
  g_failures.fetch_add(1);
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

uint8_t payload_byte(int round, int rank, size_t i) { return (uint8_t)(round * 31 + rank * 7 + (int)i * 13 + 1); }

// one all-gather round of rank `rank`, every received byte checked
void gather_round(RankRendezvous& rv, int world, const char* phase, int rank, int round) {
  const size_t bytes = SIZES[round % 3];
  std::vector<uint8_t> send(bytes), recv(bytes * world, 0);
  for (size_t i = 0; i < bytes; i++) send[i] = payload_byte(round, rank, i);
  rv.allgather(rank, send.data(), recv.data(), bytes);
  for (int j = 0; j < world; j++)
    for (size_t i = 0; i < bytes; i++)
      if (recv[j * bytes + i] != payload_byte(round, j, i)) {
        fail(phase, rank, round, "byte " + std::to_string(i) + " from rank " + std::to_string(j) + " is wrong");
        return;
      }
}

// the call must throw KGS_E_COMM with exactly `msg`, within `within_s` seconds
template <class Fn>
void expect_comm_error(const char* phase, int rank, int round, const char* msg, double within_s, Fn fn) {
  const auto t0 = std::chrono::steady_clock::now();
  try {
    fn();
    fail(phase, rank, round, std::string("returned, expected \"") + msg + "\"");
  } catch (const KgsError& e) {
    if (e.code != KGS_E_COMM || strcmp(e.what(), msg))
      fail(phase, rank, round, std::string("threw \"") + e.what() + "\", expected \"" + msg + "\"");
  }
  const double s = seconds_since(t0);
  if (s > within_s) fail(phase, rank, round, "took " + std::to_string(s) + " s");
}

template <class Fn>
void run_ranks(int world, Fn fn) {
  std::vector<std::thread> th;
  for (int r = 0; r < world; r++) th.emplace_back(fn, r);
  for (auto& t : th) t.join();
}

void phase_allgather() {
  RankRendezvous rv(W, 60.0);
  run_ranks(W, [&](int rank) {
    try {
      for (int round = 0; round < 2000; round++) gather_round(rv, W, "all-gather", rank, round);
    } catch (const KgsError& e) {
      fail("all-gather", rank, -1, std::string("threw \"") + e.what() + "\"");
    }
  });
}

void phase_abort() {
  const int AT = 1000;
  RankRendezvous rv(W, 60.0);
  run_ranks(W, [&](int rank) {
    int round = 0;
    try {
      for (; round < 2 * AT; round++) {
        if (rank == W - 1 && round == AT) {
          rv.abort();
          break;
        }
        gather_round(rv, W, "abort", rank, round);
      }
      if (rank != W - 1) fail("abort", rank, round, "went on past the aborted round");
    } catch (const KgsError& e) {
      // a rank still leaving round AT - 1's last barrier when the abort lands reports it there
      if (rank == W - 1 || e.code != KGS_E_COMM || strcmp(e.what(), "rank group aborted") || round < AT - 1 || round > AT)
        fail("abort", rank, round, std::string("threw \"") + e.what() + "\"");
    }
    // every later call on the same object fails the same way at once, on every rank
    uint8_t b = 0, all[W];
    expect_comm_error("abort", rank, -1, "rank group aborted", 1.0, [&] { rv.barrier(); });
    expect_comm_error("abort", rank, -1, "rank group aborted", 1.0, [&] { rv.allgather(rank, &b, all, 1); });
  });
}

void phase_timeout() {
  const double T = 0.2;
  RankRendezvous rv(W, T);
  run_ranks(W, [&](int rank) {
    if (rank == W - 1) return;  // never arrives
    expect_comm_error("time-out", rank, 0, "rank group barrier timed out", 5 * T, [&] { rv.barrier(); });
  });
  // the object stays broken
  uint8_t b = 0, all[W];
  expect_comm_error("time-out", 0, 1, "rank group aborted", 1.0, [&] { rv.barrier(); });
  expect_comm_error("time-out", W - 1, 1, "rank group aborted", 1.0, [&] { rv.allgather(W - 1, &b, all, 1); });
}

void phase_world1() {
  RankRendezvous rv(1, 60.0);
  const auto t0 = std::chrono::steady_clock::now();
  try {
    for (int round = 0; round < 100; round++) {
      rv.barrier();
      gather_round(rv, 1, "W = 1", 0, round);
    }
  } catch (const KgsError& e) {
    fail("W = 1", 0, -1, std::string("threw \"") + e.what() + "\"");
  }
  if (seconds_since(t0) > 1.0) fail("W = 1", 0, -1, "calls did not return at once");
}

}  // namespace

int main() {
  phase_allgather();
  phase_abort();
  phase_timeout();
  phase_world1();
  const int f = g_failures.load();
  printf("rank_rendezvous_check %s (%d mismatches)\n", f ? "FAILED" : "ok", f);
  return f ? 1 : 0;
}
