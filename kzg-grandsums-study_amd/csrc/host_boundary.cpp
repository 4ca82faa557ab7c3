// The host-buffer boundary of the C-ABI (include/kgs.h): kgs_prove over caller memory. Inputs are DMA'd
// in place from buffers the caller has pinned, staged all at once for a rank group, or staged piece by
// piece (host_copy.cpp) by a feeder thread while the prover (prover.cpp prove_impl) already runs; the
// Montgomery write-back goes the other way. Also: the pinning entry points, the copy engine's test hook.
#include <condition_variable>
#include <thread>

#include "context.hpp"

using namespace kgs;
using namespace kgsi;

namespace {

// The A/B knobs of the input feed, each read once (at the first proof); unset: the first alternative
const char* env(const char* name) {
  const char* e = getenv(name);
  return e ? e : "";
}
struct FeedKnobs {
  // KGS_STREAM_COPY=0: round 5's span-by-span copy (par_copy + DMA per span) instead of stream_copy
  const bool span_copy = env("KGS_STREAM_COPY")[0] == '0';
  // KGS_F0_SPAN_MB=<1..64>: DMA span of vector 0 (default 2 MiB)
  const int f0_mb = atoi(env("KGS_F0_SPAN_MB"));
  const size_t f0_span = (size_t)(f0_mb >= 1 && f0_mb <= 64 ? f0_mb : 2) << 20;
  // KGS_F0_STREAM=copy: F_0's DMAs on the copy stream too, the main stream waits on ev_in[0]
  const bool f0_on_copy = !strcmp(env("KGS_F0_STREAM"), "copy");
  // KGS_FEED_ORDER=0: the copy stream's DMAs may overlap F_0's instead of starting after them
  const bool ordered = env("KGS_FEED_ORDER")[0] != '0';
};
const FeedKnobs& feed_knobs() {
  static const FeedKnobs k;
  return k;
}

// Caller buffers the DMAs can read / write in place: memory the caller already pinned (hipHostMalloc,
// kgs_host_register) is used as it is and left alone, so a caller that keeps its buffers across
// proofs skips the staging copy. Registering pageable buffers per call (KGS_HOST_REGISTER=1) is kept
// as an opt-in only: measured at 2^20 it makes the host path slower, 21.5 vs 16.0 ms per proof, and
// the JS concurrent rate 44.9 vs 78.8 proofs/s (register + unregister of 2 x 32 MiB costs more than
// the ~1 ms copy it saves, and registrations serialise across contexts), profiles/r03/boundary_ab.txt.
// Per-call registrations are released after every stream of the context is drained (also on an error
// path). Concurrent calls may pass the same buffer (e.g. one selector vector shared by several
// proofs): the registrations are reference-counted process-wide, so the first call to finish does not
// unpin memory another call is still DMA-ing. Overlapping buffers with different starts fail to
// register and take the staging path.
std::mutex g_pin_mu;
std::map<void*, std::pair<size_t, int>> g_pins;  // start -> (bytes, calls holding it)
struct HostPins {
  kgs_ctx* ctx;
  std::vector<void*> mine;
  explicit HostPins(kgs_ctx* c) : ctx(c) {}
  static bool pinned_elsewhere(const void* p) {
    hipPointerAttribute_t a{};
    const bool ok = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // a pageable pointer is an error here: not a sticky launch error
    return ok;
  }
  bool pin(const void* cp, size_t n) {
    void* p = const_cast<void*>(cp);
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pins.find(p);
    if (it != g_pins.end()) {
      if (it->second.first < n) return false;
      it->second.second++;
      mine.push_back(p);
      return true;
    }
    if (pinned_elsewhere(p)) return true;  // the caller's own pinned memory: use, never unpin
    static const bool reg = getenv("KGS_HOST_REGISTER") != nullptr;  // opt-in, see above
    if (!reg) return false;
    if (hipHostRegister(p, n, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    g_pins[p] = {n, 1};
    mine.push_back(p);
    return true;
  }
  static void drop(void* p) {  // under g_pin_mu
    auto it = g_pins.find(p);
    if (it != g_pins.end() && --it->second.second == 0) {
      hipHostUnregister(p);
      g_pins.erase(it);
    }
  }
  void release_from(size_t k) {  // the pins made after the first k (no DMA issued on them yet)
    std::lock_guard<std::mutex> lk(g_pin_mu);
    while (mine.size() > k) {
      drop(mine.back());
      mine.pop_back();
    }
  }
  ~HostPins() {
    if (mine.empty()) return;
    hipSetDevice(ctx->device);
    for (const auto& s : ctx->streams())
      if (s.st) hipStreamSynchronize(s.st);
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (void* p : mine) drop(p);
  }
};

// One input vector of a proof, numbered as HostHooks numbers them (F_i at 2i, T_i at 2i + 1, then selF,
// selT): the caller's buffer, its slot in the pinned staging area, its device buffer.
struct InputVec {
  const uint8_t* src;
  uint8_t* slot;
  uint32_t* dst;
};

// the copy stream and one event per input vector; in.ready sized, all "already ordered"
void ensure_input_events(kgs_ctx* ctx, size_t n, ProveIn& in) {
  if (!ctx->st_copy) ctx->st_copy = copy_stream();
  while (ctx->ev_in.size() < n) {
    hipEvent_t e;
    HC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->ev_in.push_back(e);
  }
  in.ready.assign(n, nullptr);
}

// zero-copy, if every input is in pinned caller memory (else false, with nothing left pinned and nothing
// enqueued): each DMA'd straight from the caller's buffer, one after the other on the copy stream (not
// two streams at once: F_0 then arrives after one vector's transfer time instead of sharing the link
// with T_0), each with the event its first kernel waits for
bool feed_in_place(kgs_ctx* ctx, HostPins& pins, const std::vector<InputVec>& ins, size_t E, ProveIn& in) {
  for (const InputVec& iv : ins)
    if (!pins.pin(iv.src, E)) {
      pins.release_from(0);
      return false;
    }
  ensure_input_events(ctx, ins.size(), in);
  for (size_t v = 0; v < ins.size(); v++) {
    HC(hipMemcpyAsync(ins[v].dst, ins[v].src, E, hipMemcpyHostToDevice, ctx->st_copy));
    HC(hipEventRecord(ctx->ev_in[v], ctx->st_copy));
    in.ready[v] = ctx->ev_in[v];
  }
  return true;
}

// the distributed prover reads every input at once: one parallel host copy into the pinned slots, then
// one DMA per vector
void feed_group(kgs_ctx* ctx, const std::vector<InputVec>& ins, size_t E) {
  std::vector<CopyJob> jobs;
  for (const InputVec& iv : ins) jobs.push_back({iv.slot, iv.src, E});
  par_copy(jobs);
  for (const InputVec& iv : ins) HC(hipMemcpyAsync(iv.dst, iv.slot, E, hipMemcpyHostToDevice, ctx->st));
}

// One vector in pieces: the host copy of piece p + 1 into the pinned slot runs while piece p is
// DMA'd, so a vector's DMA ends one piece after its host copy instead of a whole vector after.
// Vector 0 (F_0, whose transform starts round 1) in 2 MiB pieces, so that its first DMA starts
// ~0.03 ms into the call and its last ends ~0.04 ms after its copy; the others in 8 MiB pieces
// (fewer DMA submissions on the feeder thread)
void feed_vector(const InputVec& iv, bool first, size_t E, hipStream_t st) {
  const FeedKnobs& k = feed_knobs();
  const size_t span = first ? k.f0_span : (size_t)8 << 20;
  if (k.span_copy) {
    for (size_t o = 0; o < E; o += span) {
      const size_t len = std::min(span, E - o);
      par_copy({{iv.slot + o, iv.src + o, len}});
      HC(hipMemcpyAsync((uint8_t*)iv.dst + o, iv.slot + o, len, hipMemcpyHostToDevice, st));
    }
    return;
  }
  stream_copy(iv.slot, iv.src, E, span, [&](size_t o, size_t len) {
    HC(hipMemcpyAsync((uint8_t*)iv.dst + o, iv.slot + o, len, hipMemcpyHostToDevice, st));
  });
}

struct Feeder {  // the input-copy thread of vectors 1.. (joined on every exit path)
  std::thread t;
  std::mutex mu;
  std::condition_variable cv;
  size_t issued = 1;
  std::exception_ptr err;
  ~Feeder() {
    if (t.joinable()) t.join();
  }
};

// pipelined: vector v's host copy into its pinned slot overlaps vector v - 1's DMA; vector 0
// goes on the main stream, the others on the copy stream with an event that the main stream
// waits for right before the vector's first kernel, so F_0's transform starts while the rest
// are still in flight. (The Montgomery write-back has pinned slots of its own, written on st_wb:
// vector v's D2H is ordered after its conversion kernel, which waits on ev_in[v], i.e. after
// vector v's input DMA.) `feeder` and `ins` are the caller's: the thread started here reads both.
void feed_pipelined(kgs_ctx* ctx, const std::vector<InputVec>& ins, size_t E, ProveIn& in, Feeder& feeder) {
  const FeedKnobs& k = feed_knobs();
  ensure_input_events(ctx, ins.size(), in);
  if (k.f0_on_copy) {
    feed_vector(ins[0], true, E, ctx->st_copy);
    HC(hipEventRecord(ctx->ev_in[0], ctx->st_copy));
    in.ready[0] = ctx->ev_in[0];
  } else {
    feed_vector(ins[0], true, E, ctx->st);
  }
  // the link carries F_0 first: the copy stream's DMAs start after F_0's last one (ev_in[0] on the
  // main stream, which holds only F_0's DMAs here). With the multi-threaded staging copy, T_0's DMAs
  // otherwise shared the link with F_0's and F_0 arrived ~0.5 ms later (profiles/r06/copy_ab/);
  // KGS_FEED_ORDER=0 lets them overlap (A/B)
  const bool wait_f0 = k.ordered && ins.size() > 1 && !k.f0_on_copy;  // (same stream: ordered anyway)
  if (wait_f0) HC(hipEventRecord(ctx->ev_in[0], ctx->st));
  for (size_t v = 1; v < ins.size(); v++) in.ready[v] = ctx->ev_in[v];
  // vectors 1.. are copied into their pinned slots and DMA'd by a feeder thread while the prover
  // already enqueues (and the GPU runs) vector 0's work; prove_rounds waits for a vector's DMA to be
  // ENQUEUED (input_issued) before its kernels wait on the vector's event
  if (ins.size() < 2) return;
  feeder.t = std::thread([ctx, &ins, &feeder, E, wait_f0] {
    try {
      HC(hipSetDevice(ctx->device));
      if (wait_f0) HC(hipStreamWaitEvent(ctx->st_copy, ctx->ev_in[0], 0));
      for (size_t v = 1; v < ins.size(); v++) {
        feed_vector(ins[v], false, E, ctx->st_copy);
        HC(hipEventRecord(ctx->ev_in[v], ctx->st_copy));
        std::lock_guard<std::mutex> lk(feeder.mu);
        feeder.issued = v + 1;
        feeder.cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(feeder.mu);
      feeder.err = std::current_exception();
      feeder.issued = ins.size();
      feeder.cv.notify_all();
    }
  });
  in.input_issued = [&feeder](size_t v) {
    std::unique_lock<std::mutex> lk(feeder.mu);
    feeder.cv.wait(lk, [&] { return feeder.issued > v; });
    if (feeder.err) std::rethrow_exception(feeder.err);
  };
}

// The Montgomery write-back plan: in.mont_f_out / mont_t_out per vector (nullptr: not asked for) and
// the host copies left to do. D2H goes straight into the caller's buffer once it is pinned (the JS
// addon keeps its recycled output buffers registered), else into the vector's pinned slot of `pio`,
// from where a host thread copies it to the caller (the returned jobs) while rounds 2-5 run.
std::vector<CopyJob> plan_write_back(kgs_ctx* ctx, HostPins& pins, int npols, uint8_t* const* mont_f,
                                     uint8_t* const* mont_t, uint8_t* pio, size_t E, ProveIn& in) {
  std::vector<CopyJob> jobs;
  auto target = [&](uint8_t* const* mont, int i, size_t slot) -> uint8_t* {
    uint8_t* user = mont ? mont[i] : nullptr;
    if (!user) return nullptr;
    if (!ctx->group && pins.pin(user, E)) return user;
    jobs.push_back({user, pio + slot * E, E});
    return pio + slot * E;
  };
  for (int i = 0; i < npols; i++) {
    in.mont_f_out.push_back(target(mont_f, i, 2 * i));
    in.mont_t_out.push_back(target(mont_t, i, 2 * i + 1));
  }
  return jobs;
}

struct WriteBackCopy {  // the host thread of the write-back's pinned -> caller copies
  std::thread t;
  bool failed = false;
  ~WriteBackCopy() {
    if (t.joinable()) t.join();
  }
};

}  // namespace

extern "C" {

int kgs_host_register(void* ptr, uint64_t bytes) {
  API_BEGIN
  if (!ptr || !bytes) throw KgsError(KGS_E_ARG, "NULL argument");
  HC(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
  API_END
}

int kgs_host_unregister(void* ptr) {
  API_BEGIN
  if (!ptr) throw KgsError(KGS_E_ARG, "NULL argument");
  HC(hipHostUnregister(ptr));
  API_END
}

int kgs_test_stream_copy(uint8_t* dst, const uint8_t* src, uint64_t len, uint64_t span, int fail_at,
                         uint64_t* spans_out, int max, int* nspans) {
  API_BEGIN
  if (!dst || !src || !nspans || (max > 0 && !spans_out)) throw KgsError(KGS_E_ARG, "NULL argument");
  *nspans = 0;
  stream_copy(dst, src, (size_t)len, (size_t)span, [&](size_t o, size_t) {
    if (*nspans == fail_at) throw KgsError(KGS_E_HIP, "injected span failure");
    if (*nspans < max) spans_out[*nspans] = o;
    (*nspans)++;
  });
  API_END
}

int kgs_prove(kgs_ctx_t* ctx, int kind, int nbits, int npols, const uint8_t* const* evals_f,
              const uint8_t* const* evals_t, const uint8_t* sel_f, const uint8_t* sel_t, uint8_t* const* mont_f,
              uint8_t* const* mont_t, uint8_t* commitments_out, uint8_t* evaluations_out) {
  API_BEGIN
  if (!ctx || !evals_f || !evals_t || !commitments_out || !evaluations_out) throw KgsError(KGS_E_ARG, "NULL argument");
  CTX_LOCK(ctx);
  if ((sel_f == nullptr) != (sel_t == nullptr)) throw KgsError(KGS_E_ARG, "selectors must be both given or both NULL");
  if (npols < 1 || npols > KGS_MAX_POLS || nbits < 1 || nbits > 28) throw KgsError(KGS_E_ARG, "bad shape");
  HC(hipSetDevice(ctx->device));
  // The order of these declarations is the error-path contract (destruction runs it backwards):
  //  1. DrainOnError first, so destroyed last: an error return drains the context's streams, so no DMA
  //     of this call still reads or writes caller memory (pinned inputs DMA'd in place, pinned
  //     write-back targets) once the caller has it back;
  //  2. then the proofs-in-progress scope (the staging copy's store choice);
  //  3. then HostPins, before the feeder and the write-back thread: both are joined before any buffer
  //     is unpinned or any stream drained, so nothing can enqueue another DMA on them. What the two
  //     threads read (ins, out_jobs) is declared before them for the same reason.
  // None of these objects lives inside a step function: the steps take them by reference.
  DrainOnError drain(ctx);
  ProofInProgress proof_active;
  std::vector<InputVec> ins;
  std::vector<CopyJob> out_jobs;
  HostPins pins(ctx);
  Feeder feeder;
  WriteBackCopy out_copy;
  const size_t E = (size_t)32 << nbits;
  ProveIn in;
  in.kind = kind;
  in.nbits = nbits;
  in.npols = npols;
  // pageable caller buffers -> write-combined pinned staging (parallel host copies) -> DMAs; the
  // Montgomery write-back goes device -> its own pinned slots (st_wb) -> caller (a host thread)
  const int nvec = 2 * npols + (sel_f ? 2 : 0);
  uint8_t* pin_in = ctx->io_in((size_t)nvec * E);
  uint8_t* pio = mont_f || mont_t ? ctx->io((size_t)2 * npols * E) : nullptr;  // write-back slots
  ctx->sync();  // the staging area may still feed a previous call's copies
  auto input = [&](const uint8_t* src, const std::string& name) {
    ins.push_back({src, pin_in + ins.size() * E, ctx->buf(name, E)});
    return ins.back().dst;
  };
  for (int i = 0; i < npols; i++) {
    in.f_std.push_back(input(evals_f[i], "in_f" + std::to_string(i)));
    in.t_std.push_back(input(evals_t[i], "in_t" + std::to_string(i)));
  }
  if (sel_f) {
    in.sel_f = input(sel_f, "in_sf");
    in.sel_t = input(sel_t, "in_st");
  }

  using hclk = std::chrono::steady_clock;
  const auto h0 = hclk::now();
  {
    Range rin("kgs.host.input_copy");
    if (ctx->group) feed_group(ctx, ins, E);
    else if (!feed_in_place(ctx, pins, ins, E, in)) feed_pipelined(ctx, ins, E, in, feeder);
  }
  const auto h1 = hclk::now();
  out_jobs = plan_write_back(ctx, pins, npols, mont_f, mont_t, pio, E, in);
  // the Montgomery forms are in the pinned slots once round 1 is synchronised: copy them to the
  // caller on a host thread while rounds 2-5 run
  if (!out_jobs.empty())
    in.after_round1 = [&] {
      out_copy.t = std::thread([&, dev = ctx->device] {
        // the device -> pinned write-back (st_wb) must be complete before the pinned -> caller copy
        if (hipSetDevice(dev) != hipSuccess || (ctx->st_wb && hipStreamSynchronize(ctx->st_wb) != hipSuccess)) {
          out_copy.failed = true;
          return;
        }
        par_copy(out_jobs);
      });
    };
  const auto h2 = hclk::now();
  prove_impl(*ctx, in, commitments_out, evaluations_out);  // ends synchronised
  const auto h3 = hclk::now();
  {
    Range rout("kgs.host.writeback_wait");
    if (out_copy.t.joinable()) out_copy.t.join();
    if (out_copy.failed) throw KgsError(KGS_E_HIP, "Montgomery write-back: copy stream failed");
  }
  const auto h4 = hclk::now();
  // host-boundary phases: [6] input copy into pinned staging, [7] prover, [8] write-back wait
  ctx->timing.resize(9, 0.0);
  ctx->timing[6] = std::chrono::duration<double, std::milli>(h1 - h0).count();
  ctx->timing[7] = std::chrono::duration<double, std::milli>(h3 - h2).count();
  ctx->timing[8] = std::chrono::duration<double, std::milli>(h4 - h3).count();
  API_END
}

}  // extern "C"
