// The commitment MSM's host side: the resident SRS and its window tables, the MSM work buffers of
// both lanes, the launch of a commitment (whole, sharded, split over the lanes) and its host finish,
// and the C-ABI entry points that are only about the MSM (include/kgs.h). Device side: msm.hip.
#include <mutex>

#include "context.hpp"

namespace kgsi {

// ------------------------------------------------------------------ SRS
// Window c of the MSM tables of `npts` resident points: lg - 4, between 7 and 17. The bucket entries
// of an N-point MSM are N * ceil(255 / c) XYZZ mixed adds, its bucket tail (row / column sums) ~2^c
// full adds. Windows up to c = 20 are built and parity-tested (KGS_MSM_C, the sort's partitions grow
// to 2048), but c = 20 at n = 2^20 measured slower: 13 windows instead of 15 cut the accumulation
// 1.25 -> 1.10 ms, while the sort went 0.15 -> 0.30 ms and the tail 0.21 -> 0.53 ms, 93.3 -> 85.3
// proofs/s in flight (DESIGN.md §13 "Wider windows", profiles/r06/wide/)
int choose_window(uint64_t n, int c_min, int c_max, const char* env_name, int env_max) {
  int lg = 0;
  while ((1ull << lg) < n) lg++;
  int cc = lg - 4;
  if (cc < c_min) cc = c_min;
  if (cc > c_max) cc = c_max;
  if (const char* e = getenv(env_name)) {  // A/B override of the window
    const int v = atoi(e);
    if (v >= c_min && v <= env_max) cc = v;
  }
  return cc;
}

// at least 7: staging LDS of the partition pass, 256 * 2 * ceil(255/c) * 7 B <= 133 KB
int choose_c(uint64_t npts) { return choose_window(npts, 7, 17, "KGS_MSM_C", KGS_C_MAX); }

void msm_work_from_pool(kgs_ctx& c, MsmWork& w, const std::string& prefix, const std::string& suffix,
                        const MsmSizes& z) {
  auto get = [&](const char* name, uint64_t bytes) { return c.buf(prefix + name + suffix, (size_t)bytes); };
  w.digit = (int32_t*)get("digit", z.digit);
  w.sorted = get("sorted", z.sorted);
  w.lo = (uint8_t*)get("lo", z.lo);
  w.blockhist = get("blockhist", z.blockhist);
  w.counts = get("counts", z.counts);
  w.offsets = get("offsets", z.offsets);
  w.cursor = get("cursor", z.cursor);
  w.segowner = get("segowner", z.segowner);
  w.locnt = get("locnt", z.locnt);
  w.chunklist = get("chunklist", z.chunklist);
  w.chunkcnt = get("chunkcnt", 64);  // CB_LEVELS words
  w.raw29 = get("raw29", z.raw29);
  w.part = get("part", z.part);
}

// MSM work buffers of both lanes, for MSMs of up to npts points with window c
void ensure_msm_work(kgs_ctx& c) {
  const uint64_t npts = c.tb.npts;
  if (c.work_npts >= npts && c.work_npts) return;
  c.work_npts = 0;  // invalid until every buffer below exists
  const int cc = c.tb.c;
  const MsmSizes z = msm_work_sizes(npts, cc, cc, 1ull << (cc - 1), 1);
  msm_work_from_pool(c, c.mw, "msm_", "", z);
  msm_work_from_pool(c, c.mw2, "msm_", "_2", z);
  c.work_npts = npts;
}

// Build (or share) the window tables of `npts` LEM points. `file` identifies the source; an empty
// `file` (in-memory points) is never shared. (srank, sworld): the points are a rank's slice of the
// SRS (points srank + sworld * j of the file; sworld == 1: the prefix). The context's SRS is replaced
// only once the new tables and the work buffers exist: a failed load leaves the context without an
// SRS ("no SRS loaded"), never with a half-built one. The device registry lock is held only to look
// up and to publish: the build (H2D copy + window expansion, seconds at 2^25 points) runs outside it,
// so other contexts of the device are not blocked meanwhile; a concurrent build of the same tables
// that published first wins and this one is dropped.
static std::shared_ptr<SrsTables> srs_lookup(int device, const std::string& file, int nbits_max, int srank, int sworld) {
  if (file.empty()) return nullptr;
  for (auto& w : g_srs_reg) {
    auto t = w.lock();
    if (t && t->device == device && t->file == file && t->nbits_max >= nbits_max && t->slice_rank == srank &&
        t->slice_world == sworld)
      return t;
  }
  return nullptr;
}

void load_points(kgs_ctx& c, const uint8_t* lem, uint64_t npts, int power, int nbits_max, const std::string& file,
                 int srank, int sworld) {
  if (npts < 2) throw KgsError(KGS_E_ARG, "SRS needs at least 2 points");
  c.sync();
  c.use_srs(nullptr);
  c.work_npts = 0;
  std::shared_ptr<SrsTables> s;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    s = srs_lookup(c.device, file, nbits_max, srank, sworld);
  }
  if (!s) {
    int cc = choose_c(npts);
    int W = (255 + cc - 1) / cc;
    // sorted entries pack j * npts + i into 31 bits (bit 31 = sign): widen the window until it fits
    while ((uint64_t)W * npts > (1ull << 31) && cc < KGS_C_MAX) {
      cc++;
      W = (255 + cc - 1) / cc;
    }
    if ((uint64_t)W * npts > (1ull << 31)) throw KgsError(KGS_E_SRS, "SRS too large for the MSM entry index");
    auto t = std::make_shared<SrsTables>();
    t->device = c.device;
    t->file = file;
    t->power = power;
    t->nbits_max = nbits_max;
    t->slice_rank = srank;
    t->slice_world = sworld;
    t->tb.npts = npts;
    t->tb.c = cc;
    t->tb.W = W;
    HC(dev_malloc((void**)&t->tb.table, (size_t)W * npts * 64));
    HC(hipMemcpyAsync(t->tb.table, lem, npts * 64, hipMemcpyHostToDevice, c.st));
    // build temporaries are released right after the build (they would otherwise stay in the pool)
    struct Tmp {
      void* p = nullptr;
      ~Tmp() {
        if (p) hipFree(p);
      }
    } tmp, scr, zflag;
    HC(dev_malloc(&tmp.p, npts * 128));
    HC(dev_malloc(&scr.p, npts * 32));
    HC(dev_malloc(&zflag.p, 16));
    // rho = 2^-256 mod r as a standard integer: the Montgomery word 1 stands for it
    host::Fr rinv = host::Fr::zero();
    rinv.v[0] = 1;
    uint64_t rho64[4];
    rinv.to_std(rho64);
    uint32_t rho[8];
    memcpy(rho, rho64, 32);
    msm_build_table(c.st, t->tb.table, npts, cc, W, (uint32_t*)tmp.p, (uint32_t*)scr.p, rho, (uint32_t*)zflag.p);
    check_launch();
    uint32_t zero_points = 1;
    HC(hipMemcpyAsync(&zero_points, zflag.p, 4, hipMemcpyDeviceToHost, c.st));
    HC(hipStreamSynchronize(c.st));
    t->tb.zero_points = zero_points != 0;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (auto other = srs_lookup(c.device, file, nbits_max, srank, sworld)) {
      s = other;  // built concurrently by another context and published first: ours is released
    } else {
      g_srs_reg.erase(std::remove_if(g_srs_reg.begin(), g_srs_reg.end(), [](auto& w) { return w.expired(); }),
                      g_srs_reg.end());
      if (!file.empty()) g_srs_reg.push_back(t);
      s = t;
    }
  }
  ensure_domain(c, s->nbits_max + 1);
  MsmTables keep = c.tb;
  c.tb = s->tb;  // ensure_msm_work sizes from the new tables
  try {
    ensure_msm_work(c);
  } catch (...) {
    c.tb = keep;
    c.use_srs(nullptr);
    throw;
  }
  c.sync();
  c.use_srs(s);
}

// ------------------------------------------------------------------ MSM (commit)
// Polynomial.multiExponentiation (polynomial.js:1106-1115): device Pippenger -> c bit-sum points
// T_k (XYZZ) -> host sum_k 2^k T_k -> affine LEM. Sharded (world > 1): this rank's point range
// only; the partials of all ranks are all-gathered once per batch of commits (one prover round).

// The host-boundary copy streams (st_copy: input DMAs, st_wb: the Montgomery write-back) carry only
// copies and event waits. HIP maps streams onto a few hardware queues per priority level
// (GPU_MAX_HW_QUEUES, 4 by default), so with several contexts in flight a copy stream would share a
// hardware queue with another proof's compute stream, whose kernels then queue behind the copy
// stream's waits. Created at the lowest priority they get their own pool of hardware queues
// (KGS_COPY_STREAM_PRIO=normal keeps them in the compute streams' pool, for A/B).
hipStream_t copy_stream() {
  static const bool low = [] {
    const char* e = getenv("KGS_COPY_STREAM_PRIO");
    return !(e && !strcmp(e, "normal"));
  }();
  hipStream_t s = nullptr;
  if (low) {
    int least = 0, greatest = 0;
    HC(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HC(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least));
  } else {
    HC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  }
  return s;
}

void shard_range(uint64_t n, int rank, int world, uint64_t& lo, uint64_t& hi) {
  lo = (uint64_t)((unsigned __int128)n * (unsigned)rank / (unsigned)world);
  hi = (uint64_t)((unsigned __int128)n * (unsigned)(rank + 1) / (unsigned)world);
}

// `to` waits for everything issued so far on `from` (lane hand-over inside a round)
void lane_join(kgs_ctx& c, hipStream_t from, hipStream_t to) {
  if (from == to) return;
  if (!c.ev_join) HC(hipEventCreateWithFlags(&c.ev_join, hipEventDisableTiming));
  HC(hipEventRecord(c.ev_join, from));
  HC(hipStreamWaitEvent(to, c.ev_join, 0));
}

// the second MSM lane starts after everything issued so far on the main stream (the round's inputs)
void fork_lanes(kgs_ctx& c) {
  if (c.msm_lanes < 2) return;
  if (!c.st2) {
    HC(hipStreamCreateWithFlags(&c.st2, hipStreamNonBlocking));
    HC(hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming));
  }
  HC(hipEventRecord(c.ev_fork, c.st));
  HC(hipStreamWaitEvent(c.st2, c.ev_fork, 0));
}

Commit commit_launch_slice(kgs_ctx& c, const uint32_t* scalars, uint64_t count, uint64_t pbase, uint64_t pstride,
                           uint64_t N, int slot, int lane) {
  Commit cm;
  cm.N = N;
  const int cc = c.tb.c;
  const int slots = c.msm_slots > 64 ? c.msm_slots : 64;
  if (slot >= slots) throw KgsError(KGS_E_ARG, "too many commitments in flight");
  uint64_t cap = c.tb.npts;  // global points the resident SRS covers
  if (c.srs_slice_world > 1) {
    // a rank's SRS slice holds the points slice_rank + slice_world * j only: it serves exactly the
    // commitments over this rank's CYCLIC slice, whose scalar j multiplies that point
    if (count && (pstride != (uint64_t)c.srs_slice_world || pbase != (uint64_t)c.srs_slice_rank))
      throw KgsError(KGS_E_ARG, "the loaded SRS slice (rank " + std::to_string(c.srs_slice_rank) + " of " +
                                    std::to_string(c.srs_slice_world) + ") does not hold this commitment's points");
    pbase = 0;
    pstride = 1;
    cap = (uint64_t)c.srs_slice_rank + (uint64_t)c.srs_slice_world * c.tb.npts;
  }
  if (N > cap || (count && pbase + pstride * (count - 1) >= c.tb.npts))
    throw KgsError(KGS_E_SRS, "MSM larger than the resident SRS");
  uint32_t* dT = c.buf("msm_T", (size_t)slots * cc * 128) + (size_t)slot * cc * 32;
  cm.h_T = c.pin((size_t)cc * 128);
  if (count == 0) {
    memset(cm.h_T, 0, (size_t)cc * 128);  // ZZ == 0: infinity
    return cm;
  }
  if (c.msm_lanes < 2) lane = 0;
  hipStream_t st = lane ? c.st2 : c.st;  // lane 1 was forked (fork_lanes) after the round's inputs
  if (!msm_run(st, c.tb, lane ? c.mw2 : c.mw, scalars, count, dT, nullptr, pbase, pstride, c.msm_lanes >= 2))
    throw KgsError(KGS_E_ARG, "unsupported MSM window");
  check_launch();
  HC(hipMemcpyAsync(cm.h_T, dT, (size_t)cc * 128, hipMemcpyDeviceToHost, st));
  return cm;
}

// MSM point-range sharding (kgs_ctx_set_shard): this rank's contiguous range of the N points
Commit commit_launch(kgs_ctx& c, const uint32_t* scalars, uint64_t N, int slot, int lane) {
  uint64_t lo = 0, hi = N;
  if (c.shard_world > 1) shard_range(N, c.shard_rank, c.shard_world, lo, hi);
  Commit cm = commit_launch_slice(c, scalars + (size_t)8 * lo, hi - lo, lo, 1, N, slot, lane);
  return cm;
}

bool split_commits(const kgs_ctx& c) { return c.msm_lanes >= 2 && c.shard_world == 1; }

Commit commit_launch_split(kgs_ctx& c, const uint32_t* scalars, uint64_t N, uint64_t cut, int slot) {
  if (!split_commits(c) || cut == 0 || cut >= N) return commit_launch(c, scalars, N, slot, 0);
  Commit a = commit_launch_slice(c, scalars, cut, 0, 1, N, slot, 0);
  Commit b = commit_launch_slice(c, scalars + (size_t)8 * cut, N - cut, cut, 1, N, slot + 1, 1);
  a.h_T2 = b.h_T;
  return a;
}

// sum_k 2^k sum_r T_k^(r) -> affine LEM
void combine_partials(const uint8_t* T_all, size_t part_stride, int nparts, int cc, uint8_t out[64]) {
  host::G1 acc = host::G1::inf();
  for (int k = cc - 1; k >= 0; k--) {
    acc = acc.dbl();
    for (int r = 0; r < nparts; r++) acc = acc.add(host::G1::from_bytes128(T_all + r * part_stride + 128 * k));
  }
  acc.to_affine_lem(out);
}

// after sync: finish a batch of commits; with world > 1 the partials of all ranks are exchanged in
// ONE all-gather per batch (one prover round) and summed on the host
void commits_finish_with(kgs_ctx& c, const std::vector<Commit>& cms, std::vector<uint8_t*> outs, int world,
                         const HostAllgather& ag) {
  const int cc = c.tb.c;
  const size_t tb = (size_t)cc * 128;
  bool any = false;
  for (auto& cm : cms) any |= cm.N > 0;
  if (world == 1 || !any) {
    std::vector<uint8_t> two;
    for (size_t i = 0; i < cms.size(); i++) {
      if (cms[i].N && cms[i].h_T2) {  // split over the two lanes: both partials
        two.resize(2 * tb);
        memcpy(two.data(), cms[i].h_T, tb);
        memcpy(two.data() + tb, cms[i].h_T2, tb);
        combine_partials(two.data(), tb, 2, cc, outs[i]);
      } else if (cms[i].N) {
        combine_partials(cms[i].h_T, tb, 1, cc, outs[i]);
      } else {
        host::G1::inf().to_affine_lem(outs[i]);
      }
    }
    return;
  }
  const size_t bytes = tb * cms.size();
  std::vector<uint8_t> send(bytes), recv(bytes * world);
  for (size_t i = 0; i < cms.size(); i++) memcpy(send.data() + i * tb, cms[i].h_T, tb);
  ag(send.data(), recv.data(), bytes);
  for (size_t i = 0; i < cms.size(); i++) {
    if (cms[i].N) combine_partials(recv.data() + i * tb, bytes, world, cc, outs[i]);
    else host::G1::inf().to_affine_lem(outs[i]);
  }
}

void commits_finish(kgs_ctx& c, const std::vector<Commit>& cms, std::vector<uint8_t*> outs) {
  commits_finish_with(c, cms, outs, c.shard_world, [&](const void* send, void* recv, size_t bytes) {
    if (!c.shard_fn) throw KgsError(KGS_E_COMM, "sharding enabled without an all-gather callback");
    if (c.shard_fn(c.shard_user, (const uint8_t*)send, (uint8_t*)recv, bytes) != 0)
      throw KgsError(KGS_E_COMM, "shard all-gather failed");
  });
}

void commit_finish(kgs_ctx& c, const Commit& cm, uint8_t out[64]) { commits_finish(c, {cm}, {out}); }

}  // namespace kgsi

extern "C" {

int kgs_msm(kgs_ctx_t* ctx, const uint8_t* scalars_mont, uint64_t n, uint8_t out_lem[64]) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  HC(hipSetDevice(ctx->device));
  if (n > ctx->tb.npts) throw KgsError(KGS_E_SRS, "MSM larger than the resident SRS");
  ctx->reset_staging();
  uint32_t* a = ctx->buf("prim_a", 32 * (n ? n : 1));
  HC(hipMemcpyAsync(a, scalars_mont, 32 * n, hipMemcpyHostToDevice, ctx->st));
  Commit cm = commit_launch(*ctx, a, n, 0);
  ctx->sync();
  commit_finish(*ctx, cm, out_lem);
  ctx->reset_staging();
  API_END
}

int kgs_shard_range(uint64_t n, int rank, int world, uint64_t* lo, uint64_t* hi) {
  API_BEGIN
  if (world < 1 || rank < 0 || rank >= world || !lo || !hi) throw KgsError(KGS_E_ARG, "bad shard rank/world");
  shard_range(n, rank, world, *lo, *hi);
  API_END
}

int kgs_msm_combine(const uint8_t* T_all, int nparts, int c, uint8_t out_lem[64]) {
  API_BEGIN
  if (!T_all || !out_lem || nparts < 1 || c < 1 || c > 32) throw KgsError(KGS_E_ARG, "bad msm_combine arguments");
  combine_partials(T_all, (size_t)c * 128, nparts, c, out_lem);
  API_END
}

int kgs_bench_msm(kgs_ctx_t* ctx, const void* d_scalars_mont, uint64_t n, int reps, double* ms) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  HC(hipSetDevice(ctx->device));
  if (n > ctx->tb.npts || ctx->srs_slice_world > 1) throw KgsError(KGS_E_SRS, "MSM larger than the resident SRS (or an SRS slice)");
  uint32_t* dT = ctx->buf("msm_T", (size_t)64 * ctx->tb.c * 128);
  if (!msm_run(ctx->st, ctx->tb, ctx->mw, (const uint32_t*)d_scalars_mont, n, dT))  // warm
    throw KgsError(KGS_E_ARG, "unsupported MSM window");
  *ms = EventTimer().ms(ctx->st, [&] {  // one interval around all the repetitions
    for (int r = 0; r < reps; r++) msm_run(ctx->st, ctx->tb, ctx->mw, (const uint32_t*)d_scalars_mont, n, dT);
  });
  API_END
}

int kgs_bench_msm_phases(kgs_ctx_t* ctx, const void* d_scalars_mont, uint64_t n, int reps, double* phase_ms,
                         uint64_t* entries) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  HC(hipSetDevice(ctx->device));
  if (n > ctx->tb.npts || ctx->srs_slice_world > 1) throw KgsError(KGS_E_SRS, "MSM larger than the resident SRS (or an SRS slice)");
  uint32_t* dT = ctx->buf("msm_T", (size_t)64 * ctx->tb.c * 128);
  hipEvent_t ev[5];
  for (auto& e : ev) HC(hipEventCreate(&e));
  for (int i = 0; i < 4; i++) phase_ms[i] = 0;
  for (int r = 0; r < reps; r++) {
    if (!msm_run(ctx->st, ctx->tb, ctx->mw, (const uint32_t*)d_scalars_mont, n, dT, ev))
      throw KgsError(KGS_E_ARG, "unsupported MSM window");
    HC(hipEventSynchronize(ev[4]));
    for (int i = 0; i < 4; i++) {
      float f = 0;
      HC(hipEventElapsedTime(&f, ev[i], ev[i + 1]));
      phase_ms[i] += f;
    }
  }
  const uint32_t B = 1u << (ctx->tb.c - 1);
  uint32_t tot = 0;
  HC(hipMemcpy(&tot, ctx->mw.offsets + (B + 1), 4, hipMemcpyDeviceToHost));
  if (entries) *entries = tot;
  for (auto& e : ev) hipEventDestroy(e);
  API_END
}

}  // extern "C"
