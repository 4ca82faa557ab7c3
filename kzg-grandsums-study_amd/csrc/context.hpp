// Internal interface of the prover library (not part of the C-ABI): the context, the shared
// device tables and the host-side building blocks of a proof. Shared by prover.cpp (building blocks,
// single prover, context entry points), host_boundary.cpp (kgs_prove over host buffers), primitives.cpp
// (the C-ABI building blocks), srs_api.cpp (SRS / ptau entry points), msm_commit.cpp (SRS tables and the
// commitment MSM), prover_rounds.cpp (the protocol rounds of the single and the multi-argument prover,
// DESIGN.md §16), prover_multi.cpp (the multi prover's entry points) and the distributed prover over a
// rank group: prover_dist.cpp (its five rounds), dist_layout.hpp (the layouts, exchange steps
// and exchange accounting), dist_math.hpp (its cross-rank host arithmetic) and dist_group.cpp (the
// transports behind kgs_group, with rank_rendezvous.hpp, and the kgs_group_* entry points). The
// Fiat-Shamir schedule of every prover and verifier is transcript.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <array>
#include <string>
#include <vector>

#include "../../include/kgs.h"
#include "host_copy.hpp"
#include "host_error.hpp"
#include "host_field.hpp"
#include "kernels.hpp"
#ifndef KGS_NO_ROCTX
#include <rocprofiler-sdk-roctx/roctx.h>
#endif

namespace kgsi {
using namespace kgs;
using host::Fq;
using host::Fr;

#define HC(x)                                                                                    \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess)                                                                        \
      throw KgsError(KGS_E_HIP, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x); \
  } while (0)

inline void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw KgsError(KGS_E_HIP, std::string("HIP launch error: ") + hipGetErrorString(e));
}

using host::fr_w;

// roctx ranges (rocprofv3 --marker-trace): one per prover round and per host-boundary phase, so a
// trace shows where a proof's host wall time goes next to its kernels. -DKGS_NO_ROCTX removes them.
struct Range {
  bool open = false;
  explicit Range(const char* name = nullptr) {
    if (name) push(name);
  }
  void push(const char* name) {
    pop();
#ifndef KGS_NO_ROCTX
    roctxRangePushA(name);
#endif
    open = true;
  }
  void pop() {
#ifndef KGS_NO_ROCTX
    if (open) roctxRangePop();
#endif
    open = false;
  }
  ~Range() { pop(); }
};
inline const char* const ROUND_NAMES[5] = {"kgs.round1.commit_witness", "kgs.round2.grand_poly", "kgs.round3.quotient",
                                    "kgs.round4.evaluations", "kgs.round5.openings"};

// Every device allocation goes through here (prover.cpp). KGS_DEBUG_ALLOC_LIMIT=<bytes> (fault
// injection for the tests) makes any single request above that size fail as out-of-memory.
hipError_t dev_malloc(void** p, size_t bytes);

// multisets per proof (the reference has no limit; this only bounds host-side bookkeeping)
constexpr int KGS_MAX_POLS = 1024;

#ifndef KGS_C_MAX
#define KGS_C_MAX 20
#endif

struct DBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// Read-only device tables shared by every context on a device (one copy per device, not per
// in-flight context): the SRS window tables of a ptau (keyed by file identity and the domain they
// were loaded for) and the NTT / coset twiddle tables (the largest domain built so far serves every
// smaller one: stage tables tw[h + t] = w_2h^t do not depend on the maximum domain). Published only
// after their build has completed (stream synchronised), released when the last context drops them.
// One row of device points derived from a resident SRS for a domain of n = 2^nbits points and cached on its
// SrsTables entry (srs_row_cached below): the Lagrange bases, or the SRS side of the openings' Toeplitz product
struct SrsRow {
  int device = 0;
  uint32_t* p = nullptr;
  uint64_t n = 0;
  static std::shared_ptr<SrsRow> make(int device, uint64_t n, size_t bytes) {
    auto row = std::make_shared<SrsRow>();
    row->device = device;
    row->n = n;
    HC(dev_malloc((void**)&row->p, bytes));
    return row;
  }
  ~SrsRow() {
    if (p) {
      hipSetDevice(device);
      hipFree(p);
    }
  }
};

struct SrsTables {
  int device = 0;
  std::string file;  // file identity (path + size + mtime) or "mem#<id>"
  int power = -1, nbits_max = -1;
  // a rank's slice of the SRS (kgs_srs_load_ptau_slice): row 0 holds the points slice_rank +
  // slice_world * j only (slice_world == 1: the whole prefix)
  int slice_rank = 0, slice_world = 1;
  MsmTables tb;
  // nbits -> the Lagrange-basis SRS [L_i(tau)]_1, i < n (g1_ntt.cpp, kgs_srs_lagrange): n points in the form
  // msm_points_run reads
  std::map<int, std::shared_ptr<SrsRow>> lagrange;
  // (nbits, lbits) -> the SRS side of the openings (kzg_open.cpp); lbits == 0 is
  // kgs_kzg_open_all's row: the forward G1 transform of size 2n of (s_{n-2}, .., s_0, identity ..) over table
  // row 0, scaled by 1 / 2n. lbits >= 1 are kgs_kzg_open_cosets' rows: the l = 2^lbits transforms of size
  // 2m = 2n / l of the stride-l subsequences of that vector, scaled by 1 / 2m; block b of 2m points belongs to
  // the residue bitrev_l(b). 2n affine points in the 2^256 form either way, still carrying the row's rho
  std::map<std::pair<int, int>, std::shared_ptr<SrsRow>> fk;
  ~SrsTables() {
    if (tb.table) {
      hipSetDevice(device);
      hipFree(tb.table);
    }
  }
};

struct DomainTables {
  int device = 0, logM = -1;
  uint32_t* mem = nullptr;
  uint32_t *tw_fwd = nullptr, *tw_inv = nullptr, *coset_pow = nullptr, *coset_ipow = nullptr, *invm = nullptr;
  // every table of `mem` again as 9 x 29-bit limbs of x * 2^261 (10 words per element, fr29.hpp): the
  // LDS NTT passes' twiddle and scaling products (ntt_register_tw29 maps a pointer into `mem` to its
  // record here)
  uint32_t* mem29 = nullptr;
  ~DomainTables() {
    hipSetDevice(device);
    if (mem29) {
      ntt_unregister_tw29(mem);
      hipFree(mem29);
    }
    if (mem) hipFree(mem);
  }
};

extern std::mutex g_reg_mu;  // lock order: kgs_ctx::mu, then g_reg_mu
extern std::vector<std::weak_ptr<SrsTables>> g_srs_reg;
extern std::vector<std::weak_ptr<DomainTables>> g_dom_reg;

}  // namespace kgsi

using namespace kgsi;

// Rank group of the distributed prover (transports in dist_group.cpp). wait() drains a stream that
// may hold the group's exchanges: a transport whose peers can hang (RCCL) polls it against a
// deadline instead of blocking forever.
struct kgs_group {
  int world = 1;
  virtual ~kgs_group() {}
  // blocking host all-gather: recv = world x bytes, rank-major
  virtual void allgather(int rank, const void* send, void* recv, size_t bytes) = 0;
  // device all-to-all ordered on st: chunk j of send -> rank j; chunk j of recv <- rank j
  virtual void alltoall(int rank, struct kgs_ctx& c, hipStream_t st, const void* send, void* recv, size_t chunk) = 0;
  // bytes that leave a rank in one alltoall of `chunk`-byte chunks on this transport: the chunks for
  // the W - 1 other ranks, unless the transport moves more (HostGroup without an all-to-all callback
  // all-gathers the whole send buffer)
  virtual uint64_t alltoall_wire_bytes(size_t chunk) const { return (uint64_t)chunk * (world - 1); }
  // a rank failed: unblock the others (they fail too instead of waiting forever)
  virtual void abort() {}
  // a context on `device` becomes `rank` (kgs_ctx_set_group): transports that move device data
  // between the ranks' devices directly prepare that here
  virtual void attach(int rank, int device) { (void)rank; (void)device; }
  virtual void wait(hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) throw KgsError(KGS_E_HIP, std::string("HIP error: ") + hipGetErrorString(e) + " (stream sync)");
  }
};
// seconds a rank waits for its peers in a group exchange (KGS_GROUP_TIMEOUT_S, default 120)
double group_timeout_s();

// Exchanges of the last distributed proof on a context (kgs_last_exchange): every all-to-all is
// bracketed by two events on the stream it is ordered on (its span includes waiting for the peers),
// every host all-gather by the wall clock; bytes are those leaving this rank.
struct ExchangeStats {
  int a2a_n = 0, ag_n = 0;
  double a2a_ms = 0, ag_ms = 0;
  uint64_t a2a_bytes = 0, ag_bytes = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;  // grow-only pool
  void reset() {
    a2a_n = ag_n = 0;
    a2a_ms = ag_ms = 0;
    a2a_bytes = ag_bytes = 0;
  }
  ~ExchangeStats() {
    for (auto& e : ev) {
      hipEventDestroy(e.first);
      hipEventDestroy(e.second);
    }
  }
};

struct kgs_ctx {
  // every C-ABI entry point that touches the context holds mu: a busy context blocks its caller,
  // it is never entered twice (the JS backend runs prove() calls on libuv worker threads)
  std::mutex mu;
  int device = 0;
  hipStream_t st = nullptr;
  std::map<std::string, DBuf> pool;
  // pinned staging of the host-buffer boundary: h_in receives kgs_prove's inputs (the CPU only writes
  // it, the DMA engine reads it), h_io the Montgomery write-back (the CPU reads it). KGS_STAGE_WC=1
  // makes h_in write-combined: SDMA reads that at ~55 GB/s against ~30 GB/s from coherent pinned
  // memory alone (profiles/r05/d2h_engine.txt), but the host copy into it is slower and a proof
  // measured the same either way (profiles/r05/stage_wc_ab.txt), so it is off by default
  uint8_t* h_in = nullptr;
  size_t h_in_bytes = 0;
  uint8_t* h_io = nullptr;
  size_t h_io_bytes = 0;
  // pinned staging
  uint8_t* h_pin = nullptr;
  size_t h_pin_bytes = 0;
  size_t h_pin_off = 0;
  uint32_t* d_scal = nullptr;  // device scalar area
  size_t d_scal_off = 0;
  static constexpr size_t SCAL_BYTES = 1 << 16;
  // SRS (shared, read-only) and this context's views of it
  std::shared_ptr<SrsTables> srs;
  int srs_power = -1;
  int nbits_max = -1;
  MsmTables tb;
  MsmWork mw;
  uint64_t work_npts = 0;  // MSM work buffers (both lanes) are sized for this many points
  int msm_slots = 0;       // commitments in flight per proof (msm_T slots)
  // second MSM lane: independent commitments of one round (R1's F_i/T_i, R5's two W) alternate
  // between st and st2 (own work buffers), so one MSM's latency-bound tail overlaps the other's
  // bucket accumulation
  hipStream_t st2 = nullptr;
  hipStream_t st_copy = nullptr;  // kgs_prove's input DMAs (vectors 1..)
  // the Montgomery write-back (prover.js:147-148): its own stream, so that it never sits between
  // the input DMAs on st_copy; each vector's D2H waits only for that vector's conversion
  hipStream_t st_wb = nullptr;
  std::vector<hipEvent_t> ev_wb;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  std::vector<hipEvent_t> ev_in;  // kgs_prove: one per input vector DMA'd on the copy stream
  MsmWork mw2;
  int msm_lanes = 2;  // kgs_ctx_set_msm_lanes
  bool ref_quirks = true;  // kgs_ctx_set_reference_quirks (ref_quirks.cpp); default on
  // domain tables (M = 2^logM; shared) and this context's views of them
  std::shared_ptr<DomainTables> dom;
  int logM = -1;
  uint32_t *tw_fwd = nullptr, *tw_inv = nullptr, *coset_pow = nullptr, *coset_ipow = nullptr, *invm = nullptr;
  std::map<std::pair<int, int>, uint32_t*> nxm1;  // (nbits, lcs) -> 1/(n(x-1)) on the coset (bitrev)
  std::vector<double> timing;
  // MSM point-range sharding (kgs_ctx_set_shard): world > 1 splits every commitment MSM
  int shard_rank = 0, shard_world = 1;
  kgs_allgather_fn shard_fn = nullptr;
  void* shard_user = nullptr;
  // distributed prover (kgs_ctx_set_group): every vector sharded over the group's ranks
  kgs_group* group = nullptr;
  int group_rank = 0;
  int srs_slice_rank = 0, srs_slice_world = 1;  // of the loaded SRS (SrsTables::slice_*)
  std::map<std::string, uint32_t*> dist_tabs;  // per-rank coset / 1/(n(x-1)) tables (pool buffers)
  ExchangeStats xs;                             // exchanges of the last distributed proof
  bool dist_err_agreed = false;  // the distributed proof's current failure is the same on every rank

  ~kgs_ctx() {
    hipSetDevice(device);
    // every stream may still read pool buffers or pinned staging: drain all before freeing. A drain
    // that fails is reported here, naming the stream: HIP errors are sticky, and unreported the fault
    // would surface at the next checked call of whatever runs next in the process (round 5's fault
    // surfaced that way in the NEXT test's first copy, profiles/r05/boundary/feed_per_piece_dma_fault.log)
    for (const auto& s : streams()) {
      if (!s.st) continue;
      const hipError_t e = hipStreamSynchronize(s.st);
      if (e != hipSuccess)
        fprintf(stderr, "kgs: context on device %d: its %s stream failed while draining at destruction: %s\n", device,
                s.name, hipGetErrorString(e));
    }
    for (auto& kv : pool) hipFree(kv.second.p);
    if (h_pin) hipHostFree(h_pin);
    if (h_io) hipHostFree(h_io);
    if (h_in) hipHostFree(h_in);
    if (ev_fork) hipEventDestroy(ev_fork);
    if (ev_join) hipEventDestroy(ev_join);
    for (hipEvent_t e : ev_in) hipEventDestroy(e);
    for (hipEvent_t e : ev_wb) hipEventDestroy(e);
    if (st_wb) hipStreamDestroy(st_wb);
    if (st_copy) hipStreamDestroy(st_copy);
    if (st2) hipStreamDestroy(st2);
    if (st) hipStreamDestroy(st);
    {
      std::lock_guard<std::mutex> lk(g_reg_mu);  // shared tables are released under the registry lock
      srs.reset();
      dom.reset();
    }
  }

  // every stream of the context, created or not yet (nullptr), with the name a report gives it
  struct NamedStream { hipStream_t st; const char* name; };
  std::array<NamedStream, 4> streams() const {
    return {{{st, "main"}, {st2, "lane 2"}, {st_copy, "input copy"}, {st_wb, "write-back"}}};
  }

  // A failed (re)allocation leaves the slot empty (bytes = 0), never a stale size over a freed block.
  uint32_t* buf(const std::string& name, size_t bytes) {
    DBuf& b = pool[name];
    if (b.bytes < bytes) {
      if (b.p) {
        sync();  // any stream may still use the old block
        HC(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
      }
      const size_t sz = bytes < 64 ? 64 : bytes;
      HC(dev_malloc(&b.p, sz));
      b.bytes = sz;
    }
    return (uint32_t*)b.p;
  }
  // a grow-only pinned host area: the old block is freed only after every stream is drained
  void grow_pinned(uint8_t*& p, size_t& have, size_t bytes, unsigned flags = hipHostMallocDefault) {
    if (have >= bytes) return;
    if (p) {
      sync();
      HC(hipHostFree(p));
      p = nullptr;
      have = 0;
    }
    HC(hipHostMalloc((void**)&p, bytes, flags));
    have = bytes;
  }
  uint8_t* io_in(size_t bytes) {
    static const bool wc = [] {
      const char* e = getenv("KGS_STAGE_WC");
      return e && !strcmp(e, "1");
    }();
    grow_pinned(h_in, h_in_bytes, bytes, wc ? hipHostMallocWriteCombined : hipHostMallocDefault);
    return h_in;
  }
  uint8_t* io(size_t bytes) {
    grow_pinned(h_io, h_io_bytes, bytes);
    return h_io;
  }
  void ensure_pin(size_t bytes) {
    if (h_pin_bytes < bytes) h_pin_off = 0;
    grow_pinned(h_pin, h_pin_bytes, bytes);
  }
  // bump-allocated pinned region (valid until reset_staging(), i.e. until the next sync point)
  uint8_t* pin(size_t bytes) {
    bytes = (bytes + 63) & ~size_t(63);
    if (h_pin_off + bytes > h_pin_bytes) throw KgsError(KGS_E_ARG, "pinned staging exhausted");
    uint8_t* p = h_pin + h_pin_off;
    h_pin_off += bytes;
    return p;
  }
  // copy host scalars to the device scalar area; returns the device pointer
  uint32_t* scal(const Fr* v, int count) {
    size_t bytes = 32 * (size_t)count;
    if (d_scal_off + bytes > SCAL_BYTES) throw KgsError(KGS_E_ARG, "scalar staging exhausted");
    uint8_t* h = pin(bytes);
    for (int i = 0; i < count; i++) v[i].to_bytes(h + 32 * i);
    uint32_t* d = d_scal + d_scal_off / 4;
    d_scal_off += bytes;
    HC(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    return d;
  }
  void sync() {
    for (const auto& s : streams())
      if (group && s.st == st) group->wait(st);  // the main stream carries the group's exchanges
      else if (s.st) HC(hipStreamSynchronize(s.st));
  }
  void reset_staging() {
    sync();
    h_pin_off = 0;
    d_scal_off = 0;
  }
  void use_srs(const std::shared_ptr<SrsTables>& s) {
    srs = s;
    tb = s ? s->tb : MsmTables{};
    srs_power = s ? s->power : -1;
    nbits_max = s ? s->nbits_max : -1;
    srs_slice_rank = s ? s->slice_rank : 0;
    srs_slice_world = s ? s->slice_world : 1;
  }
  void use_domain(const std::shared_ptr<DomainTables>& d) {
    dom = d;
    logM = d->logM;
    tw_fwd = d->tw_fwd;
    tw_inv = d->tw_inv;
    coset_pow = d->coset_pow;
    coset_ipow = d->coset_ipow;
    invm = d->invm;
  }
};


namespace kgsi {

// ------------------------------------------------------------------ building blocks (prover.cpp)
// twin: also the tables' 29-bit twin (false only for the reference-quirks replay's growth)
void ensure_domain(kgs_ctx& c, int logM, bool twin = true);
void ensure_twin(kgs_ctx& c);  // the context's domain gets its twin if it was grown without one
uint32_t* get_nxm1(kgs_ctx& c, int nbits, int lcs);
void intt_nat(kgs_ctx& c, uint32_t* out, const uint32_t* in, int logm, hipStream_t st = nullptr);
// coefficients (len <= 2^lcs) -> coset evaluations p(g w^i), bit-reversed order
void coset_fwd(kgs_ctx& c, uint32_t* out, const uint32_t* in, uint64_t len, int lcs, hipStream_t st = nullptr);
// bit-reversed coset evaluations ALREADY SCALED BY 1/2^lcs -> natural coefficients (in place allowed);
// the quotient takes its 1/cs from the Z_H scalars and get_nxm1's table
void coset_inv_prescaled(kgs_ctx& c, uint32_t* out, const uint32_t* in, int lcs);

// reference-quirks mode (ref_quirks.cpp; kgs_ctx_set_reference_quirks)
uint32_t* ref_quirks_probe(kgs_ctx& c, uint64_t n, const std::vector<const uint32_t*>& ops, const uint32_t* Q,
                           uint64_t qlen);
bool ref_quirks_needed(const uint32_t* probe, size_t nops, uint64_t n);
bool ref_quotient_is_zero(const uint32_t* probe);
uint32_t* ref_quirks_quotient(kgs_ctx& c, bool gs, bool sel, bool lookup, int nbits, const Fr& alpha, const Fr& gamma,
                              const uint32_t* dF, const uint32_t* dT, const uint32_t* dS, const uint32_t* dSF,
                              const uint32_t* dST, uint64_t& qlen, uint32_t*& fmut);

// ------------------------------------------------------------------ SRS and commitment MSM (msm_commit.cpp)
#define CTX_LOCK(c) std::lock_guard<std::mutex> ctx_lock_(c->mu)
// The window rule of both MSMs: clamp(ceil(log2 n) - 4, c_min, c_max); the environment variable
// env_name overrides it for A/B timing when its value lies in [c_min, env_max] (else it is ignored)
int choose_window(uint64_t n, int c_min, int c_max, const char* env_name, int env_max);
int choose_c(uint64_t npts);
// w's buffers from the context's pool, named prefix + <buffer> + suffix, of the sizes z
void msm_work_from_pool(kgs_ctx& c, MsmWork& w, const std::string& prefix, const std::string& suffix,
                        const MsmSizes& z);
void ensure_msm_work(kgs_ctx& c);
void load_points(kgs_ctx& c, const uint8_t* lem, uint64_t npts, int power, int nbits_max, const std::string& file,
                 int srank = 0, int sworld = 1);
// MSM commitment: device Pippenger -> c bit-sum points T_k (this rank's partial, pinned host)
struct Commit {
  uint8_t* h_T = nullptr;   // pinned, c x 128 B (this rank's partial)
  uint64_t N = 0;
  uint8_t* h_T2 = nullptr;  // second point range's partial (commit_launch_split), or nullptr
};
void shard_range(uint64_t n, int rank, int world, uint64_t& lo, uint64_t& hi);
hipStream_t copy_stream();  // a new stream for the host-boundary copies (st_copy, st_wb)
void fork_lanes(kgs_ctx& c);
// work issued on `to` after this waits for everything issued on `from` so far
void lane_join(kgs_ctx& c, hipStream_t from, hipStream_t to);
Commit commit_launch(kgs_ctx& c, const uint32_t* scalars, uint64_t N, int slot, int lane = 0);
// latency mode (two MSM lanes, one unsharded context): points [0, cut) on lane 0 and [cut, N) on
// lane 1 (slots slot, slot + 1); the two partials are summed by commits_finish. Otherwise the same
// as commit_launch on `lane`.
Commit commit_launch_split(kgs_ctx& c, const uint32_t* scalars, uint64_t N, uint64_t cut, int slot);
bool split_commits(const kgs_ctx& c);
// MSM over `count` scalars whose SRS points are pbase + pstride * i (a rank's slice of a
// distributed polynomial); N = the polynomial's global point count (0: infinity)
Commit commit_launch_slice(kgs_ctx& c, const uint32_t* scalars, uint64_t count, uint64_t pbase, uint64_t pstride,
                           uint64_t N, int slot, int lane = 0);
void combine_partials(const uint8_t* T_all, size_t part_stride, int nparts, int cc, uint8_t out[64]);
// all-gather of per-rank partials (nullptr: this rank alone) -> affine LEM commitments
using HostAllgather = std::function<void(const void* send, void* recv, size_t bytes)>;
void commits_finish(kgs_ctx& c, const std::vector<Commit>& cms, std::vector<uint8_t*> outs);
void commits_finish_with(kgs_ctx& c, const std::vector<Commit>& cms, std::vector<uint8_t*> outs, int world,
                         const HostAllgather& ag);
void commit_finish(kgs_ctx& c, const Commit& cm, uint8_t out[64]);
// The variable-base MSM over a row already in msm_points_run's form (msm_points.cpp): n >= 1 device
// scalars in standard form, window_c as for kgs_msm_points, the call's own "mp_*" buffers, the host
// finish. Ends with the main stream drained.
void msm_points_over_row(kgs_ctx& c, const uint32_t* row29, const uint32_t* d_scalars_std, uint64_t n, int window_c,
                         uint8_t out[64]);

// Horner evaluations (tile partials on the device, tile combine on the host)
struct EvalJob {
  std::vector<const uint32_t*> src;
  std::vector<uint64_t> len;
  uint8_t* h_part = nullptr;
  uint32_t ntiles = 0;
  Fr x;
};
uint32_t* xpowers(kgs_ctx& c, const Fr& x);
void fr29_record(const Fr& x, Fr out[2]);
EvalJob eval_launch(kgs_ctx& c, const std::vector<const uint32_t*>& src, const std::vector<uint64_t>& len, const Fr& x,
                    int slot);
std::vector<Fr> eval_finish(const EvalJob& j);

// out[i] = sum_k coef_k * src_k[i] (zero beyond len_k) + (i == 0 ? c0 : 0), any number of terms
struct LcTerms {
  std::vector<const uint32_t*> src;
  std::vector<uint64_t> len;
  std::vector<Fr> coef;
  Fr c0 = Fr::zero();
  void add(const uint32_t* s, uint64_t l, const Fr& k) {
    src.push_back(s);
    len.push_back(l);
    coef.push_back(k);
  }
};
void run_lincomb(hipStream_t st, uint32_t* out, uint64_t n, const LcTerms& t);

// Round 3's launch sequence (prover.cpp), shared by the round engine and the test primitives of kgs.h
// (kgs_quotient_ex, kgs_divcheck). One argument's device vectors: on H in natural order for the
// divisibility check (S, fcomb, tcomb, selectors), on the coset in bit-reversed order for the quotient.
struct QuotIn {
  int kind = 0;
  const uint32_t *S = nullptr, *F = nullptr, *T = nullptr, *SF = nullptr, *ST = nullptr;  // SF, ST: nullptr unselected
  bool gs() const { return kind != KGS_GRANDPRODUCT; }
  bool lk() const { return kind == KGS_LOOKUP; }
  bool sel() const { return SF != nullptr; }
};
// Stages the argument's nine quotient scalars (alpha, gamma, the two 1/Z_H / cs, alpha_t, the two alpha / Z_H
// records) on the main stream and enqueues its divisibility check there: *flag |= 1 if some
// N(w^(gbase + i)) != 0, i < n (poly.hip k_divcheck; S_next == nullptr: the wrap S[0]). Returns the staged
// set, which run_quotient takes for argument 0. The check itself reads alpha, gamma and alpha_t only, so a
// caller without a coset (kgs_divcheck) passes nbits = lcs = 0.
const uint32_t* run_divcheck(kgs_ctx& c, int nbits, int lcs, const QuotIn& a, const Fr& alpha, const Fr& gamma, uint64_t n,
                             uint32_t* flag, const uint32_t* S_next = nullptr, uint64_t gbase = 0);
// Q = (sum_j dpow[j] N_j) / Z_H / cs on the coset of 2^lcs points, into Qc on the main stream: k_quotient
// for one argument, with `fused` (the multi-argument prover, always) k_quotient_multi in groups of QM_MAX,
// the later groups accumulating. qs0: argument 0's scalar set if run_divcheck has staged it (else it is
// staged here). The 1/(n(x - 1)) table is get_nxm1's (a cache hit in a proof: round 2 has built it).
void run_quotient(kgs_ctx& c, int nbits, int lcs, const std::vector<QuotIn>& args, const Fr& alpha, const Fr& gamma,
                  const std::vector<Fr>& dpow, uint32_t* Qc, bool fused, const uint32_t* qs0 = nullptr);

// ------------------------------------------------------------------ the protocol rounds (prover_rounds.cpp)
enum R5Poly { R5_S, R5_Q, R5_F, R5_T, R5_SELF, R5_SELT, R5_POLT };

// One argument of a proof. The shape arithmetic of the protocol lives here and nowhere else.
struct ArgIn {
  int kind = 0, k = 0;
  std::vector<const uint32_t*> f_std, t_std;          // device, standard form
  const uint32_t *sel_f = nullptr, *sel_t = nullptr;  // device, Montgomery (nullptr: unselected)
  bool gs() const { return kind != KGS_GRANDPRODUCT; }  // KGS_LOOKUP is a selected grand-sum
  bool lk() const { return kind == KGS_LOOKUP; }
  bool sel() const { return sel_f != nullptr; }
  int ncom_r1() const { return 2 * k + (sel() ? 2 : 0); }                  // round-1 commitments
  int nev_xi() const { return (gs() ? 2 : 1) * k + (sel() ? 2 : 0); }      // openings at xi
  // fn(R5Poly, index) for every polynomial opened at xi. Proof (and transcript) order interleaves
  // F_0 [T_0] F_1 [T_1] ...; the powers of v in W_xi run over every F_i, then every T_i. A grand
  // product does not open its T_i. The selectors come last in both.
  template <class Fn>
  void each_xi(bool by_power, Fn fn) const {
    for (int i = 0; i < k; i++) {
      fn(R5_F, i);
      if (gs() && !by_power) fn(R5_T, i);
    }
    for (int i = 0; i < k && gs() && by_power; i++) fn(R5_T, i);
    if (sel()) {
      fn(R5_SELF, 0);
      fn(R5_SELT, 0);
    }
  }
};

// an argument's polynomials in coefficient form (device), as round 5 names them
struct ArgPolys {
  std::vector<uint32_t*> Fc, Tc;
  uint32_t *sFc = nullptr, *sTc = nullptr, *Sc = nullptr;
  const uint32_t *polT = nullptr, *Qc = nullptr;
  const uint32_t* poly(R5Poly id, int idx) const {
    switch (id) {
      case R5_S: return Sc;
      case R5_Q: return Qc;
      case R5_F: return Fc[idx];
      case R5_T: return Tc[idx];
      case R5_SELF: return sFc;
      case R5_SELT: return sTc;
      case R5_POLT: return polT;
    }
    return nullptr;
  }
};

// an argument's round-4 values at xi; unpack() takes them in proof order (ArgIn::each_xi)
struct XiEvals {
  std::vector<Fr> fx, tx;
  Fr sFx = Fr::zero(), sTx = Fr::zero();
  Fr& at(R5Poly id, int idx) { return id == R5_F ? fx[idx] : id == R5_T ? tx[idx] : id == R5_SELF ? sFx : sTx; }
  const Fr& at(R5Poly id, int idx) const { return const_cast<XiEvals*>(this)->at(id, idx); }
  const Fr* unpack(const ArgIn& a, const Fr* ev) {
    fx.assign(a.k, Fr::zero());
    tx.assign(a.k, Fr::zero());
    a.each_xi(false, [&](R5Poly id, int i) { at(id, i) = *ev++; });
    return ev;
  }
};

// The host-boundary hooks of kgs_prove (all empty for device-resident inputs). Input vectors are numbered
// F_i at 2i, T_i at 2i + 1, then selF, selT.
struct HostHooks {
  std::vector<uint8_t*> mont_f_out, mont_t_out;  // host outputs (may be empty)
  std::function<void()> after_round1;             // called once round 1 is synchronised (write-back on st_wb)
  // per input vector an event the vector's first kernel waits for, or nullptr (already ordered on the
  // main stream)
  std::vector<hipEvent_t> ready;
  // blocks until vector v's DMA (and ready[v]) has been enqueued; null: all already are
  std::function<void(size_t)> input_issued;
};
struct ProveIn : HostHooks {
  int kind, nbits, npols;
  std::vector<const uint32_t*> f_std, t_std;  // device, standard form
  const uint32_t *sel_f = nullptr, *sel_t = nullptr;  // device, Montgomery (nullptr: unselected)
  ArgIn arg() const {
    ArgIn a;
    a.kind = kind;
    a.k = npols;
    a.f_std = f_std;
    a.t_std = t_std;
    a.sel_f = sel_f;
    a.sel_t = sel_t;
    return a;
  }
};

struct R5Term {
  R5Poly id;
  int idx;  // vector index for R5_F / R5_T
  Fr coef;
};
struct R5 {
  Fr c0;
  std::vector<R5Term> terms;
};
// one argument's linearisation r_j (prover.cpp): c0 and the coefficients of S, polT and Q
R5 round5_terms(bool gs, bool sel, int k, int nbits, const Fr& alpha, const Fr& beta, const Fr& gamma, const Fr& xi,
                const std::vector<Fr>& fx, const std::vector<Fr>& tx, const Fr& sFx, const Fr& sTx, const Fr& sxiw,
                bool lookup, const Fr* fxi_override = nullptr);
// W_xi's numerator of m >= 1 arguments (prover.cpp), shared by the round engine (len = n) and the
// distributed prover (len = its slice length, c0 kept on rank 0 only)
struct OpenArg {
  const ArgIn* in;
  const ArgPolys* polys;
  const XiEvals* x;
  Fr sxiw;
};
LcTerms wxi_numerator(const std::vector<OpenArg>& args, int nbits, const Fr& alpha, const Fr& beta, const Fr& gamma,
                      const std::vector<Fr>& dpow, const Fr& xi, const Fr& v, const uint32_t* Qc, uint64_t len,
                      uint64_t qlen, const Fr* fxi_override = nullptr);
// round 2's beta combinations of a vector argument (prover.cpp): the terms of fcomb, tcomb, polF, polT
struct BetaComb {
  LcTerms fcomb, tcomb, polF, polT;
};
BetaComb beta_combination(const std::vector<uint32_t*>& fm, const std::vector<uint32_t*>& tm,
                          const std::vector<uint32_t*>& Fc, const std::vector<uint32_t*>& Tc, int k, const Fr& beta,
                          uint64_t len);

// What distinguishes the callers of prove_rounds. The engine never infers these from the argument count.
struct RoundOpts {
  const HostHooks* hooks = nullptr;
  // round 1: each input vector's conversion, transform and commitment on the lane of its commitment
  // (else: every transform on the main stream, then the commitments alternate between the lanes)
  bool piped_round1 = false;
  // follow the reference on degenerate inputs (ref_quirks.cpp); one argument only
  bool ref_quirks = false;
  // "argument j: " in front of NOT_WELL_CALC and NOT_DIVISIBLE
  bool name_arguments = false;
};
// Rounds 1 to 5 of a proof of m >= 1 arguments over one domain. Commitments and
// evaluations in proof order; ends synchronised. The caller has checked the shapes and the SRS
// (check_srs) and holds the context.
void prove_rounds(kgs_ctx& c, int nbits, const std::vector<ArgIn>& args, const RoundOpts& o, uint8_t* com_out,
                  uint8_t* ev_out);
// the SRS preconditions every prover shares word for word
void check_srs(const kgs_ctx& c, int nbits);
// The refusals of every call that runs on one plain context only (after its mutex is held). The batch verifier and
// kgs_g1_lincomb (verify_batch.cpp) accept a sharded context and refuse the rank group alone.
inline void check_no_group(const kgs_ctx& c, const std::string& fn) {
  if (c.group) throw KgsError(KGS_E_ARG, fn + " does not run on a context attached to a rank group.");
}
inline void check_plain_ctx(const kgs_ctx& c, const char* fn) {
  check_no_group(c, fn);
  if (c.shard_world > 1)
    throw KgsError(KGS_E_ARG, std::string(fn) + " does not run on a context with MSM sharding (kgs_ctx_set_shard).");
}
std::string arg_prefix(int j);  // "argument j: "

// the per-round wall clock (kgs_last_timing) and roctx range of a proof
struct RoundClock {
  kgs_ctx& c;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  Range range{ROUND_NAMES[0]};
  explicit RoundClock(kgs_ctx& ctx) : c(ctx) {}
  void lap(int r) {
    const auto t1 = std::chrono::steady_clock::now();
    c.timing[r] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    if (r + 1 < 5) range.push(ROUND_NAMES[r + 1]);
    else range.pop();
  }
};

// in-flight contexts (one MSM lane) launch the NTT passes built to co-reside with the other proofs'
// accumulate waves, the latency mode (two lanes) the build that is fastest alone (ntt.hip, WV)
struct NttMode {
  bool prev;
  explicit NttMode(bool on) : prev(ntt_set_coresident(on)) {}
  ~NttMode() { ntt_set_coresident(prev); }
};

// The provers' error contract: a call that leaves by an exception drains every stream of the context
// first, so nothing of it still reads the caller's buffers. Rank-group contexts are left alone: their
// main stream may wait in an exchange whose peers failed (the group's abort releases it), and they
// never DMA caller memory in place.
struct DrainOnError {
  kgs_ctx* ctx;
  int unwinding = std::uncaught_exceptions();
  explicit DrainOnError(kgs_ctx* c) : ctx(c) {}
  ~DrainOnError() {
    if (std::uncaught_exceptions() <= unwinding || ctx->group) return;
    hipSetDevice(ctx->device);
    for (const auto& s : ctx->streams())
      if (s.st) (void)hipStreamSynchronize(s.st);
    (void)hipGetLastError();
  }
};

// The one rule of the rows cached on an SRS (SrsTables::lagrange, ::fk): a row is looked up and published under
// g_reg_mu (taken after the context's mutex, never the other way round), built outside it on the context's main
// stream, and published only complete, after the stream has drained. Of two contexts that build the same row at
// once the first publisher wins and the other's row is released. `build` enqueues the row and returns it; a
// failed build drains the context (DrainOnError). The caller holds the context and has checked it. Ends with the
// main stream drained when it built.
template <class Map, class Build>
std::shared_ptr<SrsRow> srs_row_cached(kgs_ctx& c, Map& rows, const typename Map::key_type& key, Build build) {
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = rows.find(key);
    if (it != rows.end()) return it->second;
  }
  DrainOnError drain(&c);
  const std::shared_ptr<SrsRow> row = build();
  HC(hipStreamSynchronize(c.st));
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto& slot = rows[key];
  if (!slot) slot = row;
  return slot;
}

// The two events of a timing helper (kgs_bench_*), destroyed however the helper leaves
struct EventTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventTimer() {
    HC(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
      hipEventDestroy(e0);
      throw KgsError(KGS_E_HIP, "HIP error: hipEventCreate failed");
    }
  }
  EventTimer(const EventTimer&) = delete;
  EventTimer& operator=(const EventTimer&) = delete;
  ~EventTimer() {
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  // the milliseconds `body` takes on st, which the call drains
  template <class Body>
  double ms(hipStream_t st, Body body) {
    HC(hipEventRecord(e0, st));
    body();
    HC(hipEventRecord(e1, st));
    check_launch();
    HC(hipEventSynchronize(e1));
    float f = 0;
    HC(hipEventElapsedTime(&f, e0, e1));
    return f;
  }
};

// ------------------------------------------------------------------ G1 transform host side (g1_ntt.cpp)
constexpr int G1_NTT_LOG_MAX = 24;
void fr_words(const Fr& x, uint32_t w[8]);
Fr ntt_root(int logm, bool inverse);  // omega_{2^logm}, or its inverse
Fr ninv_std(int logm);                // 1 / 2^logm as the standard-form words the kernels take
// the transform's work buffers ("gn_*" in the context's pool) for 2^logm points
G1NttWork ntt_work(kgs_ctx& c, int logm);
// the transform on the main stream (not synchronised); scale: nullptr, or the standard-form factor
void ntt_enqueue(kgs_ctx& c, uint32_t* out, const uint32_t* in, int logm, bool inverse, const Fr* scale_words);
// the context holds a whole SRS (not a rank's slice), or the refusals of kgs.h
void check_whole_srs(const kgs_ctx& c, const char* fn);
// check_plain_ctx, check_whole_srs, and that SRS can serve 2^nbits Lagrange bases
void check_lagrange(const kgs_ctx& c, int nbits, const char* fn);

// the single-argument prover (prover.cpp): its checks, the rank-group dispatch, then prove_rounds
void prove_impl(kgs_ctx& c, const ProveIn& in, uint8_t* com_out, uint8_t* ev_out);
// the distributed prover (prover_dist.cpp): same inputs and outputs as prove_impl on every rank
void prove_dist_impl(kgs_ctx& c, const ProveIn& in, uint8_t* com_out, uint8_t* ev_out);
void prove_dist_group(kgs_ctx& c, const ProveIn& in, uint8_t* com_out, uint8_t* ev_out);

}  // namespace kgsi
