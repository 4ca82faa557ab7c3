// Rank groups of the distributed prover (prover_dist.cpp): the three transports behind the kgs_group
// interface of context.hpp and every kgs_group_* entry point of include/kgs.h.
//
// Transports: RCCL (one process per GPU, production), in-process (several contexts of one process:
// tests on one GPU, or one process driving several GPUs; its host rendezvous is rank_rendezvous.hpp),
// host callback (any all-gather, e.g. torch.distributed gloo; device data staged through the host).
// This is the only translation unit that uses RCCL.
#include <thread>
#include <rccl/rccl.h>

#include "context.hpp"
#include "rank_rendezvous.hpp"

using namespace kgs;
using namespace kgsi;

// (the kgs_group interface is in context.hpp: kgs_ctx::sync drains the main stream through it)
double group_timeout_s() {
  static const double t = [] {
    const char* e = getenv("KGS_GROUP_TIMEOUT_S");
    const double v = e ? atof(e) : 0.0;
    return v > 0 ? v : 120.0;
  }();
  return t;
}

namespace {

// several contexts of one process, driven by one host thread per rank
struct LocalGroup : kgs_group {
  RankRendezvous rv;  // barriers, abort and the published send pointers (rv.sp)
  std::mutex mu;
  std::vector<int> dev;
  std::vector<int> attached;  // device of each attached rank (-1: none yet)

  explicit LocalGroup(int w) : rv(w, group_timeout_s()), dev(w), attached(w, -1) { world = w; }

  // `a` reads from / writes to `b`'s memory in the all-to-all (hipMemcpyPeerAsync): without peer
  // access the runtime would stage the copy through the host, so a pair without it fails up front
  static void enable_peer(int a, int b) {
    int can = 0;
    HC(hipDeviceCanAccessPeer(&can, a, b));
    if (!can)
      throw KgsError(KGS_E_COMM, "in-process rank group: device " + std::to_string(a) + " has no peer access to device " +
                                     std::to_string(b) + " (hipDeviceCanAccessPeer); use one process per GPU (RCCL)");
    int cur = 0;
    HC(hipGetDevice(&cur));
    HC(hipSetDevice(a));
    const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
    (void)hipGetLastError();
    HC(hipSetDevice(cur));
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
      throw KgsError(KGS_E_COMM, std::string("in-process rank group: hipDeviceEnablePeerAccess failed: ") + hipGetErrorString(e));
  }
  void attach(int rank, int device) override {
    std::lock_guard<std::mutex> lk(mu);
    for (int j = 0; j < world; j++)
      if (j != rank && attached[j] >= 0 && attached[j] != device) {
        enable_peer(device, attached[j]);
        enable_peer(attached[j], device);
      }
    attached[rank] = device;
  }
  void abort() override { rv.abort(); }
  void allgather(int rank, const void* send, void* recv, size_t bytes) override { rv.allgather(rank, send, recv, bytes); }
  void alltoall(int rank, kgs_ctx& c, hipStream_t st, const void* send, void* recv, size_t chunk) override {
    HC(hipStreamSynchronize(st));  // send is complete
    rv.sp[rank] = send;
    dev[rank] = c.device;
    rv.barrier();
    for (int j = 0; j < world; j++) {
      uint8_t* dst = (uint8_t*)recv + (size_t)j * chunk;
      const uint8_t* src = (const uint8_t*)rv.sp[j] + (size_t)rank * chunk;
      if (dev[j] == c.device) HC(hipMemcpyAsync(dst, src, chunk, hipMemcpyDeviceToDevice, st));
      else HC(hipMemcpyPeerAsync(dst, c.device, src, dev[j], chunk, st));  // peer access: attach()
    }
    HC(hipStreamSynchronize(st));
    rv.barrier();  // nobody overwrites a send buffer a peer is still reading
  }
};

// host callbacks (torch.distributed gloo, MPI ...): device data staged through the host. With an
// all-to-all callback each rank sends chunk j to rank j and receives one chunk from each rank
// ((W - 1) / W of its vector leaves it); with only the all-gather, every rank receives every rank's
// whole vector (W x the data) and keeps its chunks.
struct HostGroup : kgs_group {
  kgs_allgather_fn fn;
  kgs_alltoall_fn a2a_fn;
  void* user;
  std::vector<uint8_t> h_send, h_recv;
  HostGroup(int w, kgs_allgather_fn f, kgs_alltoall_fn a, void* u) : fn(f), a2a_fn(a), user(u) { world = w; }
  void allgather(int, const void* send, void* recv, size_t bytes) override {
    if (fn(user, (const uint8_t*)send, (uint8_t*)recv, bytes) != 0) throw KgsError(KGS_E_COMM, "group all-gather failed");
  }
  uint64_t alltoall_wire_bytes(size_t chunk) const override {
    return a2a_fn ? (uint64_t)chunk * (world - 1) : (uint64_t)chunk * world * (world - 1);
  }
  void alltoall(int rank, kgs_ctx&, hipStream_t st, const void* send, void* recv, size_t chunk) override {
    const size_t bytes = chunk * world;
    if (h_send.size() < bytes) h_send.resize(bytes);
    HC(hipMemcpyAsync(h_send.data(), send, bytes, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    if (a2a_fn) {
      if (h_recv.size() < bytes) h_recv.resize(bytes);
      if (a2a_fn(user, h_send.data(), h_recv.data(), (uint64_t)chunk) != 0) throw KgsError(KGS_E_COMM, "group all-to-all failed");
      HC(hipMemcpyAsync(recv, h_recv.data(), bytes, hipMemcpyHostToDevice, st));
    } else {
      if (h_recv.size() < bytes * world) h_recv.resize(bytes * world);
      allgather(rank, h_send.data(), h_recv.data(), bytes);
      for (int j = 0; j < world; j++)
        HC(hipMemcpyAsync((uint8_t*)recv + (size_t)j * chunk, h_recv.data() + (size_t)j * bytes + (size_t)rank * chunk,
                          chunk, hipMemcpyHostToDevice, st));
    }
    HC(hipStreamSynchronize(st));
  }
};

#define NC(x)                                                                                           \
  do {                                                                                                  \
    ncclResult_t r_ = (x);                                                                              \
    if (r_ != ncclSuccess) throw KgsError(KGS_E_COMM, std::string("RCCL error: ") + ncclGetErrorString(r_) + " at " #x); \
  } while (0)

// one process per GPU: RCCL communicator, all-to-all as grouped send/recv on the prover's stream
struct RcclGroup : kgs_group {
  ncclComm_t comm = nullptr;
  int device = 0;
  hipStream_t st_small = nullptr;
  void* d_small = nullptr;
  size_t small_bytes = 0;
  ~RcclGroup() override {
    hipSetDevice(device);
    if (comm) ncclCommDestroy(comm);
    if (d_small) hipFree(d_small);
    if (st_small) hipStreamDestroy(st_small);
  }
  void allgather(int rank, const void* send, void* recv, size_t bytes) override {
    HC(hipSetDevice(device));
    if (!comm) throw KgsError(KGS_E_COMM, "rank group aborted");
    if (small_bytes < bytes * (world + 1)) {
      if (d_small) HC(hipFree(d_small));
      d_small = nullptr;
      small_bytes = 0;
      HC(dev_malloc(&d_small, bytes * (world + 1)));
      small_bytes = bytes * (world + 1);
    }
    uint8_t* ds = (uint8_t*)d_small;
    HC(hipMemcpyAsync(ds, send, bytes, hipMemcpyHostToDevice, st_small));
    NC(ncclAllGather(ds, ds + bytes, bytes, ncclUint8, comm, st_small));
    HC(hipMemcpyAsync(recv, ds + bytes, bytes * world, hipMemcpyDeviceToHost, st_small));
    wait(st_small);
    (void)rank;
  }
  // RCCL collectives are stream-ordered: a peer that never joins leaves the stream pending forever
  // (and ncclCommAbort on the failing rank does not release the others). Poll the stream and the
  // communicator's asynchronous error against the group deadline; on expiry or error abort this
  // rank's communicator too and fail, so every rank of a broken group ends with an error.
  void wait(hipStream_t st) override {
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::duration<double>(group_timeout_s());
    for (unsigned spin = 0;; spin++) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) return;
      if (q != hipErrorNotReady) throw KgsError(KGS_E_HIP, std::string("HIP error: ") + hipGetErrorString(q) + " (stream query)");
      ncclResult_t ae = ncclSuccess;
      if (comm && ncclCommGetAsyncError(comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
        abort();
        throw KgsError(KGS_E_COMM, std::string("RCCL asynchronous error: ") + ncclGetErrorString(ae));
      }
      if (!comm) throw KgsError(KGS_E_COMM, "rank group aborted");
      if (std::chrono::steady_clock::now() > t_end) {
        abort();
        throw KgsError(KGS_E_COMM, "rank group exchange timed out (a peer rank failed or hung; KGS_GROUP_TIMEOUT_S)");
      }
      if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
  }
  void alltoall(int, kgs_ctx&, hipStream_t st, const void* send, void* recv, size_t chunk) override {
    if (!comm) throw KgsError(KGS_E_COMM, "rank group aborted");
    NC(ncclGroupStart());
    for (int j = 0; j < world; j++) {
      NC(ncclSend((const uint8_t*)send + (size_t)j * chunk, chunk, ncclUint8, j, comm, st));
      NC(ncclRecv((uint8_t*)recv + (size_t)j * chunk, chunk, ncclUint8, j, comm, st));
    }
    NC(ncclGroupEnd());
  }
  void abort() override {
    if (comm) ncclCommAbort(comm);
    comm = nullptr;
  }
};

void check_world(int world) {
  if (world < 1 || world > 16 || (world & (world - 1))) throw KgsError(KGS_E_ARG, "group world must be 1, 2, 4, 8 or 16");
}

}  // namespace

extern "C" {

int kgs_group_create_local(int world, kgs_group_t** out) {
  API_BEGIN
  if (!out) throw KgsError(KGS_E_ARG, "NULL argument");
  check_world(world);
  *out = new LocalGroup(world);
  API_END
}

int kgs_group_create_host(int world, kgs_allgather_fn fn, void* user, kgs_group_t** out) {
  API_BEGIN
  if (!out || !fn) throw KgsError(KGS_E_ARG, "NULL argument");
  check_world(world);
  *out = new HostGroup(world, fn, nullptr, user);
  API_END
}

int kgs_group_create_host_a2a(int world, kgs_allgather_fn fn, kgs_alltoall_fn a2a, void* user, kgs_group_t** out) {
  API_BEGIN
  if (!out || !fn || !a2a) throw KgsError(KGS_E_ARG, "NULL argument");
  check_world(world);
  *out = new HostGroup(world, fn, a2a, user);
  API_END
}

int kgs_last_exchange(kgs_ctx_t* ctx, double* out, int max) {
  if (!ctx || !out) return KGS_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const ExchangeStats& x = ctx->xs;
  const double v[6] = {(double)x.a2a_n, x.a2a_ms, (double)x.a2a_bytes, (double)x.ag_n, x.ag_ms, (double)x.ag_bytes};
  const int n = max < 6 ? max : 6;
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

int kgs_group_rccl_unique_id(uint8_t id[128]) {
  API_BEGIN
  if (!id) throw KgsError(KGS_E_ARG, "NULL argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId u;
  NC(ncclGetUniqueId(&u));
  memcpy(id, &u, 128);
  API_END
}

int kgs_group_create_rccl(int rank, int world, const uint8_t id[128], int device, kgs_group_t** out) {
  API_BEGIN
  if (!out || !id) throw KgsError(KGS_E_ARG, "NULL argument");
  check_world(world);
  if (rank < 0 || rank >= world) throw KgsError(KGS_E_ARG, "bad rank");
  HC(hipSetDevice(device));
  auto* g = new RcclGroup();
  g->world = world;
  g->device = device;
  try {
    HC(hipStreamCreateWithFlags(&g->st_small, hipStreamNonBlocking));
    ncclUniqueId u;
    memcpy(&u, id, 128);
    NC(ncclCommInitRank(&g->comm, world, u, rank));
  } catch (...) {
    delete g;
    throw;
  }
  *out = g;
  API_END
}

void kgs_group_destroy(kgs_group_t* g) { delete g; }

int kgs_group_world(kgs_group_t* g, int* world) {
  if (!g || !world) return KGS_E_ARG;
  *world = g->world;
  return KGS_OK;
}

int kgs_ctx_set_group(kgs_ctx_t* ctx, kgs_group_t* g, int rank) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (g && (rank < 0 || rank >= g->world)) throw KgsError(KGS_E_ARG, "bad rank for this group");
  if (g) g->attach(rank, ctx->device);
  ctx->group = g;  // a world-1 group runs the distributed code path on one rank (transport check)
  ctx->group_rank = ctx->group ? rank : 0;
  API_END
}

}  // extern "C"
