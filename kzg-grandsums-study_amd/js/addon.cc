// N-API addon (Node >= 12, N-API 8) binding the C-ABI of libkgs.so (include/kgs.h) for the
// JavaScript drop-in modules in js/src. Heavy calls (SRS load, prove) run in napi_async_work and
// return Promises, like the reference's async module API.
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <map>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kgs.h"

#define NAPI_CALL(env, call)                                        \
  do {                                                              \
    if ((call) != napi_ok) {                                        \
      napi_throw_error((env), nullptr, "N-API call failed: " #call); \
      return nullptr;                                               \
    }                                                               \
  } while (0)

static kgs_ctx_t* get_ctx(napi_env env, napi_value v) {
  void* p = nullptr;
  napi_get_value_external(env, v, &p);
  return (kgs_ctx_t*)p;
}

static std::vector<uint8_t> bytes_of(napi_env env, napi_value v) {
  std::vector<uint8_t> out;
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) {
    napi_typedarray_type t;
    size_t len;
    void* data;
    napi_value ab;
    size_t off;
    napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off);
    out.assign((uint8_t*)data, (uint8_t*)data + len);
    return out;
  }
  bool is_buf = false;
  napi_is_buffer(env, v, &is_buf);
  if (is_buf) {
    void* data;
    size_t len;
    napi_get_buffer_info(env, v, &data, &len);
    out.assign((uint8_t*)data, (uint8_t*)data + len);
  }
  return out;
}

// zero-copy view of a Uint8Array / Buffer argument, kept alive by a reference until the async
// work completes (ArrayBuffer backing stores do not move)
struct View {
  const uint8_t* p = nullptr;
  size_t len = 0;
};
static View view_of(napi_env env, napi_value v, std::vector<napi_ref>& refs) {
  View out;
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) {
    napi_typedarray_type t;
    size_t len;
    void* data;
    napi_value ab;
    size_t off;
    napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off);
    out.p = (const uint8_t*)data;
    out.len = len;
  } else {
    bool is_buf = false;
    napi_is_buffer(env, v, &is_buf);
    if (is_buf) {
      void* data;
      size_t len;
      napi_get_buffer_info(env, v, &data, &len);
      out.p = (const uint8_t*)data;
      out.len = len;
    }
  }
  napi_ref r;
  if (napi_create_reference(env, v, 1, &r) == napi_ok) refs.push_back(r);
  return out;
}

// Output buffers handed to JS (the Montgomery forms the reference writes back into the caller's
// Evaluations, prover.js:147-148): 64 MiB per proof at n = 2^20. Fresh malloc'd memory costs a page
// fault per 4 KiB (16 K per buffer) on first touch and an munmap on release, which under several
// concurrent proofs serialise on the process's memory map. So: 2 MiB-aligned anonymous mappings
// with MADV_HUGEPAGE (32x fewer faults where transparent huge pages are enabled), recycled through a
// free list when the JS garbage collector releases them (up to 2 GiB cached), and reported to V8 as
// external memory so that collection keeps pace with the proofs.
namespace {
std::mutex g_out_mu;
std::multimap<size_t, void*> g_out_free;
size_t g_out_cached = 0;
constexpr size_t OUT_CACHE_MAX = (size_t)2 << 30;
constexpr size_t HUGE = (size_t)2 << 20;

size_t out_round(size_t len) { return (len + HUGE - 1) / HUGE * HUGE; }

// KGS_JS_OUT_REGISTER=1: pin every output buffer for its life so the write-back is DMA'd in place.
// Off by default: registering a fresh 32 MiB buffer inside the call costs more than the staging copy
// it saves whenever the caller keeps its outputs (profiles/r03/boundary_ab.txt, profiles/r04/js/). A pool
// of pre-registered, pre-faulted spares topped up by a background thread was tried too (round 4):
// no faster, and the thread's registrations kept the process from exiting.
bool out_registered() {
  static const bool reg = getenv("KGS_JS_OUT_REGISTER") != nullptr;
  return reg;
}

uint8_t* out_map(size_t sz) {
  // over-allocate by one huge page to align the start, then trim the ends
  void* raw = mmap(nullptr, sz + HUGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (raw == MAP_FAILED) return nullptr;
  uintptr_t a = ((uintptr_t)raw + HUGE - 1) & ~(uintptr_t)(HUGE - 1);
  if (a > (uintptr_t)raw) munmap(raw, a - (uintptr_t)raw);
  const uintptr_t end = (uintptr_t)raw + sz + HUGE;
  if (end > a + sz) munmap((void*)(a + sz), end - (a + sz));
  madvise((void*)a, sz, MADV_HUGEPAGE);
  if (out_registered() && kgs_host_register((void*)a, sz) != KGS_OK) {
    munmap((void*)a, sz);
    return nullptr;
  }
  return (uint8_t*)a;
}

uint8_t* out_alloc(size_t len) {
  const size_t sz = out_round(len);
  {
    std::lock_guard<std::mutex> lk(g_out_mu);
    auto it = g_out_free.find(sz);
    if (it != g_out_free.end()) {
      void* p = it->second;
      g_out_free.erase(it);
      g_out_cached -= sz;
      return (uint8_t*)p;
    }
  }
  return out_map(sz);
}

void out_release(uint8_t* p, size_t len) {
  const size_t sz = out_round(len);
  {
    std::lock_guard<std::mutex> lk(g_out_mu);
    if (g_out_cached + sz <= OUT_CACHE_MAX) {
      g_out_free.emplace(sz, p);
      g_out_cached += sz;
      return;
    }
  }
  if (out_registered()) kgs_host_unregister(p);
  munmap(p, sz);
}
}  // namespace


// External memory adopted by JS but not yet reported to V8. Reporting it (napi_adjust_external_memory)
// can start a full GC right there; done in the completion callback, that GC ran before the proof's
// Promise resolved (+6 ms per proof at n = 2^20). It is reported when the next proof has been
// queued instead (flush_external), so the GC overlaps that proof's GPU work. Main thread only.
static int64_t g_ext_pending = 0;
static void flush_external(napi_env env) {
  if (g_ext_pending > 0) {
    int64_t adj = 0;
    napi_adjust_external_memory(env, g_ext_pending, &adj);
    g_ext_pending = 0;
  }
}

static void out_finalize(napi_env env, void* data, void* hint) {
  const int64_t len = (int64_t)(uintptr_t)hint;
  if (g_ext_pending >= len) {
    g_ext_pending -= len;  // not reported yet
  } else {
    int64_t adj = 0;
    napi_adjust_external_memory(env, -len, &adj);
  }
  out_release((uint8_t*)data, (size_t)len);
}

// Uint8Array over an out_alloc'd buffer handed to JS without a copy (recycled by the GC finalizer)
static napi_value adopt_u8(napi_env env, uint8_t* data, size_t len) {
  napi_value ab, ta;
  if (napi_create_external_arraybuffer(env, data, len, out_finalize, (void*)(uintptr_t)len, &ab) != napi_ok) {
    out_release(data, len);
    return nullptr;
  }
  g_ext_pending += (int64_t)len;
  napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta);
  return ta;
}

static napi_value make_u8(napi_env env, const uint8_t* data, size_t len) {
  void* buf;
  napi_value ab, ta;
  napi_create_arraybuffer(env, len, &buf, &ab);
  memcpy(buf, data, len);
  napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta);
  return ta;
}

static void ctx_finalize(napi_env, void* data, void*) { kgs_ctx_destroy((kgs_ctx_t*)data); }

// ctxCreate(device) -> External
static napi_value CtxCreate(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t dev = 0;
  if (argc > 0) napi_get_value_int32(env, argv[0], &dev);
  kgs_ctx_t* ctx = nullptr;
  if (kgs_ctx_create(dev, &ctx) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  napi_value ext;
  NAPI_CALL(env, napi_create_external(env, ctx, ctx_finalize, nullptr, &ext));
  return ext;
}

// deviceCount() -> number of visible HIP devices
static napi_value DeviceCount(napi_env env, napi_callback_info) {
  int n = 0;
  if (kgs_device_count(&n) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  napi_value v;
  napi_create_int32(env, n, &v);
  return v;
}

// ptauPower(path) -> power from the ptau header (readPTauHeader, src/ptau_utils.js:3-24)
static napi_value PtauPower(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  size_t len = 0;
  napi_get_value_string_utf8(env, argv[0], nullptr, 0, &len);
  std::string path(len + 1, '\0');
  napi_get_value_string_utf8(env, argv[0], &path[0], len + 1, &len);
  path.resize(len);
  int power = 0;
  if (kgs_ptau_power(path.c_str(), &power) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  napi_value v;
  napi_create_int32(env, power, &v);
  return v;
}

// keccak256(Uint8Array) -> Uint8Array(32)
static napi_value Keccak(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::vector<uint8_t> d = bytes_of(env, argv[0]);
  uint8_t out[32];
  kgs_keccak256(d.data(), d.size(), out);
  return make_u8(env, out, 32);
}

// srsInfo(ctx) -> {power, npts, windowC}
static napi_value SrsInfo(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int power = 0, c = 0;
  uint64_t npts = 0;
  if (kgs_srs_info(get_ctx(env, argv[0]), &power, &npts, &c) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  napi_value o, v;
  napi_create_object(env, &o);
  napi_create_int32(env, power, &v);
  napi_set_named_property(env, o, "power", v);
  napi_create_double(env, (double)npts, &v);
  napi_set_named_property(env, o, "npts", v);
  napi_create_int32(env, c, &v);
  napi_set_named_property(env, o, "windowC", v);
  return o;
}

// ---------------------------------------------------------------- async work
struct Job {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  kgs_ctx_t* ctx = nullptr;
  int op = 0;  // 0 = load ptau, 1 = prove, 2 = elementwise Fr map / transform (frOp),
               // 3 = one distributed proof over a rank group (proveGroup), 4 = msmPoints,
               // 5 = the multiplicities of a lookup table (lookupMultiplicities)
               // 6 = a batch of proofs against one ptau (verifyBatch)
               // 7 = one proof of several arguments (proveMulti)
               // 8 = the G1 transform (g1Ntt), 9 = a commitment from evaluations (commitEvals)
               // 10 = every opening of a polynomial on its domain (kzgOpenAll)
               // 11 = every coset opening of a polynomial (kzgOpenCosets)
               // 12 = a batch of coset openings against one SRS (kzgVerifyCosetsBatch)
               // 13 = a polynomial back from a subset of its cosets (kzgRecoverCosets)
  int rc = 0;
  std::string err;
  // load
  std::string path;
  int nbits_max = -1;
  // prove
  int kind = 0, nbits = 0, npols = 0;
  std::vector<View> f, t;
  View sf, st;
  std::vector<uint8_t*> mf, mt;  // malloc'd, adopted by JS on success
  std::vector<uint8_t> com, ev;
  std::vector<napi_ref> refs;
  bool selected = false;
  bool want_mont = true;  // false: no Montgomery write-back (the other ranks of a distributed proof)
  double exec_ms = 0;     // wall time of job_execute (the libkgs call on the worker thread)
  // diagnostics: queued (main thread) -> execute start / end (libuv worker) -> complete (main thread)
  std::chrono::steady_clock::time_point t_queue, t_exec0, t_exec1;
  // proveGroup: rank r's context, SRS slice r of W, one native thread per rank
  std::vector<kgs_ctx_t*> ranks;
  // msmPoints: bases and standard-form scalars (copied: the call returns before the work runs);
  // g1Ntt: the points in `bases`, transformed in place; commitEvals: the evaluations in `scal`;
  // kzgOpenAll / kzgOpenCosets: the coefficients in `scal`, the proofs in `bases`, the evaluations in `ev`
  // (ntt_logm = nbits, ntt_inverse = lbits)
  std::vector<uint8_t> bases, scal;
  uint8_t msm_out[64];
  int ntt_logm = 0, ntt_inverse = 0;
  // verifyBatch: the proofs' shapes and bytes (copied), the verdicts and the call's diagnostics
  std::vector<kgs_proof_ref_t> vb_refs;
  std::vector<std::vector<uint8_t>> vb_bytes;
  std::vector<uint8_t> vb_valid;
  kgs_batch_diag_t vb_diag = {};
  // kzgVerifyCosetsBatch: nbits / ntt_inverse = nBits / lBits; the commitments in `com`, commit_of / index /
  // the values / the proofs (copied), the SRS points in `bases`, [tau^l]_2 in `scal`, the seed (32 B or empty)
  std::vector<uint32_t> cb_commit_of;
  std::vector<uint64_t> cb_index;
  std::vector<uint8_t> cb_ys, cb_proofs, cb_seed;
  kgs_coset_batch_diag_t cb_diag = {};
  // kzgRecoverCosets: ntt_logm / ntt_inverse = nBits / lBits; the coset indices in cb_index, the values in cb_ys
  // (copied), the length in rc_len; the coefficients come back in `scal`, the evaluations in `ev`, the verdict in rc_ok
  uint64_t rc_len = 0;
  int rc_ok = 0;
  // op 14 (kzgOpenCosetsMany): many_polys polynomials of scal.size() / 32 / many_polys coefficients each, packed
  uint64_t many_polys = 0;
  // proveMulti: the arguments' kinds and borrowed input views
  struct MultiArg {
    int kind = 0;
    std::vector<View> f, t;
    View sf, st;
    bool selected = false;
  };
  std::vector<MultiArg> margs;
  // frOp
  int fr_op = 0;
  View in;
  uint8_t* out = nullptr;  // out_alloc'd, adopted by JS on success
  size_t out_len = 0;
};

static void prove_one(Job* j, kgs_ctx_t* ctx, bool mont, std::vector<uint8_t>& com, std::vector<uint8_t>& ev, int& rc,
                      std::string& err) {
  int nc = 0, ne = 0;
  kgs_proof_shape(j->kind, j->npols, j->selected ? 1 : 0, &nc, &ne);
  com.resize(64 * (size_t)nc);
  ev.resize(32 * (size_t)ne);
  std::vector<const uint8_t*> fp, tp;
  for (int i = 0; i < j->npols; i++) {
    fp.push_back(j->f[i].p);
    tp.push_back(j->t[i].p);
  }
  rc = kgs_prove(ctx, j->kind, j->nbits, j->npols, fp.data(), tp.data(), j->selected ? j->sf.p : nullptr,
                 j->selected ? j->st.p : nullptr, mont ? j->mf.data() : nullptr, mont ? j->mt.data() : nullptr,
                 com.data(), ev.data());
  if (rc != KGS_OK) err = kgs_last_error();
}

// the inputs' shape, and (want_mont) the output buffers of the Montgomery write-back
static bool prepare_prove(Job* j) {
  const size_t E = (size_t)32 << j->nbits;
  bool ok = true;
  for (int i = 0; i < j->npols; i++) {
    ok &= j->f[i].len == E && j->t[i].len == E;
    if (j->want_mont) {
      j->mf.push_back(out_alloc(E));
      j->mt.push_back(out_alloc(E));
      ok &= j->mf.back() && j->mt.back();
    }
  }
  if (j->selected) ok &= j->sf.len == E && j->st.len == E;
  if (!ok) {
    j->rc = KGS_E_ARG;
    j->err = "evaluation buffers must hold 2^nbits 32-byte elements";
  }
  return ok;
}

// One distributed proof: every rank on its own native thread (the group's barriers join them), so
// the ranks never compete with each other — or with the context pool's proofs — for libuv's
// thread pool (a rank waiting at a barrier for a rank that never got a pool thread would stall).
// Each rank first makes its SRS slice resident (kgs_srs_load_ptau_slice: points r + W j), then
// proves; rank 0 returns the proof and the Montgomery write-back, every rank's proof must agree.
static void group_execute(Job* j) {
  const int W = (int)j->ranks.size();
  std::vector<int> rc(W, KGS_OK);
  std::vector<std::string> err(W);
  std::vector<std::vector<uint8_t>> com(W), ev(W);
  std::vector<std::thread> th;
  for (int r = 0; r < W; r++)
    th.emplace_back([&, r] {
      rc[r] = kgs_srs_load_ptau_slice(j->ranks[r], j->path.c_str(), j->nbits, r, W);
      if (rc[r] != KGS_OK) err[r] = kgs_last_error();
      // a rank whose load failed still enters the prover: the group agrees on the failure there
      int rp = KGS_OK;
      std::string ep;
      prove_one(j, j->ranks[r], r == 0 && j->want_mont, com[r], ev[r], rp, ep);
      if (rc[r] == KGS_OK) {
        rc[r] = rp;
        err[r] = ep;
      }
    });
  for (auto& t : th) t.join();
  for (int r = 0; r < W; r++)
    if (rc[r] != KGS_OK) {
      j->rc = rc[r];
      j->err = err[r];
      return;
    }
  for (int r = 1; r < W; r++)
    if (com[r] != com[0] || ev[r] != ev[0]) {
      j->rc = KGS_E_COMM;
      j->err = "ranks of the distributed proof disagree";
      return;
    }
  j->com = com[0];
  j->ev = ev[0];
}

static void job_execute(napi_env, void* data) {
  Job* j = (Job*)data;
  const auto t0 = std::chrono::steady_clock::now();
  j->t_exec0 = t0;
  struct Stamp {
    Job* j;
    std::chrono::steady_clock::time_point t0;
    ~Stamp() {
      j->t_exec1 = std::chrono::steady_clock::now();
      j->exec_ms = std::chrono::duration<double, std::milli>(j->t_exec1 - t0).count();
    }
  } stamp{j, t0};
  if (j->op == 0) {
    j->rc = kgs_srs_load_ptau(j->ctx, j->path.c_str(), j->nbits_max);
  } else if (j->op == 2) {
    const uint64_t n = j->in.len / 32;
    j->out_len = j->in.len;
    j->out = out_alloc(j->out_len);
    if (!j->out) {
      j->rc = KGS_E_ARG;
      j->err = "out of host memory";
      return;
    }
    int logm = 0;
    while ((1ull << logm) < n) logm++;
    switch (j->fr_op) {
      case 0: j->rc = kgs_fr_to_mont(j->ctx, j->in.p, j->out, n); break;
      case 1: j->rc = kgs_fr_from_mont(j->ctx, j->in.p, j->out, n); break;
      case 2: j->rc = kgs_fr_batch_inverse(j->ctx, j->in.p, j->out, n); break;
      default: j->rc = kgs_ntt(j->ctx, j->in.p, j->out, logm, j->fr_op == 4); break;
    }
  } else if (j->op == 5) {
    j->out_len = j->f[0].len;
    j->out = out_alloc(j->out_len);
    if (!j->out) {
      j->rc = KGS_E_ARG;
      j->err = "out of host memory";
      return;
    }
    std::vector<const uint8_t*> fp, tp;
    for (int i = 0; i < j->npols; i++) {
      fp.push_back(j->f[i].p);
      tp.push_back(j->t[i].p);
    }
    j->rc = kgs_lookup_multiplicities(j->ctx, j->npols, j->out_len / 32, fp.data(), tp.data(),
                                      j->selected ? j->sf.p : nullptr, j->out);
  } else if (j->op == 6) {
    j->vb_valid.assign(j->vb_refs.size() + 1, 0);
    const int rc = kgs_verify_batch_ptau(j->ctx, j->path.c_str(), j->vb_refs.data(), (int)j->vb_refs.size(),
                                         j->vb_valid.data(), &j->vb_diag);
    j->rc = rc < 0 ? rc : KGS_OK;
  } else if (j->op == 7) {
    const size_t E = (size_t)32 << j->nbits;
    std::vector<kgs_arg_t> args(j->margs.size());
    std::vector<kgs_arg_shape_t> shapes(j->margs.size());
    std::vector<std::vector<const void*>> ptrs(2 * j->margs.size());
    bool ok = true;
    for (size_t a = 0; a < j->margs.size(); a++) {
      const Job::MultiArg& m = j->margs[a];
      for (size_t i = 0; i < m.f.size(); i++) {
        ok &= m.f[i].p && m.t[i].p && m.f[i].len == E && m.t[i].len == E;
        ptrs[2 * a].push_back(m.f[i].p);
        ptrs[2 * a + 1].push_back(m.t[i].p);
      }
      if (m.selected) ok &= m.sf.p && m.st.p && m.sf.len == E && m.st.len == E;
      args[a] = kgs_arg_t{m.kind, (int)m.f.size(), ptrs[2 * a].data(), ptrs[2 * a + 1].data(),
                          m.selected ? m.sf.p : nullptr, m.selected ? m.st.p : nullptr};
      shapes[a] = kgs_arg_shape_t{m.kind, (int)m.f.size(), m.selected ? 1 : 0};
    }
    if (!ok) {
      j->rc = KGS_E_ARG;
      j->err = "evaluation buffers must hold 2^nbits 32-byte elements";
      return;
    }
    int nc = 1, ne = 1;  // shapes the library refuses are refused by kgs_prove_multi too, before it writes
    kgs_multi_proof_shape(shapes.data(), (int)shapes.size(), &nc, &ne);
    j->com.resize(64 * (size_t)nc);
    j->ev.resize(32 * (size_t)ne);
    j->rc = kgs_prove_multi(j->ctx, j->nbits, args.data(), (int)args.size(), j->com.data(), j->ev.data());
  } else if (j->op == 3) {
    if (prepare_prove(j)) group_execute(j);
    return;
  } else if (j->op == 4) {
    j->rc = kgs_msm_points(j->ctx, j->bases.data(), j->scal.data(), j->scal.size() / 32, 0, j->msm_out);
  } else if (j->op == 8) {
    j->rc = kgs_g1_ntt(j->ctx, j->bases.data(), j->bases.data(), j->ntt_logm, j->ntt_inverse);
  } else if (j->op == 9) {
    j->rc = kgs_commit_evals(j->ctx, j->scal.data(), j->ntt_logm, j->msm_out);
  } else if (j->op == 10) {
    j->bases.resize((size_t)64 << j->ntt_logm);
    j->ev.resize((size_t)32 << j->ntt_logm);
    j->rc = kgs_kzg_open_all(j->ctx, j->scal.data(), j->scal.size() / 32, j->ntt_logm, j->bases.data(), j->ev.data());
  } else if (j->op == 11) {
    j->bases.resize((size_t)64 << (j->ntt_logm - j->ntt_inverse));
    j->ev.resize((size_t)32 << j->ntt_logm);
    j->rc = kgs_kzg_open_cosets(j->ctx, j->scal.data(), j->scal.size() / 32, j->ntt_logm, j->ntt_inverse, j->bases.data(),
                                j->ev.data());
  } else if (j->op == 14) {
    const uint64_t len = j->many_polys ? j->scal.size() / 32 / j->many_polys : 0;
    j->bases.resize(((size_t)64 << (j->ntt_logm - j->ntt_inverse)) * j->many_polys);
    j->ev.resize(((size_t)32 << j->ntt_logm) * j->many_polys);
    j->rc = kgs_kzg_open_cosets_many(j->ctx, j->scal.data(), j->many_polys, len, len, j->ntt_logm, j->ntt_inverse,
                                     j->bases.data(), j->ev.data());
  } else if (j->op == 12) {
    j->vb_valid.assign(j->cb_index.size() + 1, 0);
    const int rc = kgs_kzg_verify_cosets_batch(j->ctx, j->nbits, j->ntt_inverse, j->com.data(), j->com.size() / 64,
                                               j->cb_commit_of.data(), j->cb_index.data(), j->cb_ys.data(),
                                               j->cb_proofs.data(), j->cb_index.size(), j->bases.data(), j->scal.data(),
                                               j->cb_seed.empty() ? nullptr : j->cb_seed.data(), j->vb_valid.data(),
                                               &j->cb_diag);
    j->rc = rc < 0 ? rc : KGS_OK;
  } else if (j->op == 13) {
    j->scal.resize(32 * (size_t)j->rc_len);
    j->ev.resize((size_t)32 << j->ntt_logm);
    const int rc = kgs_kzg_recover_cosets(j->ctx, j->ntt_logm, j->ntt_inverse, j->cb_index.data(), j->cb_ys.data(),
                                          j->cb_index.size(), j->rc_len, j->scal.data(), j->ev.data());
    j->rc_ok = rc == 1;
    j->rc = rc < 0 ? rc : KGS_OK;
  } else if (j->op == 15) {
    j->scal.resize(32 * (size_t)j->rc_len * j->many_polys);
    j->ev.resize(((size_t)32 << j->ntt_logm) * j->many_polys);
    j->vb_valid.assign(j->many_polys + 1, 0);
    const int rc = kgs_kzg_recover_cosets_many(j->ctx, j->ntt_logm, j->ntt_inverse, j->many_polys, j->cb_commit_of.data(),
                                               j->cb_index.data(), j->cb_ys.data(), j->cb_index.size(), j->rc_len,
                                               j->rc_len, j->scal.data(), j->ev.data(), j->vb_valid.data());
    j->rc = rc < 0 ? rc : KGS_OK;
  } else {
    if (!prepare_prove(j)) return;
    std::string e;
    prove_one(j, j->ctx, j->want_mont, j->com, j->ev, j->rc, e);
    if (j->rc != KGS_OK) j->err = e;
    return;
  }
  if (j->rc != KGS_OK) j->err = kgs_last_error();
}

static void job_complete(napi_env env, napi_status, void* data) {
  Job* j = (Job*)data;
  if (j->rc != KGS_OK) {
    napi_value msg, err, code;
    napi_create_string_utf8(env, j->err.c_str(), NAPI_AUTO_LENGTH, &msg);
    // the reference's divZh on a zero quotient throws V8's RangeError (reference-quirks mode only)
    if (j->rc == KGS_E_RANGE) napi_create_range_error(env, nullptr, msg, &err);
    else napi_create_error(env, nullptr, msg, &err);
    napi_create_int32(env, j->rc, &code);
    napi_set_named_property(env, err, "kgsCode", code);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->op == 0) {
    napi_value u;
    napi_get_undefined(env, &u);
    napi_resolve_deferred(env, j->deferred, u);
  } else if (j->op == 2 || j->op == 5) {
    napi_resolve_deferred(env, j->deferred, adopt_u8(env, j->out, j->out_len));
    j->out = nullptr;
  } else if (j->op == 4 || j->op == 9) {
    napi_resolve_deferred(env, j->deferred, make_u8(env, j->msm_out, 64));
  } else if (j->op == 8) {
    napi_resolve_deferred(env, j->deferred, make_u8(env, j->bases.data(), j->bases.size()));
  } else if (j->op == 10 || j->op == 11 || j->op == 14) {
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "proofs", make_u8(env, j->bases.data(), j->bases.size()));
    napi_set_named_property(env, o, "evals", make_u8(env, j->ev.data(), j->ev.size()));
    napi_resolve_deferred(env, j->deferred, o);
  } else if (j->op == 13) {
    napi_value o, v;
    napi_create_object(env, &o);
    napi_get_boolean(env, j->rc_ok != 0, &v);
    napi_set_named_property(env, o, "ok", v);
    napi_set_named_property(env, o, "coefs", make_u8(env, j->scal.data(), j->scal.size()));
    napi_set_named_property(env, o, "evals", make_u8(env, j->ev.data(), j->ev.size()));
    napi_resolve_deferred(env, j->deferred, o);
  } else if (j->op == 15) {
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "status", make_u8(env, j->vb_valid.data(), j->many_polys));
    napi_set_named_property(env, o, "coefs", make_u8(env, j->scal.data(), j->scal.size()));
    napi_set_named_property(env, o, "evals", make_u8(env, j->ev.data(), j->ev.size()));
    napi_resolve_deferred(env, j->deferred, o);
  } else if (j->op == 12) {
    napi_value o, v;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "valid", make_u8(env, j->vb_valid.data(), j->cb_index.size()));
    napi_create_uint32(env, j->cb_diag.pairing_checks, &v);
    napi_set_named_property(env, o, "pairingChecks", v);
    napi_get_boolean(env, j->cb_diag.on_gpu != 0, &v);
    napi_set_named_property(env, o, "onGpu", v);
    napi_create_double(env, j->cb_diag.hash_ms, &v);
    napi_set_named_property(env, o, "hashMs", v);
    napi_create_double(env, j->cb_diag.fold_ms, &v);
    napi_set_named_property(env, o, "foldMs", v);
    napi_create_double(env, j->cb_diag.pairing_ms, &v);
    napi_set_named_property(env, o, "pairingMs", v);
    napi_resolve_deferred(env, j->deferred, o);
  } else if (j->op == 6) {
    napi_value o, v;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "valid", make_u8(env, j->vb_valid.data(), j->vb_refs.size()));
    napi_create_uint32(env, j->vb_diag.pairing_checks, &v);
    napi_set_named_property(env, o, "pairingChecks", v);
    napi_create_uint32(env, j->vb_diag.terms, &v);
    napi_set_named_property(env, o, "terms", v);
    napi_get_boolean(env, j->vb_diag.on_gpu != 0, &v);
    napi_set_named_property(env, o, "onGpu", v);
    napi_create_double(env, j->vb_diag.fold_ms, &v);
    napi_set_named_property(env, o, "foldMs", v);
    napi_create_double(env, j->vb_diag.pairing_ms, &v);
    napi_set_named_property(env, o, "pairingMs", v);
    napi_resolve_deferred(env, j->deferred, o);
  } else {
    napi_value o, arr;
    napi_create_object(env, &o);
    napi_create_array(env, &arr);
    for (size_t i = 0; i < j->com.size() / 64; i++) napi_set_element(env, arr, (uint32_t)i, make_u8(env, &j->com[64 * i], 64));
    napi_set_named_property(env, o, "commitments", arr);
    napi_create_array(env, &arr);
    for (size_t i = 0; i < j->ev.size() / 32; i++) napi_set_element(env, arr, (uint32_t)i, make_u8(env, &j->ev[32 * i], 32));
    napi_set_named_property(env, o, "evaluations", arr);
    napi_create_array(env, &arr);
    const size_t E = (size_t)32 << j->nbits;
    for (size_t i = 0; i < j->mf.size(); i++) napi_set_element(env, arr, (uint32_t)i, adopt_u8(env, j->mf[i], E));
    napi_set_named_property(env, o, "montF", arr);
    napi_create_array(env, &arr);
    for (size_t i = 0; i < j->mt.size(); i++) napi_set_element(env, arr, (uint32_t)i, adopt_u8(env, j->mt[i], E));
    napi_set_named_property(env, o, "montT", arr);
    napi_value ems;
    napi_create_double(env, j->exec_ms, &ems);
    napi_set_named_property(env, o, "execMs", ems);  // diagnostics: time inside libkgs
    // diagnostics: [queued -> worker start, worker end -> this completion callback] in ms
    const auto tc = std::chrono::steady_clock::now();
    napi_create_array(env, &arr);
    const double d0 = std::chrono::duration<double, std::milli>(j->t_exec0 - j->t_queue).count();
    const double d1 = std::chrono::duration<double, std::milli>(tc - j->t_exec1).count();
    napi_create_double(env, d0, &ems);
    napi_set_element(env, arr, 0, ems);
    napi_create_double(env, d1, &ems);
    napi_set_element(env, arr, 1, ems);
    napi_set_named_property(env, o, "waitMs", arr);
    j->mf.clear();
    j->mt.clear();
    napi_resolve_deferred(env, j->deferred, o);
  }
  const size_t Eo = (size_t)32 << j->nbits;
  for (uint8_t* p : j->mf)  // error path: not adopted
    if (p) out_release(p, Eo);
  for (uint8_t* p : j->mt)
    if (p) out_release(p, Eo);
  if (j->out) out_release(j->out, j->out_len);
  for (napi_ref r : j->refs) napi_delete_reference(env, r);
  napi_delete_async_work(env, j->work);
  delete j;
}

static napi_value queue(napi_env env, Job* j, const char* name) {
  napi_value promise, rname;
  NAPI_CALL(env, napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &rname);
  NAPI_CALL(env, napi_create_async_work(env, nullptr, rname, job_execute, job_complete, j, &j->work));
  j->t_queue = std::chrono::steady_clock::now();
  NAPI_CALL(env, napi_queue_async_work(env, j->work));
  if (j->op == 1 || j->op == 3) flush_external(env);  // a GC it starts now runs beside the proof just queued
  return promise;
}

// srsLoadPtau(ctx, path, nbitsMax) -> Promise<void>
static napi_value SrsLoad(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 0;
  j->ctx = get_ctx(env, argv[0]);
  size_t len;
  napi_get_value_string_utf8(env, argv[1], nullptr, 0, &len);
  j->path.resize(len + 1);
  napi_get_value_string_utf8(env, argv[1], &j->path[0], len + 1, &len);
  j->path.resize(len);
  if (argc > 2) napi_get_value_int32(env, argv[2], &j->nbits_max);
  return queue(env, j, "kgs_srs_load");
}

// prove(ctx, kind, nbits, [F...], [T...], selF|null, selT|null[, wantMont = true])
//   -> Promise<{commitments, evaluations, montF, montT}> (montF/montT empty without wantMont)
static napi_value prove_args(napi_env env, napi_value* argv, size_t argc, Job* j);
static napi_value Prove(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 1;
  j->ctx = get_ctx(env, argv[0]);
  return prove_args(env, argv, argc, j);
}

// proveGroup([ctx_0..ctx_{W-1}], ptauPath, kind, nbits, [F...], [T...], selF|null, selT|null)
//   -> Promise<{commitments, evaluations, montF, montT}>: one proof over the contexts' rank group
//   (ctxSetGroup(ctx_r, group, r) beforehand), each rank with its SRS slice, one thread per rank
static napi_value ProveGroup(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 3;
  uint32_t W = 0;
  napi_get_array_length(env, argv[0], &W);
  for (uint32_t r = 0; r < W; r++) {
    napi_value e;
    napi_get_element(env, argv[0], r, &e);
    j->ranks.push_back(get_ctx(env, e));
  }
  size_t len = 0;
  napi_get_value_string_utf8(env, argv[1], nullptr, 0, &len);
  j->path.resize(len + 1);
  napi_get_value_string_utf8(env, argv[1], &j->path[0], len + 1, &len);
  j->path.resize(len);
  if (W < 1) {
    delete j;
    napi_throw_error(env, nullptr, "proveGroup: no ranks");
    return nullptr;
  }
  // the prove(...) argument list from `kind` on: argv[2..7] -> positions 1..6 (argv[0] unused)
  napi_value pa[8];
  pa[0] = argv[0];
  for (int i = 2; i < 8; i++) pa[i - 1] = argv[i];
  return prove_args(env, pa, argc - 1, j);
}

static napi_value prove_args(napi_env env, napi_value* argv, size_t argc, Job* j) {
  napi_get_value_int32(env, argv[1], &j->kind);
  napi_get_value_int32(env, argv[2], &j->nbits);
  uint32_t nf = 0, nt = 0;
  napi_get_array_length(env, argv[3], &nf);
  napi_get_array_length(env, argv[4], &nt);
  j->npols = (int)nf;
  for (uint32_t i = 0; i < nf; i++) {
    napi_value e;
    napi_get_element(env, argv[3], i, &e);
    j->f.push_back(view_of(env, e, j->refs));
    napi_get_element(env, argv[4], i, &e);
    j->t.push_back(view_of(env, e, j->refs));
  }
  napi_valuetype ty;
  napi_typeof(env, argv[5], &ty);
  if (ty != napi_null && ty != napi_undefined) {
    j->selected = true;
    j->sf = view_of(env, argv[5], j->refs);
    j->st = view_of(env, argv[6], j->refs);
  }
  if (argc > 7) {
    napi_typeof(env, argv[7], &ty);
    if (ty == napi_boolean) napi_get_value_bool(env, argv[7], &j->want_mont);
  }
  return queue(env, j, j->op == 3 ? "kgs_prove_group" : "kgs_prove");
}

// proveMulti(ctx, nbits, [{kind, F: [..], T: [..], selF|null, selT|null}, ..])
//   -> Promise<{commitments, evaluations}> in the order of kgs_prove_multi (include/kgs.h); the inputs are
//   borrowed until the job completes and left as they are (no Montgomery write-back)
static napi_value ProveMulti(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 7;
  j->ctx = get_ctx(env, argv[0]);
  napi_get_value_int32(env, argv[1], &j->nbits);
  uint32_t m = 0;
  napi_get_array_length(env, argv[2], &m);
  bool ok = true;
  for (uint32_t a = 0; a < m; a++) {
    napi_value e, v, lf, lt;
    napi_get_element(env, argv[2], a, &e);
    Job::MultiArg ma;
    napi_get_named_property(env, e, "kind", &v);
    napi_get_value_int32(env, v, &ma.kind);
    napi_get_named_property(env, e, "F", &lf);
    napi_get_named_property(env, e, "T", &lt);
    uint32_t nf = 0, nt = 0;
    napi_get_array_length(env, lf, &nf);
    napi_get_array_length(env, lt, &nt);
    ok &= nf == nt;
    for (uint32_t i = 0; i < nf && nf == nt; i++) {
      napi_get_element(env, lf, i, &v);
      ma.f.push_back(view_of(env, v, j->refs));
      napi_get_element(env, lt, i, &v);
      ma.t.push_back(view_of(env, v, j->refs));
    }
    napi_value sf, st;
    napi_valuetype ty;
    napi_get_named_property(env, e, "selF", &sf);
    napi_get_named_property(env, e, "selT", &st);
    napi_typeof(env, sf, &ty);
    if (ty != napi_null && ty != napi_undefined) {
      ma.selected = true;
      ma.sf = view_of(env, sf, j->refs);
      ma.st = view_of(env, st, j->refs);
    }
    j->margs.push_back(ma);
  }
  if (!ok || j->nbits < 1 || j->nbits > 28) {
    for (napi_ref r : j->refs) napi_delete_reference(env, r);
    delete j;
    napi_throw_error(env, nullptr, "proveMulti: nbits in 1 .. 28 and, per argument, F and T lists of the same length");
    return nullptr;
  }
  return queue(env, j, "kgs_prove_multi");
}

// frOp(ctx, op, Uint8Array) -> Promise<Uint8Array> on ctx's GPU, elementwise over 32 B elements:
// op 0 = Fr.batchToMontgomery, 1 = Fr.batchFromMontgomery, 2 = Fr.batchInverse (0 -> 0),
// 3 = Fr.fft, 4 = Fr.ifft (2^k elements, natural order) — the curve shim's batch members
static napi_value FrOp(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 2;
  j->ctx = get_ctx(env, argv[0]);
  napi_get_value_int32(env, argv[1], &j->fr_op);
  j->in = view_of(env, argv[2], j->refs);
  const uint64_t n = j->in.len / 32;
  const bool pow2 = n && !(n & (n - 1));
  const char* bad = j->fr_op < 0 || j->fr_op > 4                  ? "frOp: unknown op"
                    : !n || j->in.len % 32                        ? "frOp: the buffer must hold 32-byte elements"
                    : j->fr_op >= 3 && (!pow2 || n > (1ull << 28)) ? "frOp: fft size must be a power of two <= 2^28"
                                                                   : nullptr;
  if (bad) {
    for (napi_ref r : j->refs) napi_delete_reference(env, r);
    delete j;
    napi_throw_error(env, nullptr, bad);
    return nullptr;
  }
  return queue(env, j, "kgs_fr_op");
}

// lookupMultiplicities(ctx, [F...], [T...], selF|null) -> Promise<Uint8Array>: the Montgomery
// multiplicities of the table rows (kgs_lookup_multiplicities). F / T: k standard-form buffers of the
// same number of 32 B elements, selF a Montgomery selector of that length; all borrowed (referenced,
// not copied) until the job completes, as the prover's inputs are.
static napi_value LookupMultiplicities(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 5;
  j->ctx = get_ctx(env, argv[0]);
  uint32_t nf = 0, nt = 0;
  napi_get_array_length(env, argv[1], &nf);
  napi_get_array_length(env, argv[2], &nt);
  j->npols = (int)nf;
  for (uint32_t i = 0; i < nf && nf == nt; i++) {
    napi_value e;
    napi_get_element(env, argv[1], i, &e);
    j->f.push_back(view_of(env, e, j->refs));
    napi_get_element(env, argv[2], i, &e);
    j->t.push_back(view_of(env, e, j->refs));
  }
  if (argc > 3) {
    napi_valuetype ty;
    napi_typeof(env, argv[3], &ty);
    if (ty != napi_null && ty != napi_undefined) {
      j->selected = true;
      j->sf = view_of(env, argv[3], j->refs);
    }
  }
  bool ok = nf >= 1 && nf == nt;
  const size_t E = ok ? j->f[0].len : 0;
  ok = ok && E >= 32 && E % 32 == 0;
  for (uint32_t i = 0; ok && i < nf; i++) ok = j->f[i].p && j->t[i].p && j->f[i].len == E && j->t[i].len == E;
  if (ok && j->selected) ok = j->sf.p && j->sf.len == E;
  if (!ok) {
    for (napi_ref r : j->refs) napi_delete_reference(env, r);
    delete j;
    napi_throw_error(env, nullptr,
                     "lookupMultiplicities: F and T must be two lists of the same number of buffers, each (and "
                     "selF) holding the same number (>= 1) of 32-byte elements");
    return nullptr;
  }
  return queue(env, j, "kgs_lookup_multiplicities");
}

// verifyBatch(ctx, ptauPath, [{kind, nbits, npols, selected, commitments(Uint8Array), evaluations(Uint8Array)}, ..])
// -> Promise<{valid: Uint8Array (1 / 0 per proof), pairingChecks, terms, onGpu, foldMs, pairingMs}>
// (kgs_verify_batch_ptau: one pairing check for the batch, the G1 fold on the context's GPU). The
// proofs' bytes are copied: the call returns before the work runs.
static napi_value VerifyBatch(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 6;
  j->ctx = get_ctx(env, argv[0]);
  size_t plen = 0;
  napi_get_value_string_utf8(env, argv[1], nullptr, 0, &plen);
  j->path.assign(plen + 1, '\0');
  napi_get_value_string_utf8(env, argv[1], &j->path[0], plen + 1, &plen);
  j->path.resize(plen);
  uint32_t n = 0;
  napi_get_array_length(env, argv[2], &n);
  bool ok = true;
  j->vb_bytes.reserve(2 * (size_t)n);
  for (uint32_t i = 0; i < n && ok; i++) {
    napi_value e, v;
    napi_get_element(env, argv[2], i, &e);
    int32_t kind = 0, nbits = 0, npols = 0;
    bool selected = false;
    napi_get_named_property(env, e, "kind", &v);
    napi_get_value_int32(env, v, &kind);
    napi_get_named_property(env, e, "nbits", &v);
    napi_get_value_int32(env, v, &nbits);
    napi_get_named_property(env, e, "npols", &v);
    napi_get_value_int32(env, v, &npols);
    napi_get_named_property(env, e, "selected", &v);
    napi_get_value_bool(env, v, &selected);
    napi_get_named_property(env, e, "commitments", &v);
    j->vb_bytes.push_back(bytes_of(env, v));
    napi_get_named_property(env, e, "evaluations", &v);
    j->vb_bytes.push_back(bytes_of(env, v));
    int nc = 0, ne = 0;
    ok = kgs_proof_shape(kind, npols, selected ? 1 : 0, &nc, &ne) == KGS_OK &&
         j->vb_bytes[2 * i].size() == (size_t)nc * 64 && j->vb_bytes[2 * i + 1].size() == (size_t)ne * 32;
    j->vb_refs.push_back(kgs_proof_ref_t{kind, nbits, npols, selected ? 1 : 0, j->vb_bytes[2 * i].data(),
                                         j->vb_bytes[2 * i + 1].data()});
  }
  if (!ok) {
    delete j;
    napi_throw_error(env, nullptr, "verifyBatch: proof buffers do not match the proof shape");
    return nullptr;
  }
  return queue(env, j, "kgs_verify_batch");
}

// verifyPtau(kind, ptauPath, nbits, npols, selected, commitments(Uint8Array), evaluations(Uint8Array))
// -> boolean (host-only pairing check, kgs_verify_ptau)
static napi_value VerifyPtau(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t kind = 0, nbits = 0, npols = 0;
  bool selected = false;
  napi_get_value_int32(env, argv[0], &kind);
  size_t plen = 0;
  napi_get_value_string_utf8(env, argv[1], nullptr, 0, &plen);
  std::string path(plen + 1, '\0');
  napi_get_value_string_utf8(env, argv[1], &path[0], plen + 1, &plen);
  path.resize(plen);
  napi_get_value_int32(env, argv[2], &nbits);
  napi_get_value_int32(env, argv[3], &npols);
  napi_get_value_bool(env, argv[4], &selected);
  std::vector<uint8_t> com = bytes_of(env, argv[5]), ev = bytes_of(env, argv[6]);
  int nc = 0, ne = 0;
  kgs_proof_shape(kind, npols, selected ? 1 : 0, &nc, &ne);
  if (com.size() != (size_t)nc * 64 || ev.size() != (size_t)ne * 32) {
    napi_throw_error(env, nullptr, "proof buffers do not match the proof shape");
    return nullptr;
  }
  int rc = kgs_verify_ptau(kind, path.c_str(), nbits, npols, selected ? 1 : 0, com.data(), ev.data());
  if (rc < 0) {
    napi_throw_error(env, nullptr, "kgs_verify_ptau failed");
    return nullptr;
  }
  napi_value out;
  napi_get_boolean(env, rc == 1, &out);
  return out;
}

// verifyMultiPtau(ptauPath, nbits, [{kind, npols, selected}, ..], commitments(Uint8Array), evaluations(Uint8Array))
// -> boolean (host-only pairing check of a multi-argument proof, kgs_verify_multi_ptau)
static napi_value VerifyMultiPtau(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  size_t plen = 0;
  napi_get_value_string_utf8(env, argv[0], nullptr, 0, &plen);
  std::string path(plen + 1, '\0');
  napi_get_value_string_utf8(env, argv[0], &path[0], plen + 1, &plen);
  path.resize(plen);
  int32_t nbits = 0;
  napi_get_value_int32(env, argv[1], &nbits);
  uint32_t m = 0;
  napi_get_array_length(env, argv[2], &m);
  std::vector<kgs_arg_shape_t> shapes(m);
  for (uint32_t a = 0; a < m; a++) {
    napi_value e, v;
    bool selected = false;
    napi_get_element(env, argv[2], a, &e);
    napi_get_named_property(env, e, "kind", &v);
    napi_get_value_int32(env, v, &shapes[a].kind);
    napi_get_named_property(env, e, "npols", &v);
    napi_get_value_int32(env, v, &shapes[a].npols);
    napi_get_named_property(env, e, "selected", &v);
    napi_get_value_bool(env, v, &selected);
    shapes[a].selected = selected ? 1 : 0;
  }
  std::vector<uint8_t> com = bytes_of(env, argv[3]), ev = bytes_of(env, argv[4]);
  int nc = 0, ne = 0;
  if (kgs_multi_proof_shape(shapes.data(), (int)m, &nc, &ne) != KGS_OK || com.size() != (size_t)nc * 64 ||
      ev.size() != (size_t)ne * 32) {
    napi_throw_error(env, nullptr, "proof buffers do not match the arguments' shapes");
    return nullptr;
  }
  int rc = kgs_verify_multi_ptau(path.c_str(), nbits, shapes.data(), (int)m, com.data(), ev.data());
  if (rc < 0) {
    napi_throw_error(env, nullptr, "kgs_verify_multi_ptau failed");
    return nullptr;
  }
  napi_value out;
  napi_get_boolean(env, rc == 1, &out);
  return out;
}

// groupCreateLocal(world) -> rank group of `world` contexts in this process (kgs_group_create_local):
// the distributed prover with every vector sharded, driven from one Node process (one libuv
// thread per rank). ctxSetGroup(ctx, group|null, rank) attaches / detaches a context.
static void group_finalize(napi_env, void* data, void*) { kgs_group_destroy((kgs_group_t*)data); }
static napi_value GroupCreateLocal(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t world = 1;
  if (argc > 0) napi_get_value_int32(env, argv[0], &world);
  kgs_group_t* g = nullptr;
  if (kgs_group_create_local(world, &g) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  napi_value ext;
  NAPI_CALL(env, napi_create_external(env, g, group_finalize, nullptr, &ext));
  return ext;
}
static napi_value CtxSetGroup(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  kgs_ctx_t* ctx = get_ctx(env, argv[0]);
  napi_valuetype ty;
  napi_typeof(env, argv[1], &ty);
  void* g = nullptr;
  if (ty == napi_external) napi_get_value_external(env, argv[1], &g);
  int32_t rank = 0;
  if (argc > 2) napi_get_value_int32(env, argv[2], &rank);
  if (kgs_ctx_set_group(ctx, (kgs_group_t*)g, rank) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  return nullptr;
}

// ctxSetMsmLanes(ctx, lanes): 2 = the single-proof latency mode, 1 = throughput (several proofs in
// flight on the device) — kgs_ctx_set_msm_lanes; call while the context is idle
static napi_value CtxSetMsmLanes(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  kgs_ctx_t* ctx = get_ctx(env, argv[0]);
  int32_t lanes = 2;
  napi_get_value_int32(env, argv[1], &lanes);
  if (kgs_ctx_set_msm_lanes(ctx, lanes) != KGS_OK) {
    napi_throw_error(env, nullptr, kgs_last_error());
    return nullptr;
  }
  return nullptr;
}

// pairingEq(g1s, g2s): g1s = n x 64 B affine LEM G1, g2s = n x 128 B affine LEM G2 -> bool
// (curve.pairingEq, src/grandsum/mset_eq_kzg_verifier.js:182)
static napi_value PairingEq(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::vector<uint8_t> a = bytes_of(env, argv[0]), b = bytes_of(env, argv[1]);
  if (a.size() % 64 || b.size() % 128 || a.size() / 64 != b.size() / 128) {
    napi_throw_error(env, nullptr, "pairingEq: expected n x 64 B G1 and n x 128 B G2 affine points");
    return nullptr;
  }
  const int rc = kgs_pairing_eq((int)(a.size() / 64), a.data(), b.data());
  if (rc < 0) {
    napi_throw_error(env, nullptr, "pairingEq: point not on the curve");
    return nullptr;
  }
  napi_value out;
  napi_get_boolean(env, rc == 1, &out);
  return out;
}

// msmPoints(ctx, bases, scalarsStd) -> Promise<64 B affine LEM sum_i s_i P_i> on the GPU of ctx (the
// curve shim's G1.multiExpAffine, polynomial.js:1112, whose scalars are standard-form LE after
// Fr.batchFromMontgomery): kgs_msm_points reads the bases as given, builds no window tables and leaves
// ctx's SRS alone. Async work like every other heavy call.
static napi_value MsmPoints(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 4;
  j->ctx = get_ctx(env, argv[0]);
  j->bases = bytes_of(env, argv[1]);
  j->scal = bytes_of(env, argv[2]);
  const uint64_t n = j->scal.size() / 32;
  if (j->scal.size() % 32 || j->bases.size() != 64 * n || n < 1) {
    delete j;
    napi_throw_error(env, nullptr, "msmPoints: expected n >= 1 affine LEM bases and n 32 B scalars");
    return nullptr;
  }
  return queue(env, j, "kgs_msm_points");
}

// 2^k elements of `size` bytes -> k, or -1
static int log2_count(size_t bytes, size_t size) {
  if (bytes == 0 || bytes % size) return -1;
  const size_t n = bytes / size;
  if (n & (n - 1)) return -1;
  int k = 0;
  while (((size_t)1 << k) < n) k++;
  return k;
}

// g1Ntt(ctx, pointsLem, inverse) -> Promise<2^k x 64 B affine LEM> on the GPU of ctx (the curve shim's
// G1.fft / G1.ifft): kgs_g1_ntt over a copy of the points; ctx's SRS is left alone.
static napi_value G1Ntt(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 8;
  j->ctx = get_ctx(env, argv[0]);
  j->bases = bytes_of(env, argv[1]);
  bool inv = false;
  napi_get_value_bool(env, argv[2], &inv);
  j->ntt_inverse = inv ? 1 : 0;
  j->ntt_logm = log2_count(j->bases.size(), 64);
  if (j->ntt_logm < 0) {
    delete j;
    napi_throw_error(env, nullptr, "g1Ntt: expected a power of two of 64 B affine LEM points");
    return nullptr;
  }
  return queue(env, j, "kgs_g1_ntt");
}

// commitEvals(ctx, evalsStd) -> Promise<64 B affine LEM> over the SRS resident on ctx (kgs_commit_evals):
// the commitment to the polynomial with these 2^k standard-form evaluations
static napi_value CommitEvals(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 9;
  j->ctx = get_ctx(env, argv[0]);
  j->scal = bytes_of(env, argv[1]);
  j->ntt_logm = log2_count(j->scal.size(), 32);
  if (j->ntt_logm < 0) {
    delete j;
    napi_throw_error(env, nullptr, "commitEvals: expected a power of two of 32 B standard-form evaluations");
    return nullptr;
  }
  return queue(env, j, "kgs_commit_evals");
}

// kzgOpenAll(ctx, coefMont) -> Promise<{proofs, evals}> over the SRS resident on ctx (kgs_kzg_open_all): the
// openings of the polynomial with these Montgomery coefficients at every point of the smallest domain
// 2^k that holds them, 2^k x 64 B affine LEM, and its values there, 2^k x 32 B Montgomery
static napi_value KzgOpenAll(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 10;
  j->ctx = get_ctx(env, argv[0]);
  j->scal = bytes_of(env, argv[1]);
  const size_t n = j->scal.size() / 32;
  if (j->scal.size() % 32 || n > ((size_t)1 << 23)) {
    delete j;
    napi_throw_error(env, nullptr, "kzgOpenAll: expected at most 2^23 Montgomery coefficients of 32 B");
    return nullptr;
  }
  j->ntt_logm = 0;
  while (((size_t)1 << j->ntt_logm) < n) j->ntt_logm++;
  return queue(env, j, "kgs_kzg_open_all");
}

// kzgOpenCosets(ctx, coefMont, nBits, lBits) -> Promise<{proofs, evals}> over the SRS resident on ctx
// (kgs_kzg_open_cosets): one proof per coset of 2^lBits points of the domain of 2^nBits, 2^(nBits - lBits) x
// 64 B affine LEM, and the polynomial's values on the domain, 2^nBits x 32 B Montgomery
static napi_value KzgOpenCosets(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t nbits = -1, lbits = -1;
  Job* j = new Job();
  j->op = 11;
  j->ctx = get_ctx(env, argv[0]);
  j->scal = bytes_of(env, argv[1]);
  napi_get_value_int32(env, argv[2], &nbits);
  napi_get_value_int32(env, argv[3], &lbits);
  if (j->scal.size() % 32 || nbits < 0 || nbits > 23 || lbits < 0 || lbits > nbits ||
      j->scal.size() / 32 > ((size_t)1 << nbits)) {
    delete j;
    napi_throw_error(env, nullptr, "kzgOpenCosets: expected at most 2^nBits Montgomery coefficients of 32 B, nBits <= 23, lBits <= nBits");
    return nullptr;
  }
  j->ntt_logm = nbits;
  j->ntt_inverse = lbits;
  return queue(env, j, "kgs_kzg_open_cosets");
}

// kzgOpenCosetsMany(ctx, coefMont, polys, nBits, lBits) -> Promise<{proofs, evals}> over the SRS resident on ctx
// (kgs_kzg_open_cosets_many): kzgOpenCosets for `polys` polynomials of equal length packed one after the other, in
// one call; proofs polys x 2^(nBits - lBits) x 64 B, evals polys x 2^nBits x 32 B, polynomial after polynomial
static napi_value KzgOpenCosetsMany(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t nbits = -1, lbits = -1;
  int64_t polys = -1;
  Job* j = new Job();
  j->op = 14;
  j->ctx = get_ctx(env, argv[0]);
  j->scal = bytes_of(env, argv[1]);
  napi_get_value_int64(env, argv[2], &polys);
  napi_get_value_int32(env, argv[3], &nbits);
  napi_get_value_int32(env, argv[4], &lbits);
  const bool sizes = nbits >= 0 && nbits <= 23 && lbits >= 0 && lbits <= nbits && polys >= 0 &&
                     (uint64_t)polys <= ((uint64_t)1 << (24 - nbits));
  if (!sizes || j->scal.size() % 32 || (polys == 0 ? j->scal.size() != 0 : j->scal.size() / 32 % (size_t)polys != 0) ||
      (polys && j->scal.size() / 32 / (size_t)polys > ((size_t)1 << nbits))) {
    delete j;
    napi_throw_error(env, nullptr, "kzgOpenCosetsMany: expected polys x at most 2^nBits Montgomery coefficients of 32 B, "
                                   "nBits <= 23, lBits <= nBits, polys * 2^nBits <= 2^24");
    return nullptr;
  }
  j->many_polys = (uint64_t)polys;
  j->ntt_logm = nbits;
  j->ntt_inverse = lbits;
  return queue(env, j, "kgs_kzg_open_cosets_many");
}

// kzgVerifyCoset(commit, nBits, lBits, index, ysMont, proof, srsG1, tauLG2) -> bool (kgs_kzg_verify_coset, host
// only): the check of one coset opening; srsG1 = the first 2^lBits points [tau^k]_1, tauLG2 = [tau^l]_2
static napi_value KzgVerifyCoset(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t nbits = -1, lbits = -1;
  int64_t index = -1;
  std::vector<uint8_t> cm = bytes_of(env, argv[0]), ys = bytes_of(env, argv[4]), pf = bytes_of(env, argv[5]),
                       srs = bytes_of(env, argv[6]), t2 = bytes_of(env, argv[7]);
  napi_get_value_int32(env, argv[1], &nbits);
  napi_get_value_int32(env, argv[2], &lbits);
  napi_get_value_int64(env, argv[3], &index);
  if (nbits < 0 || nbits > 28 || lbits < 0 || lbits > nbits || index < 0 || cm.size() != 64 || pf.size() != 64 ||
      t2.size() != 128 || ys.size() != ((size_t)32 << lbits) || srs.size() < ((size_t)64 << lbits)) {
    napi_throw_error(env, nullptr, "kzgVerifyCoset: expected 64 B commit and proof, 2^lBits x 32 B values, at least 2^lBits x 64 B SRS points, 128 B [tau^l]_2");
    return nullptr;
  }
  const int rc = kgs_kzg_verify_coset(cm.data(), nbits, lbits, (uint64_t)index, ys.data(), pf.data(), srs.data(), t2.data());
  if (rc < 0) {
    napi_throw_error(env, nullptr, "kzgVerifyCoset: index out of range or [tau^l]_2 not on its curve");
    return nullptr;
  }
  napi_value out;
  napi_get_boolean(env, rc == 1, &out);
  return out;
}

// kzgVerifyCosetsBatch(ctx | null, nBits, lBits, commits, commitOf, index, ysMont, proofs, srsG1, tauLG2, seed | null)
//   -> Promise<{valid, pairingChecks, onGpu, hashMs, foldMs, pairingMs}> (kgs_kzg_verify_cosets_batch): commits the
// concatenated 64 B commitments, commitOf / index arrays of count numbers, ysMont count * 2^lBits x 32 B, proofs
// count x 64 B, srsG1 at least 2^lBits x 64 B, tauLG2 128 B, seed 32 B or null; ctx null: on the host
static napi_value KzgVerifyCosetsBatch(napi_env env, napi_callback_info info) {
  size_t argc = 11;
  napi_value argv[11];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 12;
  napi_valuetype vt = napi_null;
  napi_typeof(env, argv[0], &vt);
  j->ctx = vt == napi_null || vt == napi_undefined ? nullptr : get_ctx(env, argv[0]);
  int32_t nbits = -1, lbits = -1;
  napi_get_value_int32(env, argv[1], &nbits);
  napi_get_value_int32(env, argv[2], &lbits);
  j->nbits = nbits;
  j->ntt_inverse = lbits;
  j->com = bytes_of(env, argv[3]);
  uint32_t nc = 0, ni = 0;
  napi_get_array_length(env, argv[4], &nc);
  napi_get_array_length(env, argv[5], &ni);
  bool ok = nc == ni && nbits >= 0 && nbits <= 28 && lbits >= 0 && lbits <= nbits;
  for (uint32_t k = 0; ok && k < nc; k++) {
    napi_value v;
    int64_t c = -1, i = -1;
    napi_get_element(env, argv[4], k, &v);
    napi_get_value_int64(env, v, &c);
    napi_get_element(env, argv[5], k, &v);
    napi_get_value_int64(env, v, &i);
    ok = c >= 0 && c <= 0xffffffffll && i >= 0;
    j->cb_commit_of.push_back((uint32_t)c);
    j->cb_index.push_back((uint64_t)i);
  }
  j->cb_ys = bytes_of(env, argv[6]);
  j->cb_proofs = bytes_of(env, argv[7]);
  j->bases = bytes_of(env, argv[8]);
  j->scal = bytes_of(env, argv[9]);
  napi_typeof(env, argv[10], &vt);
  if (argc > 10 && vt != napi_null && vt != napi_undefined) j->cb_seed = bytes_of(env, argv[10]);
  if (!ok || j->com.size() % 64 || j->cb_proofs.size() != (size_t)64 * nc ||
      j->cb_ys.size() != ((size_t)32 * nc << lbits) || j->bases.size() < ((size_t)64 << lbits) || j->scal.size() != 128 ||
      (!j->cb_seed.empty() && j->cb_seed.size() != 32)) {
    delete j;
    napi_throw_error(env, nullptr, "kzgVerifyCosetsBatch: expected 64 B commitments, count commit indices and coset indices, count * 2^lBits x 32 B values, count x 64 B proofs, at least 2^lBits x 64 B SRS points, 128 B [tau^l]_2, a 32 B seed or null");
    return nullptr;
  }
  // the library takes NULL for an empty buffer; a vector's data() may be anything then
  j->com.reserve(1);
  j->cb_commit_of.reserve(1);
  j->cb_index.reserve(1);
  j->cb_ys.reserve(1);
  j->cb_proofs.reserve(1);
  return queue(env, j, "kgs_kzg_verify_cosets_batch");
}

// kzgRecoverCosets(ctx, nBits, lBits, index, ysMont, length) -> Promise<{ok, coefs, evals}> (kgs_kzg_recover_cosets):
// index an array of count distinct coset indices, ysMont count * 2^lBits x 32 B Montgomery values (row k = the values
// on coset index[k]), length the number of coefficients (count * 2^lBits >= length); coefs length x 32 B, evals
// 2^nBits x 32 B, both meaningless when ok is false
static napi_value KzgRecoverCosets(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 13;
  j->ctx = get_ctx(env, argv[0]);
  int32_t nbits = -1, lbits = -1;
  int64_t len = -1;
  napi_get_value_int32(env, argv[1], &nbits);
  napi_get_value_int32(env, argv[2], &lbits);
  uint32_t ni = 0;
  napi_get_array_length(env, argv[3], &ni);
  bool ok = nbits >= 0 && nbits <= 23 && lbits >= 0 && lbits <= nbits;
  for (uint32_t k = 0; ok && k < ni; k++) {
    napi_value v;
    int64_t i = -1;
    napi_get_element(env, argv[3], k, &v);
    napi_get_value_int64(env, v, &i);
    ok = i >= 0;
    j->cb_index.push_back((uint64_t)i);
  }
  j->cb_ys = bytes_of(env, argv[4]);
  napi_get_value_int64(env, argv[5], &len);
  if (!ok || ni < 1 || len < 1 || len > ((int64_t)1 << nbits) || j->cb_ys.size() != ((size_t)32 * ni << lbits)) {
    delete j;
    napi_throw_error(env, nullptr, "kzgRecoverCosets: expected nBits <= 23, lBits <= nBits, count >= 1 coset indices, count * 2^lBits x 32 B values, 1 <= length <= 2^nBits");
    return nullptr;
  }
  j->ntt_logm = nbits;
  j->ntt_inverse = lbits;
  j->rc_len = (uint64_t)len;
  return queue(env, j, "kgs_kzg_recover_cosets");
}

// kzgRecoverCosetsMany(ctx, nBits, lBits, polyOf, index, ysMont, length, polys) -> Promise<{status, coefs, evals}>
// (kgs_kzg_recover_cosets_many): cell k belongs to polynomial polyOf[k] < polys and names coset index[k]; ysMont count *
// 2^lBits x 32 B Montgomery values; status polys bytes (1 recovered, 0 no such polynomial, 2 too few cells), coefs
// polys x length x 32 B, evals polys x 2^nBits x 32 B
static napi_value KzgRecoverCosetsMany(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Job* j = new Job();
  j->op = 15;
  j->ctx = get_ctx(env, argv[0]);
  int32_t nbits = -1, lbits = -1;
  int64_t len = -1, polys = -1;
  napi_get_value_int32(env, argv[1], &nbits);
  napi_get_value_int32(env, argv[2], &lbits);
  uint32_t np = 0, ni = 0;
  napi_get_array_length(env, argv[3], &np);
  napi_get_array_length(env, argv[4], &ni);
  bool ok = nbits >= 0 && nbits <= 23 && lbits >= 0 && lbits <= nbits && np == ni;
  for (uint32_t k = 0; ok && k < ni; k++) {
    napi_value v;
    int64_t b = -1, i = -1;
    napi_get_element(env, argv[3], k, &v);
    napi_get_value_int64(env, v, &b);
    napi_get_element(env, argv[4], k, &v);
    napi_get_value_int64(env, v, &i);
    ok = b >= 0 && b <= 0xFFFFFFFFll && i >= 0;
    j->cb_commit_of.push_back((uint32_t)b);
    j->cb_index.push_back((uint64_t)i);
  }
  j->cb_ys = bytes_of(env, argv[5]);
  napi_get_value_int64(env, argv[6], &len);
  napi_get_value_int64(env, argv[7], &polys);
  if (!ok || len < 1 || len > ((int64_t)1 << nbits) || polys < 0 || polys > ((int64_t)1 << 24 >> nbits) ||
      j->cb_ys.size() != ((size_t)32 * ni << lbits)) {
    delete j;
    napi_throw_error(env, nullptr, "kzgRecoverCosetsMany: expected nBits <= 23, lBits <= nBits, one polynomial number and one coset index per cell, count * 2^lBits x 32 B values, 1 <= length <= 2^nBits, polys * 2^nBits <= 2^24");
    return nullptr;
  }
  j->ntt_logm = nbits;
  j->ntt_inverse = lbits;
  j->rc_len = (uint64_t)len;
  j->many_polys = (uint64_t)polys;
  // the library takes NULL for an empty buffer; a vector's data() may be anything then
  j->cb_commit_of.reserve(1);
  j->cb_index.reserve(1);
  j->cb_ys.reserve(1);
  return queue(env, j, "kgs_kzg_recover_cosets_many");
}

// lastTiming(ctx) -> [round 1..5 ms, -, input copy, prover, write-back wait] of the context's last
// kgs_prove call (kgs_last_timing; diagnostics, call when the context is idle)
static napi_value LastTiming(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  kgs_ctx_t* ctx = get_ctx(env, argv[0]);
  double t[9] = {0};
  const int n = kgs_last_timing(ctx, t, 9);
  napi_value arr;
  napi_create_array(env, &arr);
  for (int i = 0; i < n; i++) {
    napi_value v;
    napi_create_double(env, t[i], &v);
    napi_set_element(env, arr, (uint32_t)i, v);
  }
  return arr;
}

static napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor desc[] = {
      {"ctxCreate", nullptr, CtxCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"srsLoadPtau", nullptr, SrsLoad, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"srsInfo", nullptr, SrsInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"prove", nullptr, Prove, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"keccak256", nullptr, Keccak, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verifyPtau", nullptr, VerifyPtau, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ptauPower", nullptr, PtauPower, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"pairingEq", nullptr, PairingEq, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"groupCreateLocal", nullptr, GroupCreateLocal, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ctxSetGroup", nullptr, CtxSetGroup, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"msmPoints", nullptr, MsmPoints, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"g1Ntt", nullptr, G1Ntt, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"commitEvals", nullptr, CommitEvals, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgOpenAll", nullptr, KzgOpenAll, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgOpenCosets", nullptr, KzgOpenCosets, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgOpenCosetsMany", nullptr, KzgOpenCosetsMany, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgVerifyCoset", nullptr, KzgVerifyCoset, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgVerifyCosetsBatch", nullptr, KzgVerifyCosetsBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgRecoverCosets", nullptr, KzgRecoverCosets, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgRecoverCosetsMany", nullptr, KzgRecoverCosetsMany, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"proveGroup", nullptr, ProveGroup, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"lastTiming", nullptr, LastTiming, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ctxSetMsmLanes", nullptr, CtxSetMsmLanes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"frOp", nullptr, FrOp, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"lookupMultiplicities", nullptr, LookupMultiplicities, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verifyBatch", nullptr, VerifyBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"proveMulti", nullptr, ProveMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verifyMultiPtau", nullptr, VerifyMultiPtau, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(desc) / sizeof(desc[0]), desc);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
