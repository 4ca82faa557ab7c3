// The layout engine of the distributed prover (prover_dist.cpp): one rank's view of vectors sharded over
// W ranks as BLOCK (rank r holds indices [r M, (r + 1) M)), CYCLIC (r, r + W, ...) or E (the evaluation
// layout between the two halves of a distributed NTT), the exchange steps that move a vector between them,
// the per-rank tables, and the accounting of every exchange (kgs_last_exchange). The layouts and the
// exchange steps are specified, and checked on a CPU, by tests/test_dist_layouts.py; dist.hip holds the
// rank-local kernels.
#pragma once
#include "context.hpp"

namespace kgsi {

inline int ilog2(uint64_t x) {
  int l = 0;
  while ((1ull << l) < x) l++;
  return l;
}

struct Dist {
  kgs_ctx& c;
  kgs_group& g;
  const int W, r, logW;
  Dist(kgs_ctx& cc) : c(cc), g(*cc.group), W(cc.group->world), r(cc.group_rank), logW(ilog2(cc.group->world)) {}

  // how many of the coefficients [0, N) lie in this rank's CYCLIC slice (r, r + W, ...)
  uint64_t cyc_count(uint64_t N) const { return N > (uint64_t)r ? (N - r + W - 1) / W : 0; }

  // every exchange is counted in c.xs (kgs_last_exchange): all-to-alls by two events on the stream,
  // host all-gathers by the wall clock; bytes leaving this rank
  void a2a(const uint32_t* send, uint32_t* recv, uint64_t chunk_elems) {
    ExchangeStats& x = c.xs;
    if ((int)x.ev.size() <= x.a2a_n) {
      hipEvent_t e0, e1;
      HC(hipEventCreate(&e0));
      HC(hipEventCreate(&e1));
      x.ev.push_back({e0, e1});
    }
    const auto& ev = x.ev[x.a2a_n++];
    HC(hipEventRecord(ev.first, c.st));
    g.alltoall(r, c, c.st, send, recv, (size_t)32 * chunk_elems);
    HC(hipEventRecord(ev.second, c.st));
    x.a2a_bytes += g.alltoall_wire_bytes((size_t)32 * chunk_elems);  // what the transport moved
  }
  void allgather(const void* s, void* rv, size_t b) {
    const auto t0 = std::chrono::steady_clock::now();
    g.allgather(r, s, rv, b);
    c.xs.ag_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c.xs.ag_n++;
    c.xs.ag_bytes += (uint64_t)b * (W - 1);
  }
  // after the proof's last sync: the all-to-all spans from their events
  void finish_stats() {
    ExchangeStats& x = c.xs;
    x.a2a_ms = 0;
    for (int i = 0; i < x.a2a_n; i++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, x.ev[i].first, x.ev[i].second) == hipSuccess) x.a2a_ms += ms;
      else (void)hipGetLastError();
    }
  }
  // a per-rank device table, built once per shape and remembered in c.dist_tabs under `key` (also its
  // pool buffer's name); build(t) enqueues the kernels that fill it on the main stream
  template <class Build>
  uint32_t* cached_table(const std::string& key, size_t bytes, Build build) {
    auto it = c.dist_tabs.find(key);
    if (it != c.dist_tabs.end()) return it->second;
    uint32_t* t = c.buf(key, bytes);
    build(t);
    check_launch();
    c.dist_tabs[key] = t;
    return t;
  }
  // per-rank coset tables g^(+-(r + W i)), i < Ml, cached by (sign, logMl)
  uint32_t* coset_tab(int logMl, bool inverse) {
    const std::string key = std::string(inverse ? "d_cinv_" : "d_cfwd_") + std::to_string(logMl) + "_" +
                            std::to_string(W) + "_" + std::to_string(r);
    const uint64_t Ml = 1ull << logMl;
    return cached_table(key, 32 * Ml, [&](uint32_t* t) {
      Fr g5 = Fr::from_u64(KGS_NTT_COSET_GEN);
      if (inverse) g5 = g5.inverse();
      Fr k[2] = {g5.pow_u64((uint64_t)W), g5.pow_u64((uint64_t)r)};
      uint32_t* d = c.scal(k, 2);
      launch_powers(c.st, t, Ml, d, d + 8);
    });
  }
  // E (natural inside blocks) -> CYCLIC, scaled by 1/N and, for a coset, by g^-(global index)
  void inv_e_to_cyc(uint32_t* out, const uint32_t* inE, int logN, bool coset) {
    const int logMl = logN - logW;
    const uint64_t Ml = 1ull << logMl;
    uint32_t* send = c.buf("d_send", 32 * Ml);
    uint32_t* recv = c.buf("d_recv", 32 * Ml);
    launch_dinv_wdft_pack(c.st, send, inE, logMl, W, r, c.tw_inv, logN);
    check_launch();
    a2a(send, recv, Ml / W);
    ntt_dit(c.st, out, recv, 0, logMl, c.tw_inv, c.logM, coset ? coset_tab(logMl, true) : nullptr, c.invm + 8 * logN);
    check_launch();
  }
  // CYCLIC (in_len local coefficients, zero beyond) -> E evaluations (coset: g^(global index) first)
  void fwd_cyc_to_e(uint32_t* outE, const uint32_t* inC, uint64_t in_len, int logN, bool coset) {
    const int logMl = logN - logW;
    const uint64_t Ml = 1ull << logMl;
    uint32_t* Z = c.buf("d_Z", 32 * Ml);
    uint32_t* send = c.buf("d_send", 32 * Ml);
    uint32_t* recv = c.buf("d_recv", 32 * Ml);
    ntt_dif(c.st, Z, inC, in_len, logMl, coset ? coset_tab(logMl, false) : nullptr, c.tw_fwd, c.logM);
    launch_dfwd_pack(c.st, send, Z, logMl, W, r, c.tw_fwd, logN);
    check_launch();
    a2a(send, recv, Ml / W);
    launch_dfwd_wdft(c.st, outE, recv, logMl, W, c.tw_fwd, logN);
    check_launch();
  }
  void block_to_e(uint32_t* outE, const uint32_t* inB, uint64_t Ml) { a2a(inB, outE, Ml / W); }
  // BLOCK -> CYCLIC (the inverse of cyc_to_block): send chunk d = the block's indices = d mod W; the
  // received chunks, in source-rank order, are the cyclic slice in natural order
  void block_to_cyc(uint32_t* outC, const uint32_t* inB, uint64_t Lb) {
    uint32_t* send = c.buf("d_send", 32 * Lb);
    launch_pack_b2c(c.st, send, inB, Lb, W);
    check_launch();
    a2a(send, outC, Lb / W);
  }
  void cyc_to_block(uint32_t* outB, const uint32_t* inC, uint64_t Lb) {
    uint32_t* recv = c.buf("d_recv", 32 * Lb);
    a2a(inC, recv, Lb / W);
    launch_unpack_c2b(c.st, outB, recv, Lb, W);
    check_launch();
  }
  std::vector<Fr> gather_fr(const std::vector<Fr>& mine) {
    std::vector<uint8_t> s(32 * mine.size()), all(32 * mine.size() * W);
    for (size_t i = 0; i < mine.size(); i++) mine[i].to_bytes(s.data() + 32 * i);
    allgather(s.data(), all.data(), s.size());
    std::vector<Fr> out(mine.size() * W);
    for (size_t i = 0; i < out.size(); i++) out[i] = Fr::from_bytes(all.data() + 32 * i);
    return out;  // rank-major
  }
  uint32_t gather_or(uint32_t mine) {
    std::vector<uint32_t> all(W);
    allgather(&mine, all.data(), 4);
    uint32_t o = 0;
    for (uint32_t v : all) o |= v;
    return o;
  }
  HostAllgather host_ag() {
    return [this](const void* s, void* rv, size_t b) { allgather(s, rv, b); };
  }
  // Polynomial.degree (polynomial.js:212-226) of CYCLIC-sliced polynomials (rank r holds coefficients
  // r + W j, j < Ml): the highest nonzero global index over all ranks, 0 for the zero polynomial
  std::vector<uint64_t> degrees_cyc(const std::vector<const uint32_t*>& ops, uint64_t Ml) {
    const size_t m = ops.size();
    uint32_t* d = c.buf("d_qdeg", 4 * 16);
    HC(hipMemsetAsync(d, 0, 4 * 16, c.st));
    for (size_t i = 0; i < m; i++) launch_degree(c.st, d + i, ops[i], Ml);
    check_launch();
    uint8_t* h = c.pin(64 + 32 * m);
    HC(hipMemcpyAsync(h, d, 64, hipMemcpyDeviceToHost, c.st));
    for (size_t i = 0; i < m; i++) HC(hipMemcpyAsync(h + 64 + 32 * i, ops[i], 32, hipMemcpyDeviceToHost, c.st));
    HC(hipStreamSynchronize(c.st));
    std::vector<int64_t> mine(m);
    for (size_t i = 0; i < m; i++) {
      const uint32_t j = ((const uint32_t*)h)[i];
      bool nz0 = false;
      for (int b = 0; b < 32; b++) nz0 |= h[64 + 32 * i + b] != 0;
      mine[i] = j ? (int64_t)r + (int64_t)W * j : (nz0 ? (int64_t)r : -1);
    }
    std::vector<int64_t> all(m * W);
    allgather(mine.data(), all.data(), 8 * m);
    std::vector<uint64_t> deg(m, 0);
    for (size_t i = 0; i < m; i++)
      for (int q = 0; q < W; q++) deg[i] = std::max<int64_t>((int64_t)deg[i], all[q * m + i]);
    return deg;
  }
  // the full natural-order length-W*Ml vector of a CYCLIC-sliced polynomial, on this rank's device
  // (reference-quirks replay only: a host all-gather of the slices)
  uint32_t* gather_cyc(const uint32_t* sliceC, uint64_t Ml, const std::string& name) {
    std::vector<uint8_t> mine((size_t)32 * Ml), all((size_t)32 * Ml * W), full((size_t)32 * Ml * W);
    HC(hipMemcpyAsync(mine.data(), sliceC, mine.size(), hipMemcpyDeviceToHost, c.st));
    HC(hipStreamSynchronize(c.st));
    allgather(mine.data(), all.data(), mine.size());
    for (int q = 0; q < W; q++)
      for (uint64_t j = 0; j < Ml; j++)
        memcpy(&full[(size_t)32 * (q + W * j)], &all[(size_t)32 * (q * Ml + j)], 32);
    uint32_t* out = c.buf(name, full.size());
    HC(hipMemcpyAsync(out, full.data(), full.size(), hipMemcpyHostToDevice, c.st));
    HC(hipStreamSynchronize(c.st));
    return out;
  }
};

}  // namespace kgsi
