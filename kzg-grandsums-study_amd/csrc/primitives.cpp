// The C-ABI building blocks (include/kgs.h): field maps, NTTs, the grand-sum / grand-product builder,
// round 3, linear combinations, Horner evaluation and division, the lookup multiplicities, Keccak, the
// NTT timing loop. Each runs the round engine's own launches (prover.cpp) on the context's main stream
// over host buffers (the *_device ones: device buffers) and returns with its output complete.
#include "context.hpp"
#include "keccak.hpp"

using namespace kgs;
using namespace kgsi;

namespace {

// One primitive call on a context: the context locked and its device current, the staging areas reset
// on entry and on every way out; finish() returns only once the results have arrived.
struct Prim {
  kgs_ctx* c;
  std::lock_guard<std::mutex> lock;
  uint32_t* d_flags = nullptr;
  explicit Prim(kgs_ctx_t* ctx) : c(ctx ? ctx : throw KgsError(KGS_E_ARG, "NULL ctx")), lock(c->mu) {
    HC(hipSetDevice(c->device));
    c->reset_staging();
  }
  ~Prim() {
    try {
      c->reset_staging();
    } catch (...) {  // a failed drain has been, or will be, reported by a checked call
    }
  }
  // a pooled device buffer of max(bytes, capacity) with the upload of `bytes` enqueued
  uint32_t* up(const std::string& name, const void* host, size_t bytes, size_t capacity = 0) {
    uint32_t* d = c->buf(name, std::max(bytes, capacity));
    if (bytes) HC(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->st));
    return d;
  }
  // the 16 flag words the kernels report through, every byte set to `fill`
  uint32_t* flags(int fill = 0) {
    d_flags = c->buf("flags", 64);
    HC(hipMemsetAsync(d_flags, fill, 64, c->st));
    return d_flags;
  }
  // launches checked, `bytes` of dev copied to host_out (if given), everything drained; returns the
  // flag words (pinned, valid until this call ends) if flags() was asked for
  const uint32_t* finish(void* host_out = nullptr, const void* dev = nullptr, size_t bytes = 0) {
    check_launch();
    uint32_t* hf = d_flags ? (uint32_t*)c->pin(64) : nullptr;
    if (host_out) HC(hipMemcpyAsync(host_out, dev, bytes, hipMemcpyDeviceToHost, c->st));
    if (hf) HC(hipMemcpyAsync(hf, d_flags, 64, hipMemcpyDeviceToHost, c->st));
    c->sync();
    return hf;
  }
};

// the shim's elementwise maps (host buffers in and out, one launch on ctx's stream)
void fr_map(kgs_ctx_t* ctx, const uint8_t* in, uint8_t* out, uint64_t n,
            void (*launch)(hipStream_t, uint32_t*, const uint32_t*, uint64_t)) {
  if (!ctx || (n && (!in || !out))) throw KgsError(KGS_E_ARG, "NULL argument");
  if (!n) return;
  Prim p(ctx);
  uint32_t* a = p.up("prim_a", in, 32 * n);
  uint32_t* b = p.c->buf("prim_b", 32 * n);
  launch(p.c->st, b, a, n);
  p.finish(out, b, 32 * n);
}

void check_quot_kind(int kind, const void* sel_f, const void* sel_t) {
  if (kind != KGS_GRANDSUM && kind != KGS_GRANDPRODUCT && kind != KGS_LOOKUP) throw KgsError(KGS_E_ARG, "bad kind");
  if ((sel_f == nullptr) != (sel_t == nullptr)) throw KgsError(KGS_E_ARG, "selectors must be both given or both NULL");
  if (kind == KGS_LOOKUP && !sel_f) throw KgsError(KGS_E_ARG, "a lookup needs its selectors");
}

// Multiplicities of a lookup table (kgs.h; kernels in lookup.hip) on the context's main stream: device
// inputs, device output, and the output's copy to `host_out` when that is given. Returns once the
// stream is drained; the two error rows come back through the flags.
void lookup_multiplicities_impl(Prim& p, uint64_t n, const LookupCols& F, const LookupCols& T, const uint32_t* sel_f,
                                uint32_t* out, uint8_t* host_out) {
  kgs_ctx& c = *p.c;
  uint64_t cap = 2;
  while (cap < 2 * n) cap <<= 1;
  uint32_t* table = c.buf("lk_table", 4 * cap);
  uint32_t* count = c.buf("lk_count", 4 * n);
  HC(hipMemsetAsync(table, 0xFF, 4 * cap, c.st));
  HC(hipMemsetAsync(count, 0, 4 * n, c.st));
  launch_lookup_multiplicities(c.st, out, table, cap, count, p.flags(0xFF), F, T, sel_f, n);
  const uint32_t* hf = p.finish(host_out, out, 32 * n);
  const uint32_t miss = hf[0], bad_sel = hf[1];
  if (bad_sel != 0xFFFFFFFFu) throw KgsError(KGS_E_ARG, "selF is not binary at row " + std::to_string(bad_sel) + ".");
  if (miss != 0xFFFFFFFFu) throw KgsError(KGS_E_NOT_IN_TABLE, "Row " + std::to_string(miss) + " of F is not in the table.");
}

void lookup_check_args(kgs_ctx_t* ctx, int npols, uint64_t n, const void* f, const void* t, const void* out) {
  if (!ctx || !f || !t || !out) throw KgsError(KGS_E_ARG, "NULL argument");
  if (npols < 1 || npols > EB_MAX) throw KgsError(KGS_E_ARG, "npols must be in 1 .. " + std::to_string(EB_MAX));
  if (n < 1 || n > (1ull << 28)) throw KgsError(KGS_E_ARG, "n must be in 1 .. 2^28");
}

const char* const LOOKUP_NO_GROUP = "The multiplicities of a lookup are not computed on a context attached to a rank group.";

}  // namespace

extern "C" {

int kgs_fr_to_mont(kgs_ctx_t* ctx, const uint8_t* in_std, uint8_t* out_mont, uint64_t n) {
  API_BEGIN
  fr_map(ctx, in_std, out_mont, n, launch_to_mont);
  API_END
}

int kgs_fr_from_mont(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_std, uint64_t n) {
  API_BEGIN
  fr_map(ctx, in_mont, out_std, n, launch_from_mont);
  API_END
}

int kgs_fr_batch_inverse(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_mont, uint64_t n) {
  API_BEGIN
  fr_map(ctx, in_mont, out_mont, n, launch_fr_batch_inv);
  API_END
}

int kgs_ntt(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_mont, int logm, int inverse) {
  API_BEGIN
  Prim p(ctx);
  if (logm < 0 || logm > 28) throw KgsError(KGS_E_ARG, "bad logm");
  if (logm > ctx->logM) ensure_domain(*ctx, logm);
  const uint64_t m = 1ull << logm;
  uint32_t* a = p.up("prim_a", in_mont, 32 * m);
  uint32_t* b = ctx->buf("prim_b", 32 * m);
  if (inverse) {
    intt_nat(*ctx, b, a, logm);
  } else {
    ntt_dif(ctx->st, a, a, m, logm, nullptr, ctx->tw_fwd, ctx->logM);
    launch_bitrev_copy(ctx->st, b, a, logm);
  }
  p.finish(out_mont, b, 32 * m);
  API_END
}

// The provers' own launches of ntt_dif / ntt_dit (kgs.h): coset_fwd, coset_inv_prescaled, the distributed
// prover's last pass (post and post_s together), the replay's short-input forward, under either pass build.
int kgs_ntt_ex(kgs_ctx_t* ctx, const uint8_t* in_mont, uint64_t in_len, uint8_t* out_mont, int logm, int flags) {
  API_BEGIN
  Prim p(ctx);
  if (logm < 0 || logm > 28) throw KgsError(KGS_E_ARG, "bad logm");
  const int known = KGS_NTT_INVERSE | KGS_NTT_COSET | KGS_NTT_BITREV | KGS_NTT_NO_SCALE | KGS_NTT_INPLACE |
                    KGS_NTT_INFLIGHT;
  if (flags & ~known) throw KgsError(KGS_E_ARG, "unknown NTT flag");
  const bool inverse = flags & KGS_NTT_INVERSE, coset = flags & KGS_NTT_COSET, bitrev = flags & KGS_NTT_BITREV;
  const bool inplace = flags & KGS_NTT_INPLACE;
  const uint64_t m = 1ull << logm;
  if (inverse && inplace && !bitrev)
    throw KgsError(KGS_E_ARG, "an in-place inverse transform needs its input in bit-reversed order");
  if (inverse) in_len = m;
  if (in_len > m) throw KgsError(KGS_E_ARG, "input longer than the transform");
  if (!out_mont || (in_len && !in_mont)) throw KgsError(KGS_E_ARG, "NULL argument");
  if (logm > ctx->logM) ensure_domain(*ctx, logm);
  uint32_t* a = p.up("prim_a", in_mont, 32 * in_len, 32 * m);
  uint32_t* b = ctx->buf("prim_b", 32 * m);
  uint32_t* res = inplace ? a : b;
  {
    NttMode ntt_mode((flags & KGS_NTT_INFLIGHT) != 0);
    if (inverse) {
      ntt_dit(ctx->st, res, a, bitrev ? 1 : 0, logm, ctx->tw_inv, ctx->logM, coset ? ctx->coset_ipow : nullptr,
              (flags & KGS_NTT_NO_SCALE) ? nullptr : ctx->invm + 8 * logm);
    } else {
      ntt_dif(ctx->st, res, a, in_len, logm, coset ? ctx->coset_pow : nullptr, ctx->tw_fwd, ctx->logM);
      if (!bitrev) {
        uint32_t* nat = inplace ? b : a;
        launch_bitrev_copy(ctx->st, nat, res, logm);
        res = nat;
      }
    }
    check_launch();
  }
  p.finish(out_mont, res, 32 * m);
  API_END
}

// The batched block transforms as the coset openings and the recovery launch them (kgs.h): in place on one
// device buffer, the domain tables no larger than one block needs.
int kgs_ntt_blocks(kgs_ctx_t* ctx, const uint8_t* in_mont, uint8_t* out_mont, int logtotal, int s, int flags) {
  API_BEGIN
  Prim p(ctx);
  if (logtotal < 0 || logtotal > 28) throw KgsError(KGS_E_ARG, "bad logtotal");
  if (s < 0 || s > logtotal) throw KgsError(KGS_E_ARG, "s must be in 0 .. logtotal");
  if (flags & ~(KGS_NTT_INVERSE | KGS_NTT_NO_SCALE | KGS_NTT_INFLIGHT)) throw KgsError(KGS_E_ARG, "unknown NTT flag");
  if (!in_mont || !out_mont) throw KgsError(KGS_E_ARG, "NULL argument");
  if (s > ctx->logM) ensure_domain(*ctx, s);  // never logtotal: the stage tables are indexed by stage
  const size_t bytes = (size_t)32 << logtotal;
  uint32_t* a = p.up("prim_a", in_mont, bytes);
  {
    NttMode ntt_mode((flags & KGS_NTT_INFLIGHT) != 0);
    if (flags & KGS_NTT_INVERSE)
      ntt_dit_blocks(ctx->st, a, logtotal, s, ctx->tw_inv, (flags & KGS_NTT_NO_SCALE) ? nullptr : ctx->invm + 8 * s);
    else
      ntt_dif_blocks(ctx->st, a, logtotal, s, ctx->tw_fwd);
    check_launch();
  }
  p.finish(out_mont, a, bytes);
  API_END
}

int kgs_grand_build(kgs_ctx_t* ctx, int kind, const uint8_t* f_mont, const uint8_t* t_mont, const uint8_t* sel_f,
                    const uint8_t* sel_t, const uint8_t gamma_mont[32], uint64_t n, uint8_t* out_mont) {
  API_BEGIN
  Prim p(ctx);
  if ((sel_f == nullptr) != (sel_t == nullptr)) throw KgsError(KGS_E_ARG, "selectors must be both given or both NULL");
  const size_t E = 32 * n;
  uint32_t* f = p.up("gb_f", f_mont, E);
  uint32_t* t = p.up("gb_t", t_mont, E);
  uint32_t* o = ctx->buf("gb_o", E);
  uint32_t* sf = sel_f ? p.up("gb_sf", sel_f, E) : nullptr;
  uint32_t* st = sel_f ? p.up("gb_st", sel_t, E) : nullptr;
  Fr g = Fr::from_bytes(gamma_mont);
  uint32_t* dg = ctx->scal(&g, 1);
  uint32_t* flags = p.flags();
  const uint32_t ntiles = (uint32_t)((n + EVAL_TILE - 1) / EVAL_TILE);
  launch_builder(ctx->st, kind == KGS_GRANDPRODUCT, sel_f != nullptr, o, f, t, sf, st, dg, n,
                 ctx->buf("bt_tp", 32 * (ntiles + 1)), ctx->buf("bt_ti", 32 * (ntiles + 1)), flags);
  if (p.finish(out_mont, o, E)[0] != 0)
    throw KgsError(KGS_E_NOT_WELL_CALC, kind != KGS_GRANDPRODUCT ? "The grand-sum polynomial S is not well calculated"
                                                             : "The grand-product polynomial Z is not well calculated");
  API_END
}

// Round 3 and the linear combinations as the provers launch them (kgs.h): host buffers around
// run_quotient, run_divcheck and run_lincomb, the functions the round engine calls.
int kgs_quotient_ex(kgs_ctx_t* ctx, int nbits, int lcs, const kgs_quot_arg_t* args, int count,
                    const uint8_t alpha_mont[32], const uint8_t gamma_mont[32], const uint8_t delta_mont[32], int flags,
                    uint8_t* q_out) {
  API_BEGIN
  Prim p(ctx);
  if (nbits < 1 || nbits > 27) throw KgsError(KGS_E_ARG, "bad nbits");
  if (lcs != nbits && lcs != nbits + 1) throw KgsError(KGS_E_ARG, "the coset has n or 2n points");
  if (count < 1 || count > KGS_MAX_ARGS) throw KgsError(KGS_E_ARG, "bad argument count");
  if (flags & ~KGS_QUOT_FUSED) throw KgsError(KGS_E_ARG, "unknown quotient flag");
  if (!args || !alpha_mont || !gamma_mont || !q_out || (count > 1 && !delta_mont)) throw KgsError(KGS_E_ARG, "NULL argument");
  for (int j = 0; j < count; j++) {
    if (!args[j].S || !args[j].F || !args[j].T) throw KgsError(KGS_E_ARG, arg_prefix(j) + "NULL argument");
    check_quot_kind(args[j].kind, args[j].sel_f, args[j].sel_t);
  }
  if (lcs > ctx->logM) ensure_domain(*ctx, lcs);
  const size_t E = (size_t)32 << lcs;
  auto up = [&](int j, const char* what, const uint8_t* h) -> const uint32_t* {
    return h ? p.up("qx" + std::to_string(j) + "_" + what, h, E) : nullptr;
  };
  std::vector<QuotIn> in(count);
  for (int j = 0; j < count; j++) {
    const kgs_quot_arg_t& a = args[j];
    in[j] = QuotIn{a.kind, up(j, "S", a.S), up(j, "F", a.F), up(j, "T", a.T), up(j, "SF", a.sel_f), up(j, "ST", a.sel_t)};
  }
  std::vector<Fr> dpow(count, Fr::one());
  for (int j = 1; j < count; j++) dpow[j] = dpow[j - 1] * Fr::from_bytes(delta_mont);
  uint32_t* q = ctx->buf("qx_q", E);
  run_quotient(*ctx, nbits, lcs, in, Fr::from_bytes(alpha_mont), Fr::from_bytes(gamma_mont), dpow, q,
               count > 1 || (flags & KGS_QUOT_FUSED));
  p.finish(q_out, q, E);
  API_END
}

int kgs_divcheck(kgs_ctx_t* ctx, int kind, uint64_t n, const uint8_t* S, const uint8_t* f, const uint8_t* t,
                 const uint8_t* sel_f, const uint8_t* sel_t, const uint8_t alpha_mont[32], const uint8_t gamma_mont[32],
                 const uint8_t* s_next, uint64_t gbase, int* nonzero) {
  API_BEGIN
  Prim p(ctx);
  if (n < 1 || n > (1ull << 28)) throw KgsError(KGS_E_ARG, "bad n");
  if (!S || !f || !t || !alpha_mont || !gamma_mont || !nonzero) throw KgsError(KGS_E_ARG, "NULL argument");
  check_quot_kind(kind, sel_f, sel_t);
  const size_t E = 32 * n;
  auto up = [&](const char* name, const uint8_t* h) -> uint32_t* { return h ? p.up(name, h, E) : nullptr; };
  uint32_t* dS = p.up("dc_S", S, E, E + 32);  // S[n]: the continuation
  if (s_next) HC(hipMemcpyAsync(dS + 8 * n, s_next, 32, hipMemcpyHostToDevice, ctx->st));
  const QuotIn on_h{kind, dS, up("dc_f", f), up("dc_t", t), up("dc_sf", sel_f), up("dc_st", sel_t)};
  run_divcheck(*ctx, 0, 0, on_h, Fr::from_bytes(alpha_mont), Fr::from_bytes(gamma_mont), n, p.flags(),
               s_next ? dS + 8 * n : nullptr, gbase);
  *nonzero = p.finish()[0] != 0;
  API_END
}

int kgs_lincomb(kgs_ctx_t* ctx, const uint8_t* const* srcs, const uint64_t* lens, const uint8_t* coefs_mont, int count,
                const uint8_t c0_mont[32], uint64_t out_len, uint8_t* out_mont) {
  API_BEGIN
  Prim p(ctx);
  if (count < 0 || count > 256) throw KgsError(KGS_E_ARG, "bad term count");
  if (out_len < 1 || out_len > (1ull << 28)) throw KgsError(KGS_E_ARG, "bad output length");
  if (!c0_mont || !out_mont || (count && (!srcs || !lens || !coefs_mont))) throw KgsError(KGS_E_ARG, "NULL argument");
  // equal host pointers share one device copy (of the longest length asked of them)
  std::map<const uint8_t*, uint64_t> need;
  for (int k = 0; k < count; k++) {
    if (lens[k] > (1ull << 28)) throw KgsError(KGS_E_ARG, "bad term length");
    if (lens[k] && !srcs[k]) throw KgsError(KGS_E_ARG, "NULL source");
    if (lens[k]) need[srcs[k]] = std::max(need[srcs[k]], lens[k]);
  }
  uint64_t total = 0;
  for (auto& kv : need) total += kv.second;
  uint32_t* pool = ctx->buf("lc_src", 32 * (total ? total : 1));
  uint32_t* out = ctx->buf("lc_out", 32 * out_len);
  std::map<const uint8_t*, const uint32_t*> dev;
  uint64_t at = 0;
  for (auto& kv : need) {
    HC(hipMemcpyAsync(pool + 8 * at, kv.first, 32 * kv.second, hipMemcpyHostToDevice, ctx->st));
    dev[kv.first] = pool + 8 * at;
    at += kv.second;
  }
  LcTerms lt;
  for (int k = 0; k < count; k++) lt.add(lens[k] ? dev[srcs[k]] : pool, lens[k], Fr::from_bytes(coefs_mont + 32 * k));
  lt.c0 = Fr::from_bytes(c0_mont);
  run_lincomb(ctx->st, out, out_len, lt);
  p.finish(out_mont, out, 32 * out_len);
  API_END
}

int kgs_poly_eval(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t x_mont[32],
                  uint8_t out_mont[32]) {
  API_BEGIN
  Prim p(ctx);
  uint32_t* a = p.up("prim_a", coef_mont, 32 * len, 32);
  EvalJob j = eval_launch(*ctx, {a}, {len}, Fr::from_bytes(x_mont), 0);
  p.finish();
  eval_finish(j)[0].to_bytes(out_mont);
  API_END
}

int kgs_poly_div_x_sub(kgs_ctx_t* ctx, const uint8_t* coef_mont, uint64_t len, const uint8_t z_mont[32],
                       uint8_t* out_mont) {
  API_BEGIN
  Prim p(ctx);
  if (len < 2) throw KgsError(KGS_E_ARG, "length must be >= 2");
  uint32_t* a = p.up("prim_a", coef_mont, 32 * len);
  uint32_t* b = ctx->buf("prim_b", 32 * len);
  const uint32_t dt = (uint32_t)((len + EVAL_TILE - 1) / EVAL_TILE);
  launch_divide(ctx->st, b, p.flags(), a, len, xpowers(*ctx, Fr::from_bytes(z_mont)), ctx->buf("div_part", 32 * (dt + 1)),
                ctx->buf("div_carry", 32 * (dt + 1)));
  if (p.finish(out_mont, b, 32 * len)[0] != 0) throw KgsError(KGS_E_DOES_NOT_DIVIDE, "Polynomial does not divide");
  API_END
}

int kgs_lookup_multiplicities_device(kgs_ctx_t* ctx, int npols, uint64_t n, const void* const* d_evals_f,
                                     const void* const* d_evals_t, const void* d_sel_f, void* d_mul_t_mont) {
  API_BEGIN
  lookup_check_args(ctx, npols, n, d_evals_f, d_evals_t, d_mul_t_mont);
  Prim p(ctx);
  if (ctx->group) throw KgsError(KGS_E_ARG, LOOKUP_NO_GROUP);
  DrainOnError drain(ctx);
  LookupCols F{npols, {}}, T{npols, {}};
  for (int i = 0; i < npols; i++) {
    if (!d_evals_f[i] || !d_evals_t[i]) throw KgsError(KGS_E_ARG, "NULL argument");
    F.col[i] = (const uint32_t*)d_evals_f[i];
    T.col[i] = (const uint32_t*)d_evals_t[i];
  }
  lookup_multiplicities_impl(p, n, F, T, (const uint32_t*)d_sel_f, (uint32_t*)d_mul_t_mont, nullptr);
  API_END
}

int kgs_lookup_multiplicities(kgs_ctx_t* ctx, int npols, uint64_t n, const uint8_t* const* evals_f,
                              const uint8_t* const* evals_t, const uint8_t* sel_f, uint8_t* mul_t_mont) {
  API_BEGIN
  lookup_check_args(ctx, npols, n, evals_f, evals_t, mul_t_mont);
  Prim p(ctx);
  if (ctx->group) throw KgsError(KGS_E_ARG, LOOKUP_NO_GROUP);
  DrainOnError drain(ctx);
  const size_t E = 32 * (size_t)n;
  // F_0 .. F_{k-1}, T_0 .. T_{k-1}, selF, then the output
  uint32_t* in = ctx->buf("lk_in", E * (2 * (size_t)npols + 2));
  LookupCols F{npols, {}}, T{npols, {}};
  for (int i = 0; i < npols; i++) {
    if (!evals_f[i] || !evals_t[i]) throw KgsError(KGS_E_ARG, "NULL argument");
    uint32_t* df = in + (E / 4) * (size_t)i;
    uint32_t* dt = in + (E / 4) * (size_t)(npols + i);
    HC(hipMemcpyAsync(df, evals_f[i], E, hipMemcpyHostToDevice, ctx->st));
    HC(hipMemcpyAsync(dt, evals_t[i], E, hipMemcpyHostToDevice, ctx->st));
    F.col[i] = df;
    T.col[i] = dt;
  }
  uint32_t* dsel = nullptr;
  if (sel_f) {
    dsel = in + (E / 4) * (size_t)(2 * npols);
    HC(hipMemcpyAsync(dsel, sel_f, E, hipMemcpyHostToDevice, ctx->st));
  }
  uint32_t* dout = in + (E / 4) * (size_t)(2 * npols + 1);
  lookup_multiplicities_impl(p, n, F, T, dsel, dout, mul_t_mont);
  API_END
}

int kgs_keccak256(const uint8_t* data, uint64_t len, uint8_t out[32]) {
  host::keccak256(data, (size_t)len, out);
  return KGS_OK;
}

int kgs_bench_ntt(kgs_ctx_t* ctx, void* d_buf, int logm, int reps, double* ms) {
  API_BEGIN
  Prim p(ctx);
  if (logm > ctx->logM) ensure_domain(*ctx, logm);
  uint32_t* a = (uint32_t*)d_buf;
  const uint64_t m = 1ull << logm;
  *ms = EventTimer().ms(ctx->st, [&] {  // one interval around all the repetitions
    for (int r = 0; r < reps; r++) {
      ntt_dif(ctx->st, a, a, m, logm, nullptr, ctx->tw_fwd, ctx->logM);
      ntt_dit(ctx->st, a, a, 1, logm, ctx->tw_inv, ctx->logM, nullptr, ctx->invm + 8 * logm);
    }
  });
  API_END
}

}  // extern "C"
