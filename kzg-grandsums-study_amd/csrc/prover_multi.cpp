// The multi-argument prover's entry points (include/kgs.h kgs_prove_multi, kgs_prove_multi_device;
// DESIGN.md §16): the shape checks, the staging of host inputs, then the rounds (prover_rounds.cpp) as
// the multi prover runs them — no host-boundary hooks, round 1 unpiped, always exact-math (no reference
// behaviour exists to follow) and every failing argument named, for one argument too.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/kgs.h"
#include "context.hpp"

using namespace kgs;
using namespace kgsi;

namespace {

// shape checks shared by the two entry points; `host`: the pointers are host memory, staged by plain copies
void prove_multi_entry(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* in, int count, uint8_t* com_out, uint8_t* ev_out,
                       bool host) {
  if (!ctx || !in || !com_out || !ev_out) throw KgsError(KGS_E_ARG, "NULL argument");
  if (count < 1 || count > KGS_MAX_ARGS)
    throw KgsError(KGS_E_ARG, "the number of arguments must be in 1 .. " + std::to_string(KGS_MAX_ARGS));
  if (nbits < 1 || nbits > 28) throw KgsError(KGS_E_ARG, "nbits must be in 1 .. 28");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (ctx->group)
    throw KgsError(KGS_E_ARG, "A multi-argument proof is not computed on a context attached to a rank group.");
  if (ctx->shard_world > 1)
    throw KgsError(KGS_E_ARG, "A multi-argument proof is not computed on a context with MSM sharding (kgs_ctx_set_shard).");
  size_t nvec = 0;
  for (int j = 0; j < count; j++) {
    const kgs_arg_t& a = in[j];
    if (a.kind != KGS_GRANDSUM && a.kind != KGS_GRANDPRODUCT && a.kind != KGS_LOOKUP)
      throw KgsError(KGS_E_ARG, arg_prefix(j) + "unknown argument kind");
    if (a.npols < 1) throw KgsError(KGS_E_ARG, arg_prefix(j) + "The number of multisets must be greater than 0.");
    if (a.npols > KGS_MAX_POLS) throw KgsError(KGS_E_ARG, arg_prefix(j) + "too many multisets");
    if (!a.evals_f || !a.evals_t) throw KgsError(KGS_E_ARG, arg_prefix(j) + "NULL argument");
    for (int i = 0; i < a.npols; i++)
      if (!a.evals_f[i] || !a.evals_t[i]) throw KgsError(KGS_E_ARG, arg_prefix(j) + "NULL argument");
    if ((a.sel_f == nullptr) != (a.sel_t == nullptr))
      throw KgsError(KGS_E_ARG, arg_prefix(j) + "selectors must be both given or both NULL");
    if (a.kind == KGS_LOOKUP && !a.sel_f)
      throw KgsError(KGS_E_ARG, arg_prefix(j) + "a lookup needs both selectors (sel_t holds the multiplicities)");
    nvec += 2 * (size_t)a.npols + (a.sel_f ? 2 : 0);
  }
  HC(hipSetDevice(ctx->device));
  DrainOnError drain(ctx);
  const size_t E = (size_t)32 << nbits;
  uint32_t* stage = nullptr;
  if (host) {
    ctx->sync();
    stage = ctx->buf("multi_in", nvec * E);
  }
  size_t at = 0;
  auto take = [&](const void* p) -> const uint32_t* {
    if (!host) return (const uint32_t*)p;
    uint32_t* d = stage + (E / 4) * at++;
    HC(hipMemcpyAsync(d, p, E, hipMemcpyHostToDevice, ctx->st));
    return d;
  };
  std::vector<ArgIn> args(count);
  for (int j = 0; j < count; j++) {
    args[j].kind = in[j].kind;
    args[j].k = in[j].npols;
    for (int i = 0; i < in[j].npols; i++) {
      args[j].f_std.push_back(take(in[j].evals_f[i]));
      args[j].t_std.push_back(take(in[j].evals_t[i]));
    }
    if (in[j].sel_f) {
      args[j].sel_f = take(in[j].sel_f);
      args[j].sel_t = take(in[j].sel_t);
    }
  }
  ctx->xs.reset();
  ensure_twin(*ctx);
  check_srs(*ctx, nbits);
  if (nbits > ctx->nbits_max) throw KgsError(KGS_E_ARG, "nbits is outside the loaded SRS; reload with a larger nbits_max");
  RoundOpts o;
  o.name_arguments = true;
  prove_rounds(*ctx, nbits, args, o, com_out, ev_out);
}

}  // namespace

extern "C" {

int kgs_prove_multi(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* args, int count, uint8_t* commitments_out,
                    uint8_t* evaluations_out) {
  API_BEGIN
  prove_multi_entry(ctx, nbits, args, count, commitments_out, evaluations_out, true);
  API_END
}

int kgs_prove_multi_device(kgs_ctx_t* ctx, int nbits, const kgs_arg_t* args, int count, uint8_t* commitments_out,
                           uint8_t* evaluations_out) {
  API_BEGIN
  prove_multi_entry(ctx, nbits, args, count, commitments_out, evaluations_out, false);
  API_END
}

}  // extern "C"
