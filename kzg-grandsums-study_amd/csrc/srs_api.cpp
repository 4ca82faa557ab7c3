// The SRS entry points of the C-ABI (include/kgs.h): points or a ptau file (whole, or a rank's slice)
// into the device tables (msm_commit.cpp load_points), what a context reports about its SRS, and the
// synthetic ptau writer (fixed-base multiples on the device, or on the host without a context).
#include <sys/stat.h>

#include "context.hpp"
#include "host_pairing.hpp"
#include "ptau_io.hpp"

using namespace kgs;
using namespace kgsi;

// ------------------------------------------------------------------ host G2 (synthetic ptau): host_pairing.hpp
using host::G2A;
using host::g2_add;
using host::g2_gen;
using host::g2_lem;

// fixed-base table (d * 2^(8j)) G, affine LEM, 32 x 256
static std::vector<uint8_t> g1_fixed_table() {
  std::vector<uint8_t> tbl(32 * 256 * 64, 0);
  uint8_t gen[64];
  Fq::one().to_bytes(gen);
  Fq::from_u64(2).to_bytes(gen + 32);
  host::G1 base = host::G1::from_affine_lem(gen);
  for (int j = 0; j < 32; j++) {
    host::G1 acc = host::G1::inf();
    for (int d = 1; d < 256; d++) {
      acc = acc.add(base);
      acc.to_affine_lem(&tbl[64 * (j * 256 + d)]);
    }
    for (int s = 0; s < 8; s++) base = base.dbl();
  }
  return tbl;
}

extern "C" int kgs_srs_load_points(kgs_ctx_t* ctx, const uint8_t* g1_lem, uint64_t npts, int power, int nbits_max) {
  API_BEGIN
  if (!ctx || !g1_lem) throw KgsError(KGS_E_ARG, "NULL argument");
  CTX_LOCK(ctx);
  HC(hipSetDevice(ctx->device));
  if (nbits_max < 0) nbits_max = power;
  if (nbits_max > 28) throw KgsError(KGS_E_ARG, "nbits_max must be <= 28");
  uint64_t need = 1ull << (nbits_max + 1);
  if (npts < need) need = npts;
  load_points(*ctx, g1_lem, need, power, nbits_max, "");
  API_END
}

// ptau section 2 -> device tables: the first 2^(nbits_max+1) points, or (world > 1) rank's slice of
// them, the points rank + world * j, read in chunks and subsampled on the host
static void load_ptau_impl(kgs_ctx_t* ctx, const char* path, int nbits_max, int rank, int world) {
  if (!ctx || !path) throw KgsError(KGS_E_ARG, "NULL argument");
  if (world < 1 || world > 16 || (world & (world - 1)) || rank < 0 || rank >= world)
    throw KgsError(KGS_E_ARG, "SRS slice: world must be 1, 2, 4, 8 or 16 and 0 <= rank < world");
  CTX_LOCK(ctx);
  HC(hipSetDevice(ctx->device));
  FILE* f = fopen(path, "rb");
  if (!f) throw KgsError(KGS_E_IO, std::string("cannot open ") + path);
  std::unique_ptr<FILE, int (*)(FILE*)> guard(f, fclose);
  PtauInfo info = read_ptau_header(f, path);
  if (nbits_max < 0 || nbits_max > info.power) nbits_max = info.power;
  if (nbits_max > 28) throw KgsError(KGS_E_SRS, "ptau power above 28 is not supported");
  // file identity: the reference re-reads the file on every call, so a rewritten file (same path,
  // new size or mtime) must not hit the device cache
  struct stat stt;
  if (fstat(fileno(f), &stt) != 0) throw KgsError(KGS_E_IO, std::string("cannot stat ") + path);
  char real[4096];
  const char* rp = realpath(path, real) ? real : path;
  const std::string file = std::string(rp) + "#" + std::to_string((long long)stt.st_size) + "#" +
                           std::to_string((long long)stt.st_mtim.tv_sec) + "." + std::to_string((long long)stt.st_mtim.tv_nsec);
  // grow-only: tables loaded for a larger domain of the same file (and slice) serve every smaller proof
  if (ctx->srs && ctx->srs->file == file && ctx->srs->nbits_max >= nbits_max && ctx->srs->slice_rank == rank &&
      ctx->srs->slice_world == world)
    return;
  uint64_t avail = info.s2_size / 64;
  if (avail < 2) throw KgsError(KGS_E_IO, std::string(path) + ": ptau has no tauG1 section");
  uint64_t need = 1ull << (nbits_max + 1);
  if (need > avail) need = avail;
  const uint64_t mine = need > (uint64_t)rank ? (need - rank + world - 1) / world : 0;  // points rank + world j < need
  if (mine < 2) throw KgsError(KGS_E_ARG, "SRS slice needs at least 2 points");
  std::vector<uint8_t> pts(mine * 64);
  if (fseeko(f, (off_t)info.s2_pos, SEEK_SET)) throw KgsError(KGS_E_IO, "cannot read tauG1 section");
  if (world == 1) {
    if (fread(pts.data(), 1, pts.size(), f) != pts.size()) throw KgsError(KGS_E_IO, "cannot read tauG1 section");
  } else {
    const uint64_t CH = (uint64_t)world << 16;  // points per read
    std::vector<uint8_t> buf(CH * 64);
    uint64_t j = 0;
    for (uint64_t p0 = 0; p0 < need; p0 += CH) {
      const uint64_t cnt = need - p0 < CH ? need - p0 : CH;
      if (fread(buf.data(), 1, cnt * 64, f) != cnt * 64) throw KgsError(KGS_E_IO, "cannot read tauG1 section");
      for (uint64_t q = (uint64_t)rank; q < cnt; q += world) memcpy(&pts[64 * j++], &buf[64 * q], 64);
    }
  }
  load_points(*ctx, pts.data(), mine, info.power, nbits_max, file, rank, world);
}

extern "C" {

int kgs_srs_load_ptau(kgs_ctx_t* ctx, const char* path, int nbits_max) {
  API_BEGIN
  load_ptau_impl(ctx, path, nbits_max, 0, 1);
  API_END
}

int kgs_srs_load_ptau_slice(kgs_ctx_t* ctx, const char* path, int nbits_max, int rank, int world) {
  API_BEGIN
  load_ptau_impl(ctx, path, nbits_max, rank, world);
  API_END
}

int kgs_srs_slice_info(kgs_ctx_t* ctx, int* rank, int* world, uint64_t* table_bytes) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  if (rank) *rank = ctx->srs_slice_rank;
  if (world) *world = ctx->srs_slice_world;
  if (table_bytes) *table_bytes = ctx->srs ? (uint64_t)ctx->tb.W * ctx->tb.npts * 64 : 0;
  API_END
}

int kgs_srs_info(kgs_ctx_t* ctx, int* power, uint64_t* npts, int* window_c) {
  API_BEGIN
  if (!ctx) throw KgsError(KGS_E_ARG, "NULL ctx");
  CTX_LOCK(ctx);
  if (power) *power = ctx->srs_power;
  if (npts) *npts = ctx->tb.npts;
  if (window_c) *window_c = ctx->tb.c;
  API_END
}

int kgs_srs_zero_points(kgs_ctx_t* ctx, int* zero_points) {
  API_BEGIN
  if (!ctx || !zero_points) throw KgsError(KGS_E_ARG, "NULL argument");
  CTX_LOCK(ctx);
  *zero_points = ctx->srs ? (ctx->tb.zero_points ? 1 : 0) : -1;
  API_END
}

int kgs_ptau_write_synthetic(kgs_ctx_t* ctx, const char* path, int power, const uint8_t tau_std[32]) {
  API_BEGIN
  if (!path || !tau_std || power < 1 || power > 28) throw KgsError(KGS_E_ARG, "bad argument");
  uint64_t s[4];
  memcpy(s, tau_std, 32);
  Fr tau = Fr::from_std(s);
  const uint64_t n1 = (1ull << (power + 1)) - 1;
  std::vector<uint8_t> g1(n1 * 64);
  std::vector<uint8_t> tbl = g1_fixed_table();
  if (ctx) {
    CTX_LOCK(ctx);
    HC(hipSetDevice(ctx->device));
    ctx->reset_staging();
    uint32_t* d_tau = ctx->scal(&tau, 1);
    uint32_t* pw = ctx->buf("syn_pow", 32 * n1);
    uint32_t* xy = ctx->buf("syn_xyzz", 128 * n1);
    uint32_t* scr = ctx->buf("syn_scr", 32 * n1);
    uint32_t* aff = ctx->buf("syn_aff", 64 * n1);
    uint32_t* dtbl = ctx->buf("syn_tbl", tbl.size());
    HC(hipMemcpyAsync(dtbl, tbl.data(), tbl.size(), hipMemcpyHostToDevice, ctx->st));
    launch_powers(ctx->st, pw, n1, d_tau, nullptr);
    launch_fixed_base(ctx->st, xy, pw, n1, dtbl);
    launch_batch_affine(ctx->st, aff, xy, scr, n1);
    check_launch();
    HC(hipMemcpyAsync(g1.data(), aff, g1.size(), hipMemcpyDeviceToHost, ctx->st));
    ctx->reset_staging();
  } else {
    Fr t = Fr::one();
    for (uint64_t i = 0; i < n1; i++) {
      uint64_t e[4];
      t.to_std(e);
      host::G1 acc = host::G1::inf();
      for (int j = 0; j < 32; j++) {
        unsigned d = (unsigned)((e[j >> 3] >> (8 * (j & 7))) & 0xff);
        if (d) acc = acc.add(host::G1::from_affine_lem(&tbl[64 * (j * 256 + d)]));
      }
      acc.to_affine_lem(&g1[64 * i]);
      t = t * tau;
    }
  }
  // [1]_2, [tau]_2
  G2A g = g2_gen(), acc{g.x, g.y, true}, base = g;
  uint64_t e[4];
  tau.to_std(e);
  for (int i = 0; i < 256; i++) {
    if ((e[i >> 6] >> (i & 63)) & 1) acc = g2_add(acc, base);
    base = g2_add(base, base);
  }
  uint8_t g2[256];
  g2_lem(g, g2);
  g2_lem(acc, g2 + 128);
  FILE* f = fopen(path, "wb");
  if (!f) throw KgsError(KGS_E_IO, std::string("cannot create ") + path);
  std::unique_ptr<FILE, int (*)(FILE*)> guard(f, fclose);
  auto w32 = [&](uint32_t x) { fwrite(&x, 4, 1, f); };
  auto w64 = [&](uint64_t x) { fwrite(&x, 8, 1, f); };
  fwrite("ptau", 1, 4, f);
  w32(1);
  w32(3);
  w32(1);
  w64(44);
  w32(32);
  fwrite(host::FQ_MOD.p, 1, 32, f);
  w32((uint32_t)power);
  w32((uint32_t)power);
  w32(2);
  w64(g1.size());
  fwrite(g1.data(), 1, g1.size(), f);
  w32(3);
  w64(256);
  if (fwrite(g2, 1, 256, f) != 256) throw KgsError(KGS_E_IO, "write failed");
  API_END
}

}  // extern "C"
