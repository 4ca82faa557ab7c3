#!/usr/bin/env python3
"""bench.py — grand-sum KZG proofs/s at n = 2^20 on MI355X (BASELINE.json configs[1]).

A "step" is one complete grand-sum prover call (rounds 1-5 of src/grandsum/mset_eq_kzg_prover.js:
Montgomery conversion, iNTTs, 6 KZG commitments, S builder, quotient, evaluations, openings) on one
synthetic multiset of n = 2^20 elements (k = 1 vector, no selectors), with the inputs already
resident in HBM (kgs_prove_device). The SRS is a synthetic ptau of power 20 (tau =
keccak256("kgs-bench-tau") mod r) generated on the GPU by the product's own writer; SRS load and
MSM-table precompute happen once, before the timed region (the device SRS cache).

Per GPU, `--inflight` (default 4) independent proofs are in flight: one context (own HIP stream,
resident SRS copy, buffers) and one host thread each, so the latency-bound MSM tails and the host
sync points of one proof overlap the bulk kernels of another; `latency_ms_single_proof` is the
one-at-a-time latency on a single context, measured outside the timed region.

N > 1 GPUs (torchrun, one process per GPU): every rank proves its own independent multisets
(replicas, "weak" scaling); value = proofs of all ranks / max-over-ranks time. `--gpus N` is the
rank count: under a launcher WORLD_SIZE must equal it (else exit 2); started bare with N > 1 the
script launches its own N ranks (torch.distributed.run, 127.0.0.1) as a child process.

A plain run does only what the headline needs: it sets up, warms up the device-resident path, times
`--steps` proofs, and prints the line (metric, value, unit, ms_per_step, config, ...). `--dump-outputs
DIR` writes, after the timed steps, the last timed proof of every in-flight context as
DIR/commitments_ctx<i>.npy (6 x 16) and DIR/evaluations_ctx<i>.npy (3 x 8 for the default workload):
float64 arrays of the proof's 32-bit little-endian words, exact (N > 1: prefixed rank<r>_). The inputs
are seeded, so two builds run with the same arguments can be compared output for output. Every other
leg below runs only with `--full`, `latency_ms_single_proof` among them.

Extra fields in the JSON line of a `--full` run:
  proof_verified : one proof of the timed workload checked with the native verifier (pairing)
  host_buffer_inflight : the same steps, in flight the same way, through the drop-in boundary: kgs_prove
              on pageable host F/T with the Montgomery write-back into caller-owned host buffers
              (prover.js:147-148) — PCIe-inclusive, so never `value`; `vs_device_resident` is its ratio
              to `value`, and the host path's proof must equal the device path's
  host_buffer_boundary : single-proof latency of kgs_prove on pageable host buffers (median / spread of
              7) and of the JavaScript drop-in module (javascript_module: the library default, V8
              collecting on its own schedule; javascript_module_app_eager_gc: the application's opt-in,
              node --expose-gc + KGS_JS_EAGER_GC=1, one collection beside the GPU work of a lone proof)
  latency_ms_single_proof / latency_single_proof_ms / round_ms_single_proof : one proof at a time on one
              context (2 MSM lanes), device-resident inputs, median and spread of 7
  msm       : live HIP-event timing of the MSM phases at N = n (points/s, G1 adds/s)
  roofline  : the dominant kernel (MSM bucket accumulation, k_accumulate) in algorithmic Fq products/s
              against the chip's mad-only product rate (INT-VALU bound); traffic =
              PMC FETCH+WRITE from profiles/
  hbm_view  : proof-level bytes (SURVEY.md §8d's count over the reference op list) per second vs 8 TB/s
  extra_configs : BASELINE.json configs[2] (grand-product at n), configs[3] (grand-sum n = 2^24) and
              configs[4] (selected-vector k = 4, n = 2^22) — single GPU at N = 1; at N > 1 ONE proof at
              a time over all ranks with the distributed prover (every vector sharded; RCCL
              all-to-all / all-gather; strong scaling); each checks a proof and that ranks agree.
              They run last, under a watchdog (--legs-timeout, default 300 s): if a leg hangs, the
              line is printed without the rest (extra_configs.timeout says so) and every rank exits
              with status 3 (a hang is a failure, not a pass)
  cpu_baseline : the CPU port of the reference op list (oracle/c, OpenMP) on the same workload
roctx ranges "kgs_bench_timed_region" and "kgs_bench_msm_leg" let a rocprofv3 --marker-trace run be cut
to the headline's proofs and to the MSM leg (profiles/summarize_window.py).
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_pkg():
    spec = importlib.util.spec_from_file_location(
        "kgs_amd", os.path.join(HERE, "kzg-grandsums-study_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synth_evals(n, idx):
    """F: n elements, 4 x u64 from PCG64(seed 0x4B5A4753 + idx), top 3 bits cleared (< 2^253 < r),
    32 B LE standard form. T = F rotated by one (test/mset_eq_kzg_grandsum.test.js:27-30)."""
    rng = np.random.Generator(np.random.PCG64(0x4B5A4753 + idx))
    w = rng.integers(0, np.iinfo(np.uint64).max, size=(n, 4), dtype=np.uint64, endpoint=True)
    w[:, 3] &= np.uint64((1 << 61) - 1)
    f = np.ascontiguousarray(w).view(np.uint8).reshape(n, 32)
    t = np.roll(f, 1, axis=0)
    return f, t


BENCH_TAU = None


def log(msg):
    """progress on stderr (stdout carries only the JSON line)"""
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)
# v_mad_u64_u32 issue rate of the whole chip: 256 CUs x 4 SIMDs x 64 lanes / MAD_CYCLES x 2.4 GHz.
# MAD_CYCLES = 4: the architectural full rate of a wave64 VALU instruction on a 16-lane SIMD, which
# v_mad_u64_u32 reaches when its carry-out goes to an ordinary SGPR pair, as the compiler emits it
# (profiles/ubench/issue_rates2_r03.txt: 4.16 SIMD cycles including loop overhead, the same as every
# other full-rate VOP3 op; the 4.93 of ubench_r02.txt wrote VCC). One bucket add (madd-2008-s in
# 9 x 29-bit limbs, field29.hpp) issues 1,467 partial-product mads: 6 products x 162, 2 squares x 126
# (45 symmetric partial products + 81 for the reduction), and Y3 = R*T - Y1*PPP as one lazily reduced
# double product (243); the 8 carry mads per product of fq29::reduce_row32 are reduction overhead
MAD_CYCLES = 4.0
MAD_PEAK = 256 * 4 * 64 / MAD_CYCLES * 2.4e9
MADS_PER_ADD = 6 * 162 + 2 * 126 + 243
# mads per 254-bit Montgomery product: 9 x 29-bit CIOS (81 a*b + 81 m*q, the kernel's form) and the
# representation-neutral floor of 8 x 32-bit limbs (64 + 64 32x32-bit partial products)
MADS_PER_PRODUCT_29 = 162
MADS_PER_PRODUCT_32 = 128


def roctx_range(name):
    """roctx range around a bench phase (rocprofv3 --marker-trace), so a kernel trace can be cut to
    the timed region (profiles/summarize_window.py). No-op without the roctx library."""
    import contextlib
    try:
        lib = ctypes.CDLL("librocprofiler-sdk-roctx.so")
    except OSError:
        return contextlib.nullcontext()

    @contextlib.contextmanager
    def rng():
        lib.roctxRangePushA(name.encode())
        try:
            yield
        finally:
            lib.roctxRangePop()
    return rng()


def bench_tau():
    # keccak256("kgs-bench-tau") mod r, computed with the product's own keccak
    K = load_pkg()
    R = K.R
    return int.from_bytes(K.keccak256(b"kgs-bench-tau"), "big") % R


# Collectives run on RCCL ("nccl") with device tensors. KGS_BENCH_BACKEND=gloo rehearses N > 1 on a
# single-GPU box (host-tensor collectives, every rank on cuda:0); the driver never sets it.
BACKEND = os.environ.get("KGS_BENCH_BACKEND", "nccl")


def coll_device():
    import torch
    return "cpu" if BACKEND == "gloo" else f"cuda:{torch.cuda.current_device()}"


def max_over_ranks(t):
    import torch
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized():
        return t
    te = torch.tensor([t], dtype=torch.float64, device=coll_device())
    dist.all_reduce(te, op=dist.ReduceOp.MAX)
    return float(te.item())


def shared_ptau(ctx, nbits, dist):
    """Synthetic ptau of power `nbits`, written once per node by the product's GPU writer (rank 0
    writes to a temporary name and renames atomically; the other ranks wait at a barrier)."""
    path = f"/tmp/kgs_bench_p{nbits}.ptau"
    t0 = time.time()
    if int(os.environ.get("LOCAL_RANK", "0")) == 0 and not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}.tmp"
        ctx.write_synthetic_ptau(tmp, nbits, bench_tau())
        os.replace(tmp, path)
    if dist:
        dist.barrier()
    return path, time.time() - t0


def make_group(K, torch, dist, rank, world, local):
    """Rank group of the distributed prover for N > 1: RCCL (the communicator id made on rank 0 and
    broadcast through torch.distributed); the gloo rehearsal uses a host all-gather group."""
    if BACKEND == "gloo":
        return (K.Group.host(world, K.torch_allgather(), K.torch_alltoall()),
                "host all-gather + all-to-all group (gloo rehearsal)")
    uid = K.rccl_unique_id() if rank == 0 else bytes(128)
    t = torch.tensor(list(uid), dtype=torch.uint8, device=coll_device())
    dist.broadcast(t, 0)
    return K.Group.rccl(rank, world, bytes(t.cpu().tolist()), local), "RCCL over xGMI"


def large_leg(K, torch, dist, rank, world, local, nb, k, selected, proofs, label, group=None):
    """One large configuration (BASELINE configs[3] / [4]: SURVEY C4 / C5), same inputs on every
    rank: N = 1 on one GPU; N > 1 the distributed prover (kgs_ctx_set_group: every vector sharded —
    NTTs by all-to-all, builder scan, quotient, Horner, divisions and every MSM on per-rank slices),
    strong scaling; if no group could be made, MSM point-range sharding only (kgs_ctx_set_shard).
    The last proof is checked with the native verifier (kgs_verify_ptau: transcript replay + pairing)."""
    n = 1 << nb
    log(f"large leg: {label}")
    ctx = K.Context(local)
    ptau, _ = shared_ptau(ctx, nb, dist)
    t0 = time.time()
    # the distributed prover's ranks each hold only their SRS slice (points rank + world * j)
    sliced = world > 1 and group is not None
    ctx.load_ptau(ptau, nb, slice=(rank, world) if sliced else None)
    setup_s = time.time() - t0
    table_bytes = ctx.srs_slice_info()[2]
    keep, d_f, d_t = [], [], []
    for i in range(k):
        f, t = synth_evals(n, 5000 + i)
        tf = torch.from_numpy(f.reshape(-1).copy()).to(f"cuda:{local}")
        tt = torch.from_numpy(t.reshape(-1).copy()).to(f"cuda:{local}")
        keep += [tf, tt]
        d_f.append(tf.data_ptr())
        d_t.append(tt.data_ptr())
        del f, t
    sfp = stp = None
    if selected:  # selF = ones but the last, selT = ones but the first
        one = np.frombuffer(K.FR_ONE_MONT, dtype=np.uint8)
        sf = np.tile(one, n)
        st = sf.copy()
        sf[32 * (n - 1):] = 0
        st[:32] = 0
        tsf = torch.from_numpy(sf).to(f"cuda:{local}")
        tst = torch.from_numpy(st).to(f"cuda:{local}")
        keep += [tsf, tst]
        sfp, stp = tsf.data_ptr(), tst.data_ptr()
        del sf, st
    mode = "single GPU"
    if world > 1 and group is not None:
        ctx.set_group(group[0], rank)
        mode = f"distributed prover, every vector sharded over {world} ranks ({group[1]}), strong scaling"
    elif world > 1:
        ctx.set_shard(rank, world, K.torch_allgather(device=None if BACKEND == "gloo" else f"cuda:{local}"))
        mode = "msm point-range sharded (strong scaling)"
    ctx.prove_device(K.GRANDSUM, nb, d_f, d_t, sfp, stp)  # warm-up
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(proofs):
        coms, evs = ctx.prove_device(K.GRANDSUM, nb, d_f, d_t, sfp, stp)
    torch.cuda.synchronize()
    el = max_over_ranks(time.perf_counter() - t1)
    cn, en = K.proof_names(K.GRANDSUM, k, selected)
    verified = K.grandsum_verifier(ptau, {"commitments": dict(zip(cn, coms)), "evaluations": dict(zip(en, evs))}, nb)
    out = {"workload": label, "n_gpus": world, "mode": mode,
           "proofs": proofs, "ms_per_proof": round(1000.0 * el / proofs, 3),
           "proofs_per_s": round(proofs / el, 4), "srs_setup_s_rank0": round(setup_s, 2),
           "srs_table_bytes_rank0": table_bytes, "srs_slice": f"points r + {world} j" if sliced else "whole prefix",
           "proof_verified": verified,
           "round_ms_last_proof_rank0": [round(x, 3) for x in ctx.last_timing()[:5]]}
    if dist:
        h = torch.tensor(list(K.keccak256(b"".join(coms))[:8]), dtype=torch.int64, device=coll_device())
        hs = [torch.empty_like(h) for _ in range(world)]
        dist.all_gather(hs, h)
        out["ranks_agree"] = all(bool(torch.equal(hs[0], x)) for x in hs)
    if world > 1 and group is not None:
        # the last proof's exchanges (kgs_last_exchange: all-to-all spans by HIP events on the prover's
        # stream, host all-gathers by the wall clock), max over ranks, against DESIGN.md §6's model
        x = ctx.last_exchange()
        ex_ms = max_over_ranks(x["alltoall_ms"] + x["allgather_ms"])
        model = K.dist_exchange_model(K.GRANDSUM, nb, k, selected, world)
        out["exchange"] = {
            "compute_ms": round(1000.0 * el / proofs - ex_ms, 3), "exchange_ms": round(ex_ms, 3),
            "exchange_bytes": x["alltoall_bytes"] + x["allgather_bytes"],
            "alltoall": {"n": x["alltoall_n"], "ms_rank0": round(x["alltoall_ms"], 3), "bytes": x["alltoall_bytes"]},
            "allgather": {"n": x["allgather_n"], "ms_rank0": round(x["allgather_ms"], 3), "bytes": x["allgather_bytes"]},
            "model_alltoall": model,
            "note": "per rank, last proof: exchange_ms = max over ranks of the all-to-all spans (transfer + waiting for "
                    "peers) + host all-gather wall time; compute_ms = ms_per_proof - exchange_ms; bytes leave the rank"}
    ctx.set_shard(0, 1)
    ctx.set_group(None)
    ctx.close()
    del keep
    torch.cuda.empty_cache()
    return out


def self_launch(n):
    """Run this script as n ranks under torch.distributed.run (127.0.0.1, a free port) as a CHILD
    process — this process has not touched a GPU — and return its exit status."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"launching {n} ranks: {' '.join(cmd[2:])}")
    return subprocess.call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--nbits", type=int, default=20)
    ap.add_argument("--kind", choices=["grandsum", "grandproduct"], default="grandsum")
    ap.add_argument("--npols", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--msm-reps", type=int, default=5)
    ap.add_argument("--no-extra-legs", dest="extra_legs", action="store_false",
                    help="skip the grand-product (configs[2]), grand-sum 2^24 (configs[3]) and selected-vector "
                         "2^22 (configs[4]) legs")
    ap.add_argument("--no-host-leg", dest="host_leg", action="store_false",
                    help="skip the host-buffer boundary and JavaScript legs (profiling the timed region)")
    ap.add_argument("--sv-nbits", type=int, default=22)
    ap.add_argument("--c4-nbits", type=int, default=24, help="configs[3] leg (0 = skip)")
    ap.add_argument("--c4-proofs", type=int, default=3)
    ap.add_argument("--sv-proofs", type=int, default=3,
                    help="proofs timed in the selected-vector leg (N > 1: MSMs sharded over all ranks)")
    ap.add_argument("--legs-timeout", type=float, default=300.0,
                    help="watchdog on the extra legs (seconds, 0 = none): on expiry the line is printed without them")
    ap.add_argument("--launch-check", action="store_true",
                    help="start the ranks, join the process group, count the ranks with one collective, "
                         "print {n_gpus, ranks_joined} from rank 0 and exit (no GPU touched; CPU test of the launch)")
    ap.add_argument("--inflight", type=int, default=4,
                    help="independent proofs in flight per GPU (one context + HIP stream + host thread each)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline: proof checks, single-proof latency, the host-buffer "
                         "and JavaScript legs, MSM phases / roofline, CPU baseline and the extra configurations")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed proof of every in-flight context to "
                         "DIR/<name>.npy (float64 arrays holding the proof's 32-bit little-endian words)")
    args = ap.parse_args()
    # --gpus N is the number of ranks. Under a launcher (torchrun / torch.distributed.run) WORLD_SIZE
    # must agree with it; started bare with N > 1, bench.py launches its N ranks itself (one process
    # per GPU) before anything touches a GPU and exits with the launcher's status — never a silent
    # one-GPU run.
    if "WORLD_SIZE" in os.environ:
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}", file=sys.stderr)
            sys.exit(2)
    elif args.gpus > 1:
        sys.exit(self_launch(args.gpus))
    # stdout carries the JSON line only: chatter that libraries write straight to fd 1 (gloo's
    # connection report, RCCL warnings) is sent to stderr, and the line goes out on a saved copy of fd 1
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(BACKEND, rank=rank, world_size=world)
        if BACKEND == "gloo":
            local = 0
    if args.launch_check:
        joined = world
        if dist:
            t = torch.ones(1, dtype=torch.int64)
            dist.all_reduce(t)  # gloo: host tensors
            joined = int(t.item())
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"n_gpus": world, "ranks_joined": joined}), file=json_out, flush=True)
        return
    torch.cuda.set_device(local)
    K = load_pkg()
    ctx = K.Context(local)
    extra = [K.Context(local) for _ in range(args.inflight - 1)]

    nbits = args.nbits
    n = 1 << nbits
    kind = K.GRANDSUM if args.kind == "grandsum" else K.GRANDPRODUCT
    log("writing / loading the ptau")
    ptau, t_gen = shared_ptau(ctx, nbits, dist)
    t0 = time.time()
    ctx.load_ptau(ptau, nbits)
    for c in extra:
        c.load_ptau(ptau, nbits)
    t_load = time.time() - t0
    power, npts, window_c = ctx.srs_info()

    # inputs per in-flight context: pageable host buffers (the drop-in boundary, kgs_prove) and a
    # device-resident copy of the same multiset (kgs_prove_device); each context also owns the two
    # host buffers its Montgomery write-back lands in (prover.js:147-148), recycled across proofs as
    # the JS module's pool recycles its output buffers
    ctxs = [ctx] + extra
    bufs, hbufs, keep = [], [], []
    for ci, _ in enumerate(ctxs):
        d_f, d_t, h_f, h_t = [], [], [], []
        for i in range(args.npols):
            f, t = synth_evals(n, 1000 * rank + 100 * ci + i)
            tf = torch.from_numpy(f.reshape(-1).copy()).to(f"cuda:{local}")
            tt = torch.from_numpy(t.reshape(-1).copy()).to(f"cuda:{local}")
            keep += [tf, tt]
            d_f.append(tf.data_ptr())
            d_t.append(tt.data_ptr())
            if args.full:  # only the host-buffer legs read these
                h_f.append(f.tobytes())
                h_t.append(t.tobytes())
        bufs.append((d_f, d_t))
        if args.full:
            wb = ([bytearray(32 * n) for _ in range(args.npols)], [bytearray(32 * n) for _ in range(args.npols)])
            hbufs.append((h_f, h_t, wb))
    torch.cuda.synchronize()

    # what the caller of the timed path receives: the last (commitments, evaluations) of each context
    last_proof = [None] * len(ctxs)

    def run_dev(ci, count):
        c = ctxs[ci]
        d_f, d_t = bufs[ci]
        for _ in range(count):
            last_proof[ci] = c.prove_device(kind, nbits, d_f, d_t)

    def run_host(ci, count):
        c = ctxs[ci]
        h_f, h_t, wb = hbufs[ci]
        for _ in range(count):
            c.prove(kind, nbits, h_f, h_t, mont_out=wb)

    def steps(total, fn=run_dev):
        if len(ctxs) == 1:
            fn(0, total)
            return
        share = [total // len(ctxs) + (1 if i < total % len(ctxs) else 0) for i in range(len(ctxs))]
        th = [threading.Thread(target=fn, args=(i, share[i])) for i in range(len(ctxs))]
        for x in th:
            x.start()
        for x in th:
            x.join()

    def stats_ms(xs):
        xs = sorted(1000.0 * x for x in xs)
        return {"median": round(float(np.median(xs)), 3), "min": round(xs[0], 3), "max": round(xs[-1], 3),
                "samples": len(xs)}

    # throughput contexts: one MSM lane each (the in-flight proofs keep the GPU busy); the
    # single-proof latency below uses context 0 with two lanes (kgs_ctx_set_msm_lanes)
    for c in ctxs:
        c.set_msm_lanes(1 if len(ctxs) > 1 else 2)
    log("warm-up")
    steps(max(args.warmup, len(ctxs)), run_dev)
    LAT_SAMPLES = 7
    if args.full:
        steps(max(args.warmup, len(ctxs)), run_host)
        # single-proof latency (one proof at a time on one context), outside the timed region: median and
        # spread of LAT_SAMPLES proofs, device-resident and through the host-buffer boundary
        ctx.set_msm_lanes(2)
        run_dev(0, 1)
        t_lat = []
        for _ in range(LAT_SAMPLES):
            t1 = time.perf_counter()
            run_dev(0, 1)
            t_lat.append(time.perf_counter() - t1)
        rounds = ctx.last_timing()
        run_host(0, 1)
        t_hlat, h_timing = [], []
        for _ in range(LAT_SAMPLES):
            t1 = time.perf_counter()
            run_host(0, 1)
            t_hlat.append(time.perf_counter() - t1)
            h_timing.append(ctx.last_timing())
        latency = stats_ms(t_lat)
        latency_ms = latency["median"]
        # the proofs the bench times are real: one device-resident proof checked with the native verifier
        # (pairing), and the host-buffer path must give the identical proof and write back F's Montgomery form
        d_f0, d_t0 = bufs[0]
        coms0, evs0 = ctx.prove_device(kind, nbits, d_f0, d_t0)
        cn0, en0 = K.proof_names(kind, args.npols, False)
        vf = K.grandsum_verifier if kind == K.GRANDSUM else K.grandproduct_verifier
        proof_verified = vf(ptau, {"commitments": dict(zip(cn0, coms0)), "evaluations": dict(zip(en0, evs0))}, nbits)
        h_f0, h_t0, _ = hbufs[0]
        hcoms, hevs, hmf, _ = ctx.prove(kind, nbits, h_f0, h_t0)
        host_identical = (hcoms == coms0 and hevs == evs0
                          and bytes(hmf[0][:32 * 64]) == ctx.fr_to_mont(h_f0[0][:32 * 64]))
        ctx.set_msm_lanes(1 if len(ctxs) > 1 else 2)

    def timed(fn, label):
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        with roctx_range(label):
            ts = time.perf_counter()
            steps(args.steps, fn)
            torch.cuda.synchronize()
            if dist:
                dist.barrier()
            return max_over_ranks(time.perf_counter() - ts)

    # headline: device-resident inputs (the contract's `value`: inputs in HBM when the timed region
    # starts); right after it the same proofs through the host-buffer boundary, in flight the same way
    log("timed region")
    elapsed = timed(run_dev, "kgs_bench_timed_region")
    total_proofs = args.steps * world
    value = total_proofs / elapsed
    ms_per_step = 1000.0 * elapsed / args.steps
    log(f"timed: {value:.2f} proofs/s device-resident")
    if args.dump_outputs:
        # each context proves the same multiset in every step, so its last proof is the step's output;
        # a proof is a few hundred bytes, its 32-bit little-endian words are exact in float64
        os.makedirs(args.dump_outputs, exist_ok=True)
        pre = f"rank{rank}_" if world > 1 else ""
        for ci, (coms, evs) in enumerate(last_proof):
            for name, parts in (("commitments", coms), ("evaluations", evs)):
                words = np.frombuffer(b"".join(parts), dtype="<u4").reshape(len(parts), -1)
                np.save(os.path.join(args.dump_outputs, f"{pre}{name}_ctx{ci}.npy"), words.astype(np.float64))
    host_inflight = None
    if args.full:
        # the host-buffer path in flight: three regions of the same K steps, interleaved with two more
        # device-resident ones, so the ratio compares medians of neighbouring runs (a single pair of runs
        # spread 0.95-0.99 on one box, profiles/r06/host_inflight_modes.txt); `value` stays the first region
        el_hosts, el_devs = [], [elapsed]
        for i in range(3):
            el_hosts.append(timed(run_host, "kgs_bench_host_region"))
            if i < 2:
                el_devs.append(timed(run_dev, "kgs_bench_timed_region_extra"))
        el_host = float(np.median(el_hosts))
        host_inflight = {
            "proofs_per_s": round(total_proofs / el_host, 4), "ms_per_step": round(1000.0 * el_host / args.steps, 3),
            "vs_device_resident": round(float(np.median(el_devs)) / el_host, 4),
            "samples_proofs_per_s": [round(total_proofs / x, 3) for x in el_hosts],
            "device_samples_proofs_per_s": [round(total_proofs / x, 3) for x in el_devs],
            "proof_identical_to_device_path": host_identical,
            "note": (f"kgs_prove on pageable host F/T, {len(ctxs)} contexts in flight, Montgomery forms written back "
                     "into caller-owned host buffers (prover.js:147-148): PCIe-inclusive, K steps per region like "
                     "`value`; median of 3 regions, ratio against the median of 3 device-resident regions (the first "
                     "is `value`) run interleaved")}
        log(f"host-buffer in flight: {host_inflight['proofs_per_s']:.2f} proofs/s; JS leg")

    # ---------------- host-buffer boundary latency (what the JS / Python drop-in modules call): kgs_prove
    # on pageable host buffers, including the H2D copy of F/T and the D2H Montgomery write-back
    host_leg = None
    if args.full and rank == 0 and args.host_leg:
        hl = stats_ms(t_hlat)
        best = min(range(len(t_hlat)), key=lambda i: t_hlat[i])
        host_leg = {"ms_per_proof": hl["median"], "latency_ms": hl, "proofs_per_s": round(1000.0 / hl["median"], 3),
                    "ms_best": hl["min"], "libkgs_timing_ms_best": [round(x, 3) for x in h_timing[best]],
                    "note": f"single context (2 MSM lanes), one proof at a time, median of {LAT_SAMPLES}; F/T in "
                            "pageable host memory, Montgomery forms written back (prover.js:147-148)"}

        # the JavaScript drop-in module itself (north star: JS host -> N-API -> libkgs), if node and
        # the addon are present: 7 proofs, fresh inputs each, last proof verified
        import shutil
        import subprocess
        js_dir = os.path.join(HERE, "kzg-grandsums-study_amd", "js")
        if shutil.which("node") and os.path.exists(os.path.join(js_dir, "build", "kgs_addon.node")):
            try:
                # latency: 7 one-at-a-time proofs (best, median, spread; the library default, and a
                # caller that runs gc() between its calls); throughput: 16 concurrent chains of 7
                # awaited prover() calls over the module's context pool (8 contexts on this GPU)
                env = dict(os.environ, KGS_JS_CONTEXTS=str(2 * args.inflight), KGS_DEVICES=str(local))
                env.pop("KGS_JS_EAGER_GC", None)
                out = subprocess.run(["node", "--expose-gc", os.path.join(js_dir, "test", "time_prove.js"), ptau,
                                      str(nbits), "7",
                                      str(4 * args.inflight)], capture_output=True, text=True, timeout=300, env=env)
                host_leg["javascript_module"] = json.loads(out.stdout.strip().splitlines()[-1])
                # the same single-proof samples with the application's opt-in eager collection
                # (the module never changes V8 flags or collects by default)
                env["KGS_JS_EAGER_GC"] = "1"
                out = subprocess.run(["node", "--expose-gc", os.path.join(js_dir, "test", "time_prove.js"), ptau,
                                      str(nbits), "7", "0"], capture_output=True, text=True, timeout=300, env=env)
                eg = json.loads(out.stdout.strip().splitlines()[-1])
                host_leg["javascript_module_app_eager_gc"] = {
                    "ms_per_proof": eg["ms_per_proof"], "latency_ms": eg["latency_ms"], "verified": eg["verified"],
                    "best_inside_libkgs": eg["best_inside_libkgs"],
                    "note": "node --expose-gc with KGS_JS_EAGER_GC=1 (the application's opt-in): one full V8 "
                            "collection 5 ms after a lone proof is queued, beside its GPU work; 7 single proofs"}
            except Exception as e:  # the JS leg must not hide the GPU number
                host_leg.setdefault("javascript_module", {"error": str(e)[:200]})
                host_leg.setdefault("javascript_module_app_eager_gc", {"error": str(e)[:200]})

    msm = roofline = hbm_view = cpu = None
    extra_cfg = {}
    if args.full and rank == 0:
        log("MSM leg")
        # ---------------- MSM leg: live HIP-event timing of the phases at N = n
        sc = torch.from_numpy(synth_evals(n, 777)[0].reshape(-1).copy()).to(f"cuda:{local}")
        phase = (ctypes.c_double * 4)()
        entries = ctypes.c_uint64()
        reps = args.msm_reps
        with roctx_range("kgs_bench_msm_leg"):  # lets a rocprofv3 trace be cut to these dispatches
            K._check(K.lib().kgs_bench_msm_phases(ctx.handle, ctypes.c_void_p(sc.data_ptr()), n, reps, phase,
                                                  ctypes.byref(entries)))
        ph = [phase[i] / reps for i in range(4)]
        msm_ms = sum(ph)
        W = (255 + window_c - 1) // window_c
        B = 1 << (window_c - 1)
        # executed G1 additions: one mixed add per (bucket, point) entry + the bucket tail's row and
        # column sums (2B) and bit sums (c * 2^(l-1), l = c // 2; msm.hip k_rowcol / k_bitsum_rc) + host
        # Horner (2c); the combine of segment partials (~ segments) is left out
        adds_exec = entries.value + 2 * B + window_c * (1 << (window_c // 2 - 1)) + 2 * window_c
        msm = {
            "n_points": n, "window_c": window_c, "windows": W, "precomputed_windows": True,
            "ms": round(msm_ms, 4), "phase_ms": {"digits_sort": round(ph[0], 4), "accumulate": round(ph[1], 4),
                                                 "combine": round(ph[2], 4), "reduce": round(ph[3], 4)},
            "points_per_s": n / (msm_ms / 1e3),
            "g1_adds_per_s_canonical_16N": 16 * n / (msm_ms / 1e3),
            "g1_adds_executed": adds_exec,
            "g1_adds_per_s_executed": adds_exec / (msm_ms / 1e3),
        }

        # ---------------- roofline of the dominant kernel (k_accumulate)
        # The kernel is integer-VALU issue bound. Algorithmic work per launch: entries x 1 mixed XYZZ add
        # (madd-2008-s: 8M + 2S = 10 Fq Montgomery products). Peak: the Fq-product rate at which the
        # chip's measured v_mad_u64_u32 issue rate (MAD_PEAK: MAD_CYCLES SIMD cycles per wave64
        # instruction at the 2.4 GHz nominal clock, profiles/ubench/) is spent on nothing but the mads of
        # a product — no carries, loads or control: `peak` for the kernel's 9 x 29-bit product (162
        # mads), `peak_8x32` for the 128 mads of 8 x 32-bit limbs (the fewest 32x32-bit partial products
        # a 254-bit Montgomery product can have on this ISA). Timed with HIP events on the MSM's stream
        # around the k_accumulate launch alone.
        acc_ms = ph[1]
        mults = 10 * entries.value
        achieved = mults / (acc_ms / 1e3) / 1e9
        peak = MAD_PEAK / MADS_PER_PRODUCT_29 / 1e9
        peak32 = MAD_PEAK / MADS_PER_PRODUCT_32 / 1e9
        # HBM bytes per launch from the committed counter passes: FETCH_SIZE doubled (the guide's gfx950
        # correction: FETCH_SIZE tallies 128 B requests at 64 B) + WRITE_SIZE is `traffic`; the raw
        # FETCH_SIZE + WRITE_SIZE sum is reported beside it
        traffic = traffic_raw = None
        pmc_path = os.path.join(HERE, "profiles", "pmc_accumulate.json")
        if os.path.exists(pmc_path):
            try:
                with open(pmc_path) as fh:
                    pj = json.load(fh)
                traffic_raw = pj.get("hbm_bytes_per_launch")
                if pj.get("fetch_bytes_x2_corrected") is not None and pj.get("write_bytes") is not None:
                    traffic = pj["fetch_bytes_x2_corrected"] + pj["write_bytes"]
            except Exception:
                traffic = traffic_raw = None
        # the clock the chip holds under this kernel and its achieved SIMD cycles per VALU instruction,
        # from a committed counter pass (profiles/clock_accumulate.json; GRBM_GUI_ACTIVE / 8 / duration)
        clock = None
        clk_path = os.path.join(HERE, "profiles", "clock_accumulate.json")
        if os.path.exists(clk_path):
            try:
                with open(clk_path) as fh:
                    clock = json.load(fh)
            except Exception:
                clock = None
        roofline = {"bound": "valu", "kernel": "k_accumulate", "achieved": round(achieved, 2), "peak": round(peak, 2),
                    "unit": "G Fq-products/s", "frac": round(achieved / peak, 4),
                    "peak_8x32": round(peak32, 2), "frac_8x32": round(achieved / peak32, 4), "traffic": traffic,
                    "traffic_raw_fetch_plus_write": traffic_raw,
                    "traffic_vs_algorithmic": round(traffic / (68 * entries.value), 3) if traffic else None,
                    "traffic_note": "HBM bytes per 2^20-point launch from the FETCH_SIZE / WRITE_SIZE passes "
                                    "(profiles/pmc_accumulate.json): FETCH_SIZE x 2 (gfx950 correction) + WRITE_SIZE; "
                                    "above the 68 B/entry algorithmic bytes because each 64 B table point is a "
                                    "random gather",
                    "peak_note": f"v_mad_u64_u32 issue rate ({MAD_CYCLES} SIMD cycles per wave64 instruction, 256 CUs x 4 "
                                 f"SIMDs, 2.4 GHz) / mads per product: 162 (9 x 29-bit, peak) or 128 (8 x 32-bit, peak_8x32)",
                    "bound_note": "integer-VALU issue bound (254-bit Montgomery products on v_mad_u64_u32): neither the "
                                  "HBM roof (the kernel moves ~1 TB/s of 8) nor MFMA (no dense contraction) applies",
                    "mad_issue_frac": round(entries.value * MADS_PER_ADD / (acc_ms / 1e3) / MAD_PEAK, 4),
                    "g1_adds_per_s": round(entries.value / (acc_ms / 1e3)),
                    "algorithmic_bytes_per_launch": 68 * entries.value,
                    "hbm_gbps_algorithmic": round(68 * entries.value / (acc_ms / 1e3) / 1e9, 1)}
        if clock and clock.get("held_clock_ghz"):
            ghz = float(clock["held_clock_ghz"])
            roofline["held_clock"] = {
                "ghz": ghz, "peak_at_held_clock": round(peak * ghz / 2.4, 2),
                "frac_at_held_clock": round(achieved / (peak * ghz / 2.4), 4),
                "simd_cycles_per_valu_instruction": clock.get("simd_cycles_per_valu_instruction"),
                "issue_frac_vs_register_resident_add": clock.get("issue_frac_vs_register_resident_add"),
                "note": (f"counter passes (profiles/clock_accumulate.json, real cycles = GRBM_GUI_ACTIVE/8): the chip "
                         f"holds ~{ghz:.2f} GHz under this kernel, not 2.4; it issues one VALU instruction per "
                         f"~{clock.get('simd_cycles_per_valu_instruction')} SIMD cycles, against "
                         f"{clock.get('register_resident_add_cpi')} for the same add arithmetic register-resident "
                         f"(madd29 ubench); the rest of `peak` is the carries and reductions around the mads "
                         f"(DESIGN.md §3)")}

        # ---------------- proof-level HBM view (north star: achieved HBM-bandwidth fraction). Bytes per
        # proof = SURVEY.md §8d's count over the REFERENCE op list, B_gs(n) = 131 E = 4192 n (grand-sum,
        # k = 1, no selectors); the re-planned GPU path moves fewer, so this is an upper-bound view.
        b_proof = (4192 if args.kind == "grandsum" else 101 * 32) * n
        hbm_view = {"algorithmic_bytes_per_proof": b_proof, "achieved_GBps": round(b_proof * value / 1e9, 1),
                    "peak_GBps": 8000.0, "frac": round(b_proof * value / 1e9 / 8000.0, 4),
                    "accumulate_pmc_GBps": round(traffic / (acc_ms / 1e3) / 1e9, 1) if traffic else None,  # corrected
                    "note": "the proof is INT-VALU bound (MSM bucket accumulation), not HBM bound"}

        # ---------------- CPU baseline (oracle/c port of the reference op list), N = 1 only
        log("CPU baseline")
        cpu = None
        if world == 1 and not args.no_cpu_baseline:
            try:
                sys.path.insert(0, HERE)
                from oracle import cbackend
                # the same multiset as context 0's timed proofs, and its last proof compared byte for
                # byte with the GPU's (coms0 / evs0, device-resident path)
                cpu = cbackend.cpu_baseline(nbits, args.kind, threads=args.cpu_threads, ptau=ptau,
                                            inputs=(hbufs[0][0], hbufs[0][1]), expect=(coms0, evs0))
            except Exception as e:  # baseline failure must not hide the GPU number
                cpu = {"error": str(e)[:200]}


    out = {
        "metric": "grand-sum proofs/sec + MSM G1-adds/sec at n=2^20, 1/2/4/8 MI355X",
        "value": round(value, 4),
        "unit": "proofs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32 limbs (BN254 Fr/Fq Montgomery: 8 x 32-bit; MSM buckets 9 x 29-bit), int VALU",
        "data": "synthetic (PCG64-seeded multisets, T = rot(F); synthetic ptau, tau = keccak('kgs-bench-tau'))",
        "config": {"workload": f"{args.kind} prover, n=2^{nbits}, k={args.npols}, no selectors, inputs resident in HBM",
                   "nbits": nbits, "npols": args.npols, "selectors": False, "parallelism": f"replicas x{world}", "inflight_per_gpu": args.inflight,
                   "srs_power": power, "srs_points_resident": npts, "srs_gen_s": round(t_gen, 2),
                   "srs_load_s": round(t_load, 2)},
    }
    if not args.full:
        # a plain run ends with its headline: set up, warm up, time the steps, dump, print
        if rank == 0:
            print(json.dumps(out), file=json_out, flush=True)
        if dist:
            dist.barrier()
            dist.destroy_process_group()
        return
    out.update({
        "proof_verified": proof_verified,
        "host_buffer_inflight": host_inflight,
        "host_buffer_boundary": host_leg,
        "latency_ms_single_proof": round(latency_ms, 3),
        "latency_single_proof_ms": latency,
        "round_ms_single_proof": [round(x, 3) for x in rounds],
        "msm": msm,
        "roofline": roofline,
        "hbm_view": hbm_view,
        "extra_configs": extra_cfg,
        "cpu_baseline": cpu,
    })

    # The extra legs run last, under a watchdog: at N > 1 they exercise the RCCL transport of the
    # distributed prover, and a rank that hangs there must not cost the headline line. On expiry rank
    # 0 prints the line with the legs measured so far and every rank exits.
    emitted = threading.Lock()
    state = {"printed": False}

    def emit():
        with emitted:
            if rank == 0 and not state["printed"]:
                print(json.dumps(dict(out, extra_configs=dict(extra_cfg))), file=json_out, flush=True)
                state["printed"] = True

    def legs_timeout():
        extra_cfg["timeout"] = f"extra legs exceeded {args.legs_timeout} s; line emitted without the rest"
        log(extra_cfg["timeout"])
        emit()
        json_out.flush()
        os._exit(3)  # the line is out, but a hung leg is a failure the launcher must see

    wd = None
    if args.legs_timeout > 0:
        wd = threading.Timer(args.legs_timeout + (0 if rank == 0 else 30), legs_timeout)
        wd.daemon = True
        wd.start()
    # ---------------- extra configs (BASELINE.json configs[2] and [4]), outside the timed region
    log("extra configs")
    if args.extra_legs:
        # C3: grand-product at the same n, same contexts / inputs (replicas per GPU)
        gp_steps = 4 * len(ctxs)
        kind_main = kind
        kind = K.GRANDPRODUCT if kind_main == K.GRANDSUM else K.GRANDSUM
        steps(len(ctxs))
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        steps(gp_steps)
        torch.cuda.synchronize()
        el = max_over_ranks(time.perf_counter() - t1)
        # one proof of this leg checked with the native verifier (transcript replay + pairing)
        d_f0, d_t0 = bufs[0]
        coms1, evs1 = ctxs[0].prove_device(kind, nbits, d_f0, d_t0)
        cn1, en1 = K.proof_names(kind, args.npols, False)
        vf1 = K.grandsum_verifier if kind == K.GRANDSUM else K.grandproduct_verifier
        extra_cfg["grandproduct_vs_grandsum" if kind_main == K.GRANDSUM else "grandsum_vs_grandproduct"] = {
            "workload": f"{'grandproduct' if kind == K.GRANDPRODUCT else 'grandsum'} prover, n=2^{nbits}, k={args.npols}, no selectors",
            "proofs_per_s": round(gp_steps * world / el, 4), "proofs": gp_steps * world,
            "proof_verified": vf1(ptau, {"commitments": dict(zip(cn1, coms1)), "evaluations": dict(zip(en1, evs1))}, nbits)}
        kind = kind_main
        # C5 (N = 1: one GPU; N > 1: every MSM point-range sharded over all ranks, RCCL all-gather)
        for c in ctxs[1:]:
            c.close()
        ctxs[1:] = []
        group = None
        if world > 1:
            try:
                group = make_group(K, torch, dist, rank, world, local)
            except Exception as e:  # fall back to MSM-only sharding rather than losing the legs
                extra_cfg["group_error"] = str(e)[:200]
        def leg(*a):
            # a failing leg must not lose the headline line: a library failure on one rank aborts the
            # rank group, so every rank raises here and they stay in step
            if os.environ.get("KGS_BENCH_FORCE_LEG_HANG"):  # test hook: a leg that never returns
                time.sleep(1e9)
            try:
                return large_leg(K, torch, dist, rank, world, local, *a, group)
            except Exception as e:
                log(f"leg failed: {e}")
                torch.cuda.synchronize()
                return {"workload": a[4], "error": str(e)[:300]}
        extra_cfg["selected_vector"] = leg(args.sv_nbits, 4, True, args.sv_proofs,
                                           f"selected-vector grand-sum, n=2^{args.sv_nbits}, k=4, selectors")
        if args.c4_nbits > 0:
            extra_cfg["large_grandsum"] = leg(args.c4_nbits, 1, False, args.c4_proofs,
                                              f"grand-sum, n=2^{args.c4_nbits}, k=1, no selectors")
        if group is not None:
            group[0].close()

    if wd is not None:
        wd.cancel()
    emit()
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
