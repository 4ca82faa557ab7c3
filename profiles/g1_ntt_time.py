#!/usr/bin/env python3
"""Time the G1 transform and what is built on it at n = 2^lg, one process per n, over the
points tau^i G of a synthetic ptau:
  ntt_ms          kgs_g1_ntt_device, forward and inverse, with one twiddle per lane ("lane") and one per
                  wave wherever a stage has 64 butterfly groups ("wave"); HIP events on the context's
                  stream (kgs_bench_g1_ntt), median of --reps after a warm-up
  scale_ms        the scaling pass alone: n multiplications by one launch-uniform 254-bit constant, the
                  schedule of k_tab_scale, same events. model_ms = (n/2) log2 n multiplications at that
                  rate; model_fraction = model_ms / the forward transform's time
  lagrange_ms     kgs_srs_lagrange(NULL): "cold" the one call that builds the row, "cached" the median of
                  the calls after it (wall clock; the call ends synchronised)
  commit_ms       per family of evaluations (random, 16-bit, 0/1): "evals" kgs_commit_evals_device over
                  the cached Lagrange row, "coeff" the route it replaces with the same device-resident
                  input (to Montgomery form, inverse NTT, kgs_msm over the resident window tables:
                  kgs_bench_coeff_commit); wall clock of the whole call, median of --reps after a
                  warm-up; the two results are compared byte for byte

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no
further child after one that failed or timed out.
usage: g1_ntt_time.py [--lg 16,20] [--reps 5] [--limit 500] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def wall(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def one(lg, reps):
    import common
    from oracle import ptau as opt
    K = common.load_pkg()
    L = K.lib()
    L.kgs_bench_g1_ntt.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.kgs_bench_coeff_commit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    n = 1 << lg
    ctx = K.Context(0)
    path = f"/tmp/kgs_g1_ntt_time_p{lg}.{os.getpid()}.ptau"
    try:
        ctx.write_synthetic_ptau(path, lg, common.tau())
        pts = opt.PTau(path).g1_bytes[:64 * n]
        ctx.load_ptau(path, lg)
    finally:
        if os.path.exists(path):
            os.remove(path)

    def ok(rc):
        assert rc == 0, L.kgs_last_error().decode()

    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def dev(data):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), len(data)) == 0 and hip.hipMemcpy(p, data, len(data), 1) == 0
        return p

    rec = {"lg_n": lg, "reps": reps}
    dP, dO = dev(pts), dev(bytes(64 * n))
    arr = (ctypes.c_double * reps)()

    def events(what, mapping):
        ok(L.kgs_bench_g1_ntt(ctx.handle, dP, dO, lg, what, mapping, reps, arr))
        return round(statistics.median(arr[:reps]), 3)
    rec["ntt_ms"] = {d: {m: events(w, k) for m, k in (("lane", 1), ("wave", 2), ("library", 0))}
                     for d, w in (("forward", 0), ("inverse", 1))}
    rec["scale_ms"] = events(2, 0)
    rec["model_ms"] = round(rec["scale_ms"] / n * (n // 2) * lg, 3)
    rec["model_fraction"] = round(rec["model_ms"] / min(rec["ntt_ms"]["forward"].values()), 3)

    t0 = time.perf_counter()
    ctx.srs_lagrange(lg, fetch=False)
    rec["lagrange_ms"] = {"cold": round(1e3 * (time.perf_counter() - t0), 3),
                          "cached": round(wall(lambda: ctx.srs_lagrange(lg, fetch=False), reps), 3)}

    rnd = random.Random(lg)
    fams = {"random": lambda: rnd.randrange(K.R), "16-bit": lambda: rnd.randrange(1 << 16),
            "0/1": lambda: rnd.randrange(2)}
    rec["commit_ms"] = {}
    for name, draw in fams.items():
        dE = dev(b"".join(draw().to_bytes(32, "little") for _ in range(n)))
        a, b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        ev = wall(lambda: ok(L.kgs_commit_evals_device(ctx.handle, dE, lg, a)), reps)
        co = wall(lambda: ok(L.kgs_bench_coeff_commit(ctx.handle, dE, lg, b)), reps)
        assert a.raw == b.raw
        rec["commit_ms"][name] = {"evals": round(ev, 3), "coeff": round(co, 3)}
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.reps)), flush=True)
        return 0
    rows = []
    for lg in (int(x) for x in a.lg.split(",")):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", str(lg), "--reps", str(a.reps)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"n = 2^{lg}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:
            print(f"n = 2^{lg}: exit status {res.returncode}; stopping\n{res.stderr}", file=sys.stderr)
            return 1
        rec = json.loads(res.stdout.strip().splitlines()[-1])
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
