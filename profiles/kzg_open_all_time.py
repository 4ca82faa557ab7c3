#!/usr/bin/env python3
"""Time kgs_kzg_open_all at n = 2^lg, one process per n, over the SRS tau^i G of a synthetic
ptau and n random device-resident coefficients. HIP events on the context's stream, median of --reps after
a warm-up, unless stated:
  open_all_ms     (a) kgs_kzg_open_all_device with the cached SRS side warm (kgs_bench_kzg_open_all, what 0)
  build_ms        (b) the build of the cached SRS side: one scaled forward G1 transform of 2n points (what 1)
  pointwise_ms    (c) the pointwise pass alone: 2n per-lane multiplications and their affine conversion (what 2)
  uniform_2n_ms   2n multiplications by one launch-uniform constant (kgs_bench_g1_ntt, what 2): the rate (c) is
                  held against; pointwise_over_uniform = (c) / that, derived bound 1.5
  transforms_ms   (d) the two G1 transforms alone, unscaled (kgs_bench_g1_ntt, what 0): size 2n, size n, sum
  single_ms       (e) kgs_kzg_open, wall clock of the whole call (host coefficients, ends synchronised), median
                  over 64 random points; single_times_n_ms = that times n is an EXTRAPOLATION, not a run
  ratios          (a) / (e extrapolated), (a) / (d), ((a) - (d)) / (c)
The proofs of one call are checked: 4 sampled entries equal kgs_kzg_open's proof at that point.

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no
further child after one that failed or timed out.
usage: kzg_open_all_time.py [--lg 12,16,20] [--reps 5] [--limit 500] [--out FILE.json]"""
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


def one(lg, reps):
    import common
    K = common.load_pkg()
    L = K.lib()
    L.kgs_bench_g1_ntt.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.kgs_bench_kzg_open_all.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    n = 1 << lg
    ctx = K.Context(0)
    path = f"/tmp/kgs_kzg_open_all_time_p{lg}.{os.getpid()}.ptau"
    try:
        ctx.write_synthetic_ptau(path, lg, common.tau())
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

    rnd = random.Random(lg)
    coef = b"".join(rnd.randrange(K.R).to_bytes(32, "little") for _ in range(n))  # Montgomery words of random elements
    dC, dP = dev(coef), dev(bytes(64 * n))
    arr = (ctypes.c_double * reps)()
    rec = {"lg_n": lg, "reps": reps}

    def leg(what):
        ok(L.kgs_bench_kzg_open_all(ctx.handle, dC, n, lg, what, reps, arr))
        return round(statistics.median(arr[:reps]), 3)
    rec["open_all_ms"] = leg(0)
    rec["build_ms"] = leg(1)
    rec["pointwise_ms"] = leg(2)

    # the transforms and the uniform multiplication on their own, over the proofs of two polynomials as
    # input points (2n points of period n would transform to identities at every odd index, and a stage
    # skips the multiplication of an identity)
    proofs = ctypes.create_string_buffer(64 * n)
    other = ctypes.create_string_buffer(64 * n)
    ok(L.kgs_kzg_open_all_device(ctx.handle, dC, n // 2 + 1, lg, dP, None))
    assert hip.hipMemcpy(other, dP, 64 * n, 2) == 0
    ok(L.kgs_kzg_open_all_device(ctx.handle, dC, n, lg, dP, None))
    assert hip.hipMemcpy(proofs, dP, 64 * n, 2) == 0
    dI, dO = dev(proofs.raw + other.raw), dev(bytes(128 * n))

    def events(logm, what):
        ok(L.kgs_bench_g1_ntt(ctx.handle, dI, dO, logm, what, 0, reps, arr))
        return round(statistics.median(arr[:reps]), 3)
    rec["uniform_2n_ms"] = events(lg + 1, 2)
    t2n, tn = events(lg + 1, 0), events(lg, 0)
    rec["transforms_ms"] = {"2n": t2n, "n": tn, "sum": round(t2n + tn, 3)}

    ms = []
    for i in range(-1, 64):  # -1: warm-up
        z = rnd.randrange(K.R).to_bytes(32, "little")
        t0 = time.perf_counter()
        ctx.kzg_open(coef, z)
        if i >= 0:
            ms.append(1e3 * (time.perf_counter() - t0))
    rec["single_ms"] = round(statistics.median(ms), 3)
    rec["single_times_n_ms"] = round(rec["single_ms"] * n, 1)
    rec["single_times_n_is"] = "an extrapolation: 64 openings timed, multiplied out to n"
    w = common.bn.FR_W[lg]
    for i in (0, 1, n // 2 + 1, n - 1):
        z = (pow(w, i, K.R) * (1 << 256) % K.R).to_bytes(32, "little")
        assert ctx.kzg_open(coef, z)[1] == proofs.raw[64 * i:64 * i + 64], i
    d = rec["transforms_ms"]["sum"]
    rec["ratios"] = {"open_all_over_single_times_n": round(rec["open_all_ms"] / rec["single_times_n_ms"], 6),
                     "open_all_over_transforms": round(rec["open_all_ms"] / d, 3),
                     "excess_over_pointwise": round((rec["open_all_ms"] - d) / rec["pointwise_ms"], 3),
                     "pointwise_over_uniform": round(rec["pointwise_ms"] / rec["uniform_2n_ms"], 3)}
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", default="12,16,20")
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
