#!/usr/bin/env python3
"""Time kgs_kzg_open_cosets at n = 2^lg and cosets of l = 2^lb points, one process per n, over the
SRS tau^i G of a synthetic ptau and n random device-resident coefficients (len = n). HIP events on the context's
stream, median of --reps after a warm-up (kgs_bench_kzg_open_cosets / kgs_bench_kzg_open_all):
  open_all_ms      kgs_kzg_open_all_device at the same n, cache warm, IN THIS RUN: what the coset calls are
                   held against. l = 1 is that call (kgs_kzg_open_cosets with lbits = 0 runs the same code).
  open_all_build_ms, open_all_pointwise_ms   §19's (b) and (c) at the same n, in this run
per l >= 2 (1 <= lb < lg):
  call_ms          (a) the whole call with the cached rows warm (what 0)
  build_ms         (b) the build of the cached rows: log2(2m) of the log2(2n) stages of one transform of 2n
                   points, then the scaling pass (what 1); stage_fraction = log2(2m) / log2(2n)
  mul_sum_ms       (c) the multiply-sum pass alone: 2n products, the column sums, 2m affine conversions (what 2)
  mul_each_ms      k_g1_mul_each over the same 2n terms, nothing else (what 4)
  mul_sum_l1_ms    the pass with one row per lane, k_g1_mul_each and then the column sums (what 5): the other
                   arm of §20's A/B, here once per (n, l), not alternated
  transforms_ms    (d) the inverse G1 transform of size 2m and the forward one of size m, over the call's own u
                   and h (what 3): points of this polynomial, no periodic vector
  ratios           (a) / open_all, (b) / open_all_build, (c) / mul_each, (one row per lane) / mul_each,
                   ((a) - (d)) / (c)
One proof per (n, l) is checked with kgs_kzg_verify_coset.

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no further
child after one that failed or timed out.
usage: kzg_open_cosets_time.py [--lg 12,16,20] [--lb 3,6,10] [--reps 5] [--limit 500] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one(lg, lbs, reps):
    import common
    import g1_ntt_cases as N
    import kzg_coset_cases as C
    K = common.load_pkg()
    L = K.lib()
    L.kgs_bench_kzg_open_all.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.kgs_bench_kzg_open_cosets.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    n = 1 << lg
    ctx = K.Context(0)
    path = f"/tmp/kgs_kzg_open_cosets_time_p{lg}.{os.getpid()}.ptau"
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
    dC, dP, dE = dev(coef), dev(bytes(64 * n)), dev(bytes(32 * n))
    arr = (ctypes.c_double * reps)()
    rec = {"lg_n": lg, "reps": reps}

    def leg_all(what):
        ok(L.kgs_bench_kzg_open_all(ctx.handle, dC, n, lg, what, reps, arr))
        return round(statistics.median(arr[:reps]), 3)
    rec["open_all_ms"] = leg_all(0)
    rec["open_all_build_ms"] = leg_all(1)
    rec["open_all_pointwise_ms"] = leg_all(2)
    rec["cosets"] = []
    rinv = pow(1 << 256, K.R - 2, K.R)
    c_int = [int.from_bytes(coef[i:i + 32], "little") * rinv % K.R for i in range(0, len(coef), 32)]
    commit = N.point(sum(c * t for c, t in zip(c_int, N.tau_powers(n))) % K.R) if lg <= 20 else None
    for lb in lbs:
        if not 1 <= lb < lg:
            continue

        def leg(what):
            ok(L.kgs_bench_kzg_open_cosets(ctx.handle, dC, n, lg, lb, what, reps, arr))
            return round(statistics.median(arr[:reps]), 3)
        r = {"lg_l": lb, "call_ms": leg(0), "build_ms": leg(1), "mul_sum_ms": leg(2), "mul_each_ms": leg(4),
             "mul_sum_l1_ms": leg(5),
             "transforms_ms": leg(3), "stage_fraction": round((lg - lb + 1) / (lg + 1), 3)}
        r["ratios"] = {"call_over_open_all": round(r["call_ms"] / rec["open_all_ms"], 4),
                       "build_over_open_all_build": round(r["build_ms"] / rec["open_all_build_ms"], 4),
                       "mul_sum_over_mul_each": round(r["mul_sum_ms"] / r["mul_each_ms"], 4),
                       "mul_sum_l1_over_mul_each": round(r["mul_sum_l1_ms"] / r["mul_each_ms"], 4),
                       "excess_over_mul_sum": round((r["call_ms"] - r["transforms_ms"]) / r["mul_sum_ms"], 3)}
        if commit is not None:  # one proof through the host check (the commitment costs n oracle products: n <= 2^20)
            m, l, i = n >> lb, 1 << lb, 1
            ok(L.kgs_kzg_open_cosets_device(ctx.handle, dC, n, lg, lb, dP, dE))
            pr, ev = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(32 * n)
            assert hip.hipMemcpy(pr, dP, 64 * m, 2) == 0 and hip.hipMemcpy(ev, dE, 32 * n, 2) == 0
            ys = b"".join(ev.raw[32 * (i + m * j):32 * (i + m * j) + 32] for j in range(l))
            assert K.kzg_verify_coset(C.tau_l_g2(lb), C.srs_g1(lb), commit, lg, lb, i, ys, pr.raw[64 * i:64 * i + 64])
            r["verified"] = True
        rec["cosets"].append(r)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", default="12,16,20")
    ap.add_argument("--lb", default="3,6,10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    lbs = [int(x) for x in a.lb.split(",")]
    if a.one:
        print(json.dumps(one(a.one, lbs, a.reps)), flush=True)
        return 0
    rows = []
    for lg in (int(x) for x in a.lg.split(",")):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", str(lg), "--lb", a.lb, "--reps", str(a.reps)]
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
