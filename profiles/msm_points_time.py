#!/usr/bin/env python3
"""Time the variable-base MSM (kgs_msm_points) over n arbitrary bases with uniform random
scalars, host buffers in, one process per n:
  (a) old_route_ms   what the addon's msmPoints did before kgs_msm_points existed, through the public
                     C-ABI on a scratch context: kgs_srs_load_points + kgs_fr_to_mont + kgs_msm
  (b) msm_points_ms  kgs_msm_points with window_c = 0
  (c) fixed_base_ms  kgs_msm over window tables already resident for the same points (the floor)
and (b) again at every window_c of --sweep. msm_points_device_ms is (b) through kgs_msm_points_device,
points and scalars resident on the device: (b) without its two host-to-device copies. Wall clock,
median of --reps after a warm-up. The routes' results are compared byte for byte.

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no
further child after one that failed or timed out.
usage: msm_points_time.py [--lg 12,16,20] [--sweep 16,20] [--reps 7] [--limit 400] [--out FILE.json]"""
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


def one(lg, reps, sweep):
    import common
    from oracle import ptau as opt
    K = common.load_pkg()
    L = K.lib()
    n = 1 << lg
    ctx = K.Context(0)
    path = f"/tmp/kgs_msm_points_time_p{lg}.{os.getpid()}.ptau"
    try:
        ctx.write_synthetic_ptau(path, lg, common.tau())
        pts = opt.PTau(path).g1_bytes[:64 * n]
    finally:
        if os.path.exists(path):
            os.remove(path)
    rnd = random.Random(lg)
    std = b"".join(rnd.randrange(K.R).to_bytes(32, "little") for _ in range(n))
    P = ctypes.create_string_buffer(pts, len(pts))
    S = ctypes.create_string_buffer(std, len(std))
    mont = ctypes.create_string_buffer(len(std))
    out = {k: ctypes.create_string_buffer(64) for k in "abc"}

    def ok(rc):
        assert rc == 0, L.kgs_last_error().decode()

    scratch = K.Context(0)

    def old_route():
        ok(L.kgs_srs_load_points(scratch.handle, P, n, lg - 1, lg - 1))
        ok(L.kgs_fr_to_mont(scratch.handle, S, mont, n))
        ok(L.kgs_msm(scratch.handle, mont, n, out["a"]))

    def new_call(c=0):
        ok(L.kgs_msm_points(ctx.handle, P, S, n, c, out["b"]))

    def floor():
        ok(L.kgs_msm(scratch.handle, mont, n, out["c"]))
    rec = {"lg_n": lg, "auto_window": min(max(lg - 4, 7), 16)}
    rec["old_route_ms"] = round(wall(old_route, reps), 3)
    rec["fixed_base_ms"] = round(wall(floor, reps), 3)  # the tables of the last old_route() are resident
    rec["fixed_base_window"] = scratch.srs_info()[2]
    rec["msm_points_ms"] = round(wall(new_call, reps), 3)
    assert out["a"].raw == out["b"].raw == out["c"].raw
    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    dP, dS, od = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.create_string_buffer(64)
    assert hip.hipMalloc(ctypes.byref(dP), len(pts)) == 0 and hip.hipMalloc(ctypes.byref(dS), len(std)) == 0
    assert hip.hipMemcpy(dP, P, len(pts), 1) == 0 and hip.hipMemcpy(dS, S, len(std), 1) == 0
    rec["msm_points_device_ms"] = round(wall(lambda: ok(L.kgs_msm_points_device(ctx.handle, dP, dS, n, 0, od)), reps), 3)
    assert od.raw == out["a"].raw
    if sweep:
        rec["sweep_ms"] = {}
        for c in range(7, 17):
            rec["sweep_ms"][str(c)] = round(wall(lambda: new_call(c), reps), 3)
            assert out["b"].raw == out["a"].raw
    rec["old_over_new"] = round(rec["old_route_ms"] / rec["msm_points_ms"], 2)
    rec["new_over_floor"] = round(rec["msm_points_ms"] / rec["fixed_base_ms"], 2)
    scratch.close()
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", default="12,16,20")
    ap.add_argument("--sweep", default="16,20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=400)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--with-sweep", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.reps, a.with_sweep)), flush=True)
        return 0
    sweep = {int(x) for x in a.sweep.split(",") if x}
    rows = []
    for lg in (int(x) for x in a.lg.split(",")):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", str(lg), "--reps", str(a.reps)] + (["--with-sweep"] if lg in sweep else [])
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
