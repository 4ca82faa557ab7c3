#!/usr/bin/env python3
"""Time kgs_kzg_open_cosets_many against `polys` back-to-back runs of kgs_kzg_open_cosets' device
work, at n = 2^lg, cosets of l = 2^lb points and polys polynomials, one process per n, over the SRS tau^i G of a
synthetic ptau and polys * n random device-resident coefficients (len = stride = n). HIP events on the context's
stream, median of --reps after a warm-up, the cached rows warm (kgs_bench_kzg_open_cosets_many). Per (n, l, polys):
  many_ms          the whole many-call (what 0)
  loop_ms          the yardstick (what 5): polys times the single call's work (kzg_open_cosets_run, the code of
                   kgs_kzg_open_cosets_device), one polynomial after the other, enqueued back to back between the
                   two events, so without the host synchronisation that each real call ends with
  fr_ms            the many-call's Fr side: layout, one batched transform, bit reversal (what 1)
  mul_sum_ms       its multiply-sum pass, polys * 2n terms, and the affine conversion (what 2)
  transforms_ms    its two batched G1 transforms and the slice (what 3)
  per_poly_ms      many_ms / polys;  loop_over_many = loop_ms / many_ms
at polys = 64 also the A/B the batched stage's mapping rests on, alternated three times in the same process:
  transforms_ms_ab, transforms_lane_ms_ab   what 3 (uniform wherever polys * G >= 64) and what 4 (per lane forced)
The last polynomial's proofs of the many-call are compared with the single call's, byte for byte, per row.

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no further
child after one that failed or timed out.
usage: kzg_open_cosets_many_time.py [--rows 12:6,13:6,16:6,12:3] [--polys 1,4,16,64,128] [--reps 5] [--limit 500]
                                    [--out FILE.json]"""
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
MAX_SLOTS = 1 << 24  # polys * n


def one(lg, lbs, polys_list, reps):
    import common
    K = common.load_pkg()
    L = K.lib()
    n = 1 << lg
    ctx = K.Context(0)
    path = f"/tmp/kgs_kzg_open_cosets_many_time_p{lg}.{os.getpid()}.ptau"
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

    def dev(size, data=None):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), size) == 0
        if data is not None:
            assert hip.hipMemcpy(p, data, size, 1) == 0
        return p

    polys_list = [p for p in polys_list if p * n <= MAX_SLOTS]
    pmax = max(polys_list)
    rnd = random.Random(lg)
    # Montgomery words of random elements below 2^253 < r: no periodic vector, whose transforms would be sparse
    coef = bytearray().join(rnd.randbytes(1 << 24) for _ in range(max(32 * pmax * n >> 24, 1)))[:32 * pmax * n]
    coef[31::32] = bytes(b & 0x1F for b in coef[31::32])
    coef = bytes(coef)
    dC = dev(len(coef), coef)
    arr = (ctypes.c_double * reps)()
    rows = []
    for lb in lbs:
        m = n >> lb
        dP, dQ = dev(64 * m * pmax), dev(64 * m)
        for polys in polys_list:
            def leg(what):
                ok(L.kgs_bench_kzg_open_cosets_many(ctx.handle, dC, polys, n, n, lg, lb, what, reps, arr))
                return round(statistics.median(arr[:reps]), 3)
            r = {"lg_n": lg, "lg_l": lb, "polys": polys, "reps": reps, "many_ms": leg(0), "loop_ms": leg(5),
                 "fr_ms": leg(1), "mul_sum_ms": leg(2), "transforms_ms": leg(3)}
            r["per_poly_ms"] = round(r["many_ms"] / polys, 3)
            r["loop_per_poly_ms"] = round(r["loop_ms"] / polys, 3)
            r["loop_over_many"] = round(r["loop_ms"] / r["many_ms"], 3)
            if polys == 64:
                a, b = [], []
                for _ in range(3):
                    leg(3)
                    a += arr[:reps]
                    leg(4)
                    b += arr[:reps]
                r["transforms_ms_ab"] = round(statistics.median(a), 3)
                r["transforms_lane_ms_ab"] = round(statistics.median(b), 3)
                r["lane_over_uniform"] = round(r["transforms_lane_ms_ab"] / r["transforms_ms_ab"], 3)
            ok(L.kgs_kzg_open_cosets_many_device(ctx.handle, dC, polys, n, n, lg, lb, dP, None))
            last = ctypes.c_void_p(dC.value + 32 * n * (polys - 1))
            ok(L.kgs_kzg_open_cosets_device(ctx.handle, last, n, lg, lb, dQ, None))
            got, want = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(64 * m)
            assert hip.hipMemcpy(got, ctypes.c_void_p(dP.value + 64 * m * (polys - 1)), 64 * m, 2) == 0
            assert hip.hipMemcpy(want, dQ, 64 * m, 2) == 0
            assert got.raw == want.raw and any(got.raw)
            r["equals_single_call"] = True
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="12:6,13:6,16:6,12:3")
    ap.add_argument("--polys", default="1,4,16,64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--lb", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    polys = [int(x) for x in a.polys.split(",")]
    if a.one:
        print(json.dumps(one(a.one, [int(x) for x in a.lb.split(",")], polys, a.reps)), flush=True)
        return 0
    by_n = {}
    for row in a.rows.split(","):
        lg, lb = (int(x) for x in row.split(":"))
        by_n.setdefault(lg, []).append(lb)
    rows = []
    for lg, lbs in by_n.items():
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", str(lg), "--lb", ",".join(map(str, lbs)), "--polys", a.polys,
            "--reps", str(a.reps)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"n = 2^{lg}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:
            print(f"n = 2^{lg}: exit status {res.returncode}; stopping", file=sys.stderr)
            return 1
        rows += json.loads(res.stdout.strip().splitlines()[-1])
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
    print(json.dumps(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
