#!/usr/bin/env python3
"""Time kgs_kzg_recover_cosets at n = 2^lg and cosets of l = 2^lb points, one process per n: a
random polynomial of len = n / 2 coefficients, a random half of its m = n / l cosets in random order, device-resident
inputs. HIP events on the context's stream, median of --reps after a warm-up (kgs_bench_kzg_recover_cosets).
Per (n, l):
  call_ms        the whole call without evaluations (what 0)
  tree_ms        the marks and the product tree (what 1)
  mside_ms       z's coefficients, its two transforms of size m, the batch inversion (what 2)
  nside_ms       the call's three transforms of size n alone, IN THIS RUN (what 3): what the call is held against
  call_over_nside
  leaf           the leaf size the library uses (2^leaf_log slots) and one alternative, the tree leg measured with
                 the two alternately (A B A B ..), median each
The recovered coefficients are compared with the polynomial's bytes.

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no further
child after one that failed or timed out.
usage: kzg_recover_cosets_time.py [--lg 16,20] [--lb 0,6,10] [--reps 5] [--alt-leaf 8] [--limit 500] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one(lg, lbs, reps, alt_leaf):
    import numpy as np
    import common
    import ntt_cases as T
    K = common.load_pkg()
    L = K.lib()
    n = 1 << lg
    ctx = K.Context(0)

    def ok(rc):
        assert rc == 0, L.kgs_last_error().decode()

    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]

    def dev(data):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(len(data), 64)) == 0 and hip.hipMemcpy(p, data, len(data), 1) == 0
        return p

    import re
    src = open(os.path.join(ROOT, "kzg-grandsums-study_amd", "csrc", "kernels.hpp")).read()
    leaf_log = int(re.search(r"RC_LEAF_LOG = (\d+)", src).group(1))
    length = max(n // 2, 1)
    coef = T.random_elements(lg, length)  # canonical Montgomery words
    ev = np.frombuffer(ctx.ntt(coef + bytes(32 * (n - length))), dtype=np.uint8).reshape(n, 32)
    rng = np.random.Generator(np.random.PCG64(1000 + lg))
    arr = (ctypes.c_double * (2 * reps))()
    rec = {"lg_n": lg, "len": length, "reps": reps, "rows": []}
    for lb in lbs:
        if not 0 <= lb <= lg:
            continue
        l, m = 1 << lb, n >> lb
        count = max(m // 2, (length + l - 1) // l)
        index = rng.permutation(m)[:count].astype(np.uint64)
        pos = index.astype(np.int64)[:, None] + m * np.arange(l, dtype=np.int64)[None, :]
        ys = ev[pos.reshape(-1)].tobytes()
        dI, dY, dC = dev(index.tobytes()), dev(ys), dev(bytes(32 * length))

        def leg(what, leaf=0, k=reps):
            ok(L.kgs_bench_kzg_recover_cosets(ctx.handle, lg, lb, dI, dY, count, length, dC, what, leaf, k, arr))
            return list(arr[:k])
        med = lambda v: round(statistics.median(v), 4)
        r = {"lg_l": lb, "count": int(count), "call_ms": med(leg(0)), "tree_ms": med(leg(1)), "mside_ms": med(leg(2)),
             "nside_ms": med(leg(3))}
        r["call_over_nside"] = round(r["call_ms"] / r["nside_ms"], 3)
        a, b = [], []
        for _ in range(reps):  # the two leaf sizes alternately
            a += leg(1, 0, 1)
            b += leg(1, alt_leaf, 1)
        r["leaf"] = {"leaf_log": leaf_log, "tree_ms": med(a), "alt_leaf_log": alt_leaf, "alt_tree_ms": med(b)}
        out = ctypes.create_string_buffer(32 * length)
        assert ctx.kzg_recover_cosets_device(lg, lb, dI, dY, count, length, dC) is True
        assert hip.hipMemcpy(out, dC, 32 * length, 2) == 0 and out.raw == coef
        r["verified"] = True
        for p in (dI, dY, dC):
            hip.hipFree(p)
        rec["rows"].append(r)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", default="16,20")
    ap.add_argument("--lb", default="0,6,10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alt-leaf", type=int, default=8)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    lbs = [int(x) for x in a.lb.split(",")]
    if a.one:
        print(json.dumps(one(a.one, lbs, a.reps, a.alt_leaf)), flush=True)
        return 0
    rows = []
    for lg in (int(x) for x in a.lg.split(",")):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", str(lg), "--lb", a.lb, "--reps", str(a.reps), "--alt-leaf", str(a.alt_leaf)]
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
