#!/usr/bin/env python3
"""Time kgs_kzg_recover_cosets_many against the loop of single calls it replaces, one process per n:
polys random polynomials of len = n / 2 coefficients, a random half of each one's m = n / l cosets in random order
(independent sets), or one such half shared by all (shared set); device-resident inputs. HIP events on the context's
stream (kgs_bench_kzg_recover_cosets_many), the arms alternated (many, loop, single, many, ..), median of --reps each
after a warm-up. Per (n, l, polys, sets):
  many_ms        the whole call without evaluations (what 0)
  loop_ms        the yardstick (what 4): polys runs of the single call's device work, one polynomial after the other,
                 enqueued back to back, WITHOUT the drain and the flag read a real loop of calls pays per polynomial
  single_ms      kgs_bench_kzg_recover_cosets' whole call for the last polynomial alone (what polys = 1 is held against)
  tree_ms, mside_ms, nside_ms   the legs of the many-call (what 1, 2, 3)
  loop_over_many
  claim          polys >= 4: many_ms < loop_ms;  polys = 1: many_ms <= 1.10 single_ms
The last polynomial's coefficients out of the many-call are compared with the single call's bytes and with the
polynomial itself.

Every n runs in a child process of its own under a time limit (--limit seconds); the driver starts no further child
after one that failed or timed out.
usage: kzg_recover_cosets_many_time.py [--shapes 12:6,13:6,16:6] [--polys 1,4,16,64,128] [--reps 5] [--limit 500]
                                       [--out FILE.json]"""
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


def one(lg, lb, polys_list, reps):
    import numpy as np
    import common
    import ntt_cases as T
    K = common.load_pkg()
    L = K.lib()
    n, l, m = 1 << lg, 1 << lb, 1 << (lg - lb)
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

    length = max(n // 2, 1)
    count1 = max(m // 2, (length + l - 1) // l)  # cells per polynomial
    pmax = max(polys_list)
    coefs = [T.random_elements(lg, length) if b == 0 else None for b in range(pmax)]
    rnd = np.random.Generator(np.random.PCG64(2000 + lg))
    for b in range(1, pmax):  # canonical Montgomery words: rotations of the first polynomial's elements
        a = np.frombuffer(coefs[0], dtype=np.uint8).reshape(length, 32)
        coefs[b] = np.roll(a, int(rnd.integers(1, max(length, 2))), axis=0).tobytes()
    evs = [np.frombuffer(ctx.ntt(c + bytes(32 * (n - length))), dtype=np.uint8).reshape(n, 32) for c in coefs]
    arr = (ctypes.c_double * reps)()
    med = lambda v: round(statistics.median(v), 4)
    rec = {"lg_n": lg, "lg_l": lb, "len": length, "cells_per_poly": int(count1), "reps": reps, "rows": []}
    for polys in polys_list:
        for sets in ("independent", "shared"):
            rng = np.random.Generator(np.random.PCG64(3000 + 10 * lg + polys))
            shared = rng.permutation(m)[:count1]
            index, ys = [], []
            for b in range(polys):  # grouped by ascending polynomial, as the yardstick takes them
                ix = shared if sets == "shared" else rng.permutation(m)[:count1]
                pos = ix.astype(np.int64)[:, None] + m * np.arange(l, dtype=np.int64)[None, :]
                index.append(ix.astype(np.uint64))
                ys.append(evs[b][pos.reshape(-1)].tobytes())
            count = polys * count1
            poly_of = np.repeat(np.arange(polys, dtype=np.uint32), count1)
            dP, dI, dY = dev(poly_of.tobytes()), dev(np.concatenate(index).tobytes()), dev(b"".join(ys))
            dC, dC1 = dev(bytes(32 * length * polys)), dev(bytes(32 * length))
            dI1, dY1 = dev(index[-1].tobytes()), dev(ys[-1])

            def many(what, k=1):
                ok(L.kgs_bench_kzg_recover_cosets_many(ctx.handle, lg, lb, polys, dP, dI, dY, count, length, length, dC, what,
                                                       k, arr))
                return list(arr[:k])

            def single(k=1):
                ok(L.kgs_bench_kzg_recover_cosets(ctx.handle, lg, lb, dI1, dY1, count1, length, dC1, 0, 0, k, arr))
                return list(arr[:k])

            many(0), many(4), single()  # warm-up: buffers grown, code objects loaded
            a, b, c = [], [], []
            for _ in range(reps):  # the arms alternately
                a += many(0)
                b += many(4)
                c += single()
            r = {"polys": polys, "sets": sets, "many_ms": med(a), "loop_ms": med(b), "single_ms": med(c),
                 "tree_ms": med(many(1, reps)), "mside_ms": med(many(2, reps)), "nside_ms": med(many(3, reps))}
            r["loop_over_many"] = round(r["loop_ms"] / r["many_ms"], 3)
            r["claim"] = bool(r["many_ms"] <= 1.10 * r["single_ms"]) if polys == 1 else \
                (bool(r["many_ms"] < r["loop_ms"]) if polys >= 4 else None)
            okc, st = ctx.kzg_recover_cosets_many_device(lg, lb, polys, dP, dI, dY, count, length, length, dC)
            assert okc is True and st == [1] * polys
            assert ctx.kzg_recover_cosets_device(lg, lb, dI1, dY1, count1, length, dC1) is True
            out, out1 = ctypes.create_string_buffer(32 * length * polys), ctypes.create_string_buffer(32 * length)
            assert hip.hipMemcpy(out, dC, 32 * length * polys, 2) == 0 and hip.hipMemcpy(out1, dC1, 32 * length, 2) == 0
            assert out.raw[-32 * length:] == out1.raw == coefs[polys - 1]
            r["verified"] = True
            for p in (dP, dI, dY, dC, dC1, dI1, dY1):
                hip.hipFree(p)
            rec["rows"].append(r)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="12:6,13:6,16:6", help="lg_n:lg_l, comma separated")
    ap.add_argument("--polys", default="1,4,16,64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    polys = [int(x) for x in a.polys.split(",")]
    if a.one:
        lg, lb = (int(x) for x in a.one.split(":"))
        print(json.dumps(one(lg, lb, polys, a.reps)), flush=True)
        return 0
    rows = []
    for shape in a.shapes.split(","):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", shape, "--polys", a.polys, "--reps", str(a.reps)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"shape {shape}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:
            print(f"shape {shape}: exit status {res.returncode}; stopping\n{res.stderr}", file=sys.stderr)
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
