#!/usr/bin/env python3
"""Time kgs_lookup_multiplicities_device against the lookup proof it feeds (DESIGN.md "Lookup
multiplicities"): for each shape, a uniform F (every row a random table row) and the worst case for
same-address traffic (every row of F equal to table row 0), then prove_device(K.LOOKUP) at the same
shape with the multiplicities just computed. Device-resident inputs, synthetic ptau written by the
product, torch events around each call after a warm-up, median of REPS.
usage: lookup_multiplicities_time.py [--shapes 20:1,22:4] [--reps 21] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()  # returns with the context's streams drained
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20:1,22:4")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K = bench.load_pkg()
    ctx = K.Context(0)
    rows_out = []
    for shape in a.shapes.split(","):
        nb, k = (int(x) for x in shape.split(":"))
        n = 1 << nb
        ptau = f"/tmp/kgs_bench_p{nb}.ptau"
        if not os.path.exists(ptau):
            tmp = f"{ptau}.{os.getpid()}.tmp"
            ctx.write_synthetic_ptau(tmp, nb, bench.bench_tau())
            os.replace(tmp, ptau)
        ctx.load_ptau(ptau, nb)
        rng = np.random.Generator(np.random.PCG64(nb * 100 + k))
        pick = rng.integers(0, n, size=n)
        tT, tFu, tFc = [], [], []
        for _ in range(k):
            w = rng.integers(0, np.iinfo(np.uint64).max, size=(n, 4), dtype=np.uint64, endpoint=True)
            w[:, 3] &= np.uint64((1 << 61) - 1)  # below r
            t = np.ascontiguousarray(w).view(np.uint8).reshape(n, 32)
            tT.append(torch.from_numpy(t.reshape(-1)).cuda())
            tFu.append(torch.from_numpy(t[pick].reshape(-1)).cuda())
            tFc.append(torch.from_numpy(np.tile(t[0], n)).cuda())
        sel = torch.from_numpy(np.tile(np.frombuffer(K.FR_ONE_MONT, dtype=np.uint8), n)).cuda()
        mul = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        d_t = [x.data_ptr() for x in tT]
        rec = {"nbits": nb, "npols": k, "device": torch.cuda.get_device_name(0), "reps": a.reps}
        for name, tF in (("uniform", tFu), ("all_rows_equal", tFc)):
            d_f = [x.data_ptr() for x in tF]
            med, best = timed(lambda: ctx.lookup_multiplicities_device(d_f, d_t, sel.data_ptr(), mul.data_ptr(), n),
                              a.reps)
            pmed, pbest = timed(lambda: ctx.prove_device(K.LOOKUP, nb, d_f, d_t, sel.data_ptr(), mul.data_ptr()),
                                a.reps)
            rec[name] = {"multiplicities_ms": round(med, 4), "multiplicities_min_ms": round(best, 4),
                         "prove_ms": round(pmed, 4), "prove_min_ms": round(pbest, 4), "ratio": round(med / pmed, 4)}
            print(f"n=2^{nb} k={k} {name}: multiplicities {med:.3f} ms (min {best:.3f}), "
                  f"lookup proof {pmed:.3f} ms (min {pbest:.3f}), ratio {med / pmed:.3f}", flush=True)
        rows_out.append(rec)
        del tT, tFu, tFc, sel, mul
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
