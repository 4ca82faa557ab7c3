#!/usr/bin/env python3
"""Time the multi-argument prover against the single prover: m unselected k = 1 grand-sums
at n = 2^nbits, inputs resident on the device, one context. For every m one kgs_prove_multi_device call is
timed against m back-to-back kgs_prove_device calls (the single prover as it is: the baseline) in the same
process. Wall clock, median of --reps after a warm-up; rounds_ms is kgs_last_timing's per-round split of
the last multi proof and of the last single proof.

Every m runs in a child process of its own under a time limit (--limit seconds); the driver starts no
further child after one that failed or timed out.
usage: multi_time.py [--nbits 20] [--m 1,2,4,8] [--reps 7] [--limit 240] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
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


def one(m, nbits, reps):
    import common
    from test_gpu_configs import gpu_ptau, np_inputs
    K = common.load_pkg()
    ctx = K.Context(0)
    ctx.load_ptau(gpu_ptau(K, nbits), nbits)
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def up(b):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), len(b)) == 0
        assert hip.hipMemcpy(p, b, len(b), 1) == 0
        return p.value
    dev = []
    for j in range(m):
        Fs, Ts, _, _ = np_inputs(9000 + j, nbits, 1, False)
        dev.append((up(Fs[0]), up(Ts[0])))
    args = [(K.GRANDSUM, [f], [t], None, None) for f, t in dev]
    proof = [None]

    def multi():
        proof[0] = ctx.prove_multi_device(nbits, args)

    def singles():
        for f, t in dev:
            ctx.prove_device(K.GRANDSUM, nbits, [f], [t])
    multi_ms = wall(multi, reps)
    multi_rounds = ctx.last_timing()[:5]
    singles_ms = wall(singles, reps)
    single_rounds = ctx.last_timing()[:5]
    # the timed proof is a valid one
    shapes = (K.ArgShape * m)(*[K.ArgShape(K.GRANDSUM, 1, 0)] * m)
    t2 = ctypes.create_string_buffer(128)
    assert K.lib().kgs_ptau_read_tau_g2(os.fsencode(gpu_ptau(K, nbits)), t2) == 0
    com, ev = b"".join(proof[0][0]), b"".join(proof[0][1])
    assert K.lib().kgs_verify_multi(nbits, shapes, m, K._buf(com), K._buf(ev), t2) == 1
    ctx.close()
    return {"m": m, "nbits": nbits, "multi_ms": round(multi_ms, 3), "singles_ms": round(singles_ms, 3),
            "ratio": round(singles_ms / multi_ms, 3), "predicted_ratio": round(8 * m / (3 * m + 5), 3),
            "multi_rounds_ms": [round(x, 3) for x in multi_rounds],
            "single_rounds_ms": [round(x, 3) for x in single_rounds],
            "proof_bytes": len(com) + len(ev), "singles_proof_bytes": m * (64 * 6 + 32 * 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbits", type=int, default=20)
    ap.add_argument("--m", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.nbits, a.reps)), flush=True)
        return 0
    rows = []
    for m in (int(x) for x in a.m.split(",")):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", str(m), "--nbits", str(a.nbits), "--reps", str(a.reps)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"m = {m}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(f"m = {m}: exit status {out.returncode}; stopping\n{out.stderr}", file=sys.stderr)
            return 1
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        assert rec["proof_bytes"] == 64 * (3 * m + 3) + 32 * (2 * m + m)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
