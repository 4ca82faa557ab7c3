#!/usr/bin/env python3
"""Time kgs_kzg_verify_cosets_batch on one MI355X. The openings are those of one random polynomial
at n = 2^lg with cosets of l = 2^lb points, made by kgs_kzg_open_cosets_device over the SRS tau^i G of a synthetic
ptau; a batch is the first `count` cosets, count in 1, 16, 256, 4096 and all m = n / l. C-ABI calls on buffers laid
out beforehand, wall clock, median of --reps after a warm-up, unless stated:
  loop_ms          kgs_kzg_verify_coset per opening, timed ONCE on min(count, --loop-max) openings and SCALED to count
                   (loop_timed says on how many)
  host_ms          the batch with ctx == NULL, derived seed; host_hash_ms / host_fold_ms / host_pairing_ms its diag
  gpu_ms           the batch on a context, host buffers, derived seed, KGS_VERIFY_COSETS_FOLD=gpu; gpu_hash_ms /
                   gpu_fold_ms / gpu_pairing_ms its diag (fold: uploads, structural checks, weights, D, the terms,
                   the two point sums, downloads)
  gpu_seed_ms      the same with a caller's seed (nothing hashed)
  gpu_device_ms    kgs_kzg_verify_cosets_batch_device: commit_of, index, values and proofs resident, caller's seed
  kernel_ms        k_coset_interp_fold and the reduction of its partials alone, HIP events (kgs_bench_coset_interp_fold;
                   lb <= 10), kernel_GBps = count * l * 32 B / kernel_ms
  gpu_fold_ms_route_fold / _points   fold_ms of the GPU batch (caller's seed) with KGS_VERIFY_COSETS_MSM forcing
                   kgs_g1_lincomb's fold (up to 4096 terms) or kgs_msm_points' buckets for A and B; terms = 3 count + l
  tampered_ms, tampered_checks   the GPU batch with one opening's proof exchanged, valid_out wanted, ONE run
Every (lg, lb) runs in a child process of its own under a time limit; the driver starts no further child after one
that failed or timed out.
usage: kzg_verify_cosets_batch_time.py [--cases 8:0,8:3,20:6,20:10,16:6] [--reps 5] [--loop-max 16] [--limit 500] [--out FILE.json]"""
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


def one(lg, lb, reps, loop_max):
    import numpy as np
    import common
    import g1_ntt_cases as N
    import kzg_coset_cases as C
    os.environ["KGS_VERIFY_COSETS_FOLD"] = "gpu"
    K = common.load_pkg()
    L = K.lib()
    L.kgs_bench_coset_interp_fold.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_double)]
    n, l, m = 1 << lg, 1 << lb, 1 << (lg - lb)
    ctx = K.Context(0)
    path = f"/tmp/kgs_kzg_verify_cosets_batch_time_p{lg}.{os.getpid()}.ptau"
    try:
        ctx.write_synthetic_ptau(path, lg, common.tau())
        ctx.load_ptau(path, lg)
    finally:
        if os.path.exists(path):
            os.remove(path)

    def ok(rc):
        assert rc >= 0, L.kgs_last_error().decode()
        return rc

    hip = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def dev(data):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(len(data), 64)) == 0 and hip.hipMemcpy(p, data, len(data), 1) == 0
        return p

    rnd = random.Random(lg * 100 + lb)
    coef = b"".join(rnd.randrange(K.R).to_bytes(32, "little") for _ in range(n))  # Montgomery words of random elements
    rinv = pow(1 << 256, K.R - 2, K.R)
    c_int = [int.from_bytes(coef[i:i + 32], "little") * rinv % K.R for i in range(0, len(coef), 32)]
    commit = N.point(sum(c * t for c, t in zip(c_int, N.tau_powers(n))) % K.R)
    dC, dP, dE = dev(coef), dev(bytes(64 * m)), dev(bytes(32 * n))
    ok(L.kgs_kzg_open_cosets_device(ctx.handle, dC, n, lg, lb, dP, dE))
    pr, ev = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(32 * n)
    assert hip.hipMemcpy(pr, dP, 64 * m, 2) == 0 and hip.hipMemcpy(ev, dE, 32 * n, 2) == 0
    # row i of the batch: the values e[i + m j], j < l
    ys = np.frombuffer(ev.raw, dtype=np.uint8).reshape(l, m, 32).transpose(1, 0, 2).tobytes()
    proofs = pr.raw
    t2 = C.tau_l_g2(lb)
    # the first l points tau^k G of the ptau's SRS, through the library (l oracle products are slow at l = 1024)
    srs = ctx.g1_mul_each(N.point(1) * l, N.scalar_bytes(N.tau_powers(l)))
    commit_of = (ctypes.c_uint32 * m)()
    index = (ctypes.c_uint64 * m)(*range(m))
    d_cof, d_idx, d_ys, d_pr = dev(bytes(commit_of)), dev(bytes(index)), dev(ys), dP
    d_w = dev(b"".join(rnd.randrange(K.R).to_bytes(32, "little") for _ in range(m)))
    seed = bytes(range(32))
    cb, yb, pb, sb = (ctypes.create_string_buffer(x, len(x)) for x in (commit, ys, proofs, srs))
    void = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def batch(handle, count, seed32, valid=None, device=False, proofs_buf=pb):
        d = K.CosetBatchDiag()
        t0 = time.perf_counter()
        if device:
            rc = L.kgs_kzg_verify_cosets_batch_device(handle, lg, lb, cb, 1, d_cof, d_idx, d_ys, d_pr, count, sb, t2,
                                                      seed32, valid, ctypes.byref(d))
        else:
            rc = L.kgs_kzg_verify_cosets_batch(handle, lg, lb, cb, 1, void(commit_of), void(index), yb, proofs_buf,
                                               count, sb, t2, seed32, valid, ctypes.byref(d))
        return ok(rc), (time.perf_counter() - t0) * 1e3, d

    def med(fn):
        fn()
        runs = [fn() for _ in range(reps)]
        k = sorted(range(reps), key=lambda i: runs[i][1])[reps // 2]
        assert all(r[0] == 1 for r in runs)
        return runs[k]

    rows = []
    for count in sorted({min(c, m) for c in (1, 16, 256, 4096, m)}):
        r = {"count": count, "terms": 3 * count + l}
        k = min(count, loop_max)
        L.kgs_kzg_verify_coset(cb, lg, lb, 0, yb, pb, sb, t2)  # warm-up
        t0 = time.perf_counter()
        for i in range(k):
            assert L.kgs_kzg_verify_coset(cb, lg, lb, i, ctypes.byref(yb, 32 * l * i), ctypes.byref(pb, 64 * i), sb, t2) == 1
        r["loop_timed"], r["loop_ms"] = k, round((time.perf_counter() - t0) * 1e3 / k * count, 2)
        for name, handle, s32, device in (("host", None, None, False), ("gpu", ctx.handle, None, False),
                                          ("gpu_seed", ctx.handle, seed, False), ("gpu_device", ctx.handle, seed, True)):
            _, ms, d = med(lambda: batch(handle, count, s32, device=device))
            assert d.on_gpu == (0 if handle is None else 1) and d.pairing_checks == 1
            r[name + "_ms"] = round(ms, 3)
            if name in ("host", "gpu"):
                r.update({f"{name}_hash_ms": round(d.hash_ms, 3), f"{name}_fold_ms": round(d.fold_ms, 3),
                          f"{name}_pairing_ms": round(d.pairing_ms, 3)})
        for route in ("fold", "points"):  # the two routes of the point sums, forced: where the switch belongs
            if route == "fold" and 3 * count + l > 4096:
                continue  # one thread sums a whole segment: not a candidate there
            os.environ["KGS_VERIFY_COSETS_MSM"] = route
            _, ms, d = med(lambda: batch(ctx.handle, count, seed))
            r[f"gpu_fold_ms_route_{route}"] = round(d.fold_ms, 3)
        del os.environ["KGS_VERIFY_COSETS_MSM"]
        if lb <= 10:
            arr = (ctypes.c_double * reps)()
            ok(L.kgs_bench_coset_interp_fold(ctx.handle, lg, lb, d_idx, d_ys, d_w, count, reps, arr))
            r["kernel_ms"] = round(statistics.median(arr[:reps]), 4)
            r["kernel_GBps"] = round(count * l * 32 / (r["kernel_ms"] * 1e-3) / 1e9, 1)
        if count > 1:
            bad = bytearray(proofs)
            j = count // 3
            bad[64 * j:64 * j + 64] = proofs[64 * (j + 1):64 * (j + 2)]
            bb = ctypes.create_string_buffer(bytes(bad), len(bad))
            valid = ctypes.create_string_buffer(count)
            rc, ms, d = batch(ctx.handle, count, None, valid=valid, proofs_buf=bb)
            assert rc == 0 and [i for i in range(count) if valid.raw[i] == 0] == [j]
            r["tampered_ms"], r["tampered_checks"] = round(ms, 2), d.pairing_checks
        rows.append(r)
    ctx.close()
    return {"lg_n": lg, "lg_l": lb, "m": m, "reps": reps, "counts": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8:0,8:3,20:6,20:10,16:6")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=16)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_verify_cosets_batch_time.json"))
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        lg, lb = (int(x) for x in a.one.split(":"))
        print(json.dumps(one(lg, lb, a.reps, a.loop_max)), flush=True)
        return 0
    rows = []
    for case in a.cases.split(","):
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            os.path.abspath(__file__), "--one", case, "--reps", str(a.reps), "--loop-max", str(a.loop_max)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:
            print(f"{case}: exit status {res.returncode}; stopping\n{res.stderr}", file=sys.stderr)
            return 1
        rec = json.loads(res.stdout.strip().splitlines()[-1])
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
