#!/usr/bin/env python3
"""Time the batch verifier against the single-proof verifier (DESIGN.md "Batch verifier"): batches of
1, 16, 256 and 4096 proofs made by cycling the golden proofs (tests/golden), each verified three ways
through the C-ABI with the buffers laid out beforehand:
  loop   kgs_verify proof by proof on one thread (the only way before kgs_verify_batch; measured on the
         first --loop-max proofs of the batch and scaled to its size)
  host   kgs_verify_batch with ctx == NULL
  gpu    kgs_verify_batch on a context, the fold forced onto the GPU
and a 256-proof batch with one tampered proof (bisection). Wall clock, median of --reps after a warm-up;
fold_ms / pairing_ms are the library's own (kgs_batch_diag_t).
usage: verify_batch_time.py [--sizes 1,16,256,4096] [--reps 5] [--loop-max 256] [--no-gpu] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_cases as B  # noqa: E402
import common  # noqa: E402


def wall(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=256)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K = common.load_pkg()
    L = K.lib()
    ctx = None if a.no_gpu else K.Context(0)
    ptau = "/tmp/kgs_test_oracle_p11.ptau"
    if not os.path.exists(ptau):
        if ctx is None:
            ptau = common.oracle_ptau(11)
        else:  # the product's writer gives the same bytes as the oracle's
            ctx.write_synthetic_ptau(ptau + f".{os.getpid()}", 11, common.tau())
            os.replace(ptau + f".{os.getpid()}", ptau)
    t2 = ctypes.create_string_buffer(128)
    assert L.kgs_ptau_read_tau_g2(ptau.encode(), t2) == 0
    gold = [(kind, nbits) + K._proof_buffers(kind, proof) for kind, proof, nbits in B.all_items()]
    bufs = [(ctypes.create_string_buffer(com, len(com)), ctypes.create_string_buffer(ev, len(ev)))
            for _, _, _, _, com, ev in gold]

    def refs_of(count, tamper_at=None):
        refs = (K.ProofRef * count)()
        keep = []
        for i in range(count):
            kind, nbits, npols, sel, com, ev = gold[i % len(gold)]
            cb, eb = bufs[i % len(gold)]
            if i == tamper_at:
                bad = bytearray(ev)
                bad[0] ^= 1
                eb = ctypes.create_string_buffer(bytes(bad), len(bad))
                keep.append(eb)
            refs[i] = K.ProofRef(kind, nbits, npols, int(sel), ctypes.cast(cb, ctypes.c_void_p),
                                 ctypes.cast(eb, ctypes.c_void_p))
        return refs, keep

    def batch(handle, refs, count, valid, want):
        d = K.BatchDiag()

        def call():
            rc = L.kgs_verify_batch(handle, refs, count, t2, valid, ctypes.byref(d))
            assert rc == want, (rc, L.kgs_last_error())
        ms = wall(call, a.reps)
        return {"ms": round(ms, 3), "fold_ms": round(d.fold_ms, 3), "pairing_ms": round(d.pairing_ms, 3),
                "pairing_checks": d.pairing_checks, "terms": d.terms, "on_gpu": d.on_gpu}

    rows = []
    for count in (int(x) for x in a.sizes.split(",")):
        refs, keep = refs_of(count)
        valid = ctypes.create_string_buffer(count)
        m = min(count, a.loop_max)

        def loop():
            for i in range(m):
                r = refs[i]
                assert L.kgs_verify(r.kind, r.nbits, r.npols, r.selected, r.commitments, r.evaluations, t2) == 1
        rec = {"proofs": count, "loop_measured_proofs": m, "loop_ms": round(wall(loop, 1, warmup=0) * count / m, 3)}
        os.environ["KGS_VERIFY_BATCH_FOLD"] = "host"
        rec["host"] = batch(None, refs, count, valid, 1)
        if ctx is not None:
            os.environ["KGS_VERIFY_BATCH_FOLD"] = "gpu"
            rec["gpu"] = batch(ctx.handle, refs, count, valid, 1)
            rec["loop_over_gpu"] = round(rec["loop_ms"] / rec["gpu"]["ms"], 2)
        rec["loop_over_host"] = round(rec["loop_ms"] / rec["host"]["ms"], 2)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    # one invalid proof among 256: the aggregate check fails, bisection finds it
    count, at = 256, 100
    refs, keep = refs_of(count, tamper_at=at)
    valid = ctypes.create_string_buffer(count)
    rec = {"proofs": count, "tampered": at}
    os.environ["KGS_VERIFY_BATCH_FOLD"] = "host"
    rec["host"] = batch(None, refs, count, valid, 0)
    assert [i for i in range(count) if valid.raw[i] == 0] == [at]
    if ctx is not None:
        os.environ["KGS_VERIFY_BATCH_FOLD"] = "gpu"
        rec["gpu"] = batch(ctx.handle, refs, count, valid, 0)
        assert [i for i in range(count) if valid.raw[i] == 0] == [at]
    rows.append(rec)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
