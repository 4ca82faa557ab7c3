"""The device timing helpers (kgs_bench_*) that share one event timer (context.hpp EventTimer), called through ctypes
at the smallest shapes each accepts: every legal `what` returns KGS_OK with finite positive times, leaves the context
idle, and a real call on the same context returns afterwards the bytes it returned before; one refused call per helper
(an argument check that returns before any launch) gives KGS_E_ARG and leaves the context idle and usable."""
import ctypes
import math
import os
import random

import pytest

import common
import kzg_open_cases as Z
import kzg_recover_cases as C

pytestmark = pytest.mark.gpu
KGS_OK, KGS_E_ARG = 0, -1
POWER = 6
NBITS, LBITS, POLYS, REPS = 4, 2, 3, 2
N, L_, M = 1 << NBITS, 1 << LBITS, 1 << (NBITS - LBITS)
RC_INDEX, RC_LEN = [2, 0], 2 << LBITS  # count = 2 = ceil(len / l): the fewest cosets the recovery accepts for this len

c_int, c_u64, c_vp, c_dp = ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)


class DevBuf:
    def __init__(self, hip, data):
        self.hip, self.p = hip, ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(self.p), max(len(data), 64)) == 0
        assert hip.hipMemcpy(self.p, bytes(data), len(data), 1) == 0

    def free(self):
        self.hip.hipFree(self.p)


class Env:
    """one context with an SRS, the device operands of every helper, and the real calls whose bytes must not move"""

    def __init__(self, K):
        self.K, self.L = K, K.lib()
        L = self.L
        L.kgs_bench_g1_ntt.argtypes = [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_dp]
        L.kgs_bench_kzg_open_all.argtypes = [c_vp, c_vp, c_u64, c_int, c_int, c_int, c_dp]
        L.kgs_bench_kzg_open_cosets.argtypes = [c_vp, c_vp, c_u64, c_int, c_int, c_int, c_int, c_dp]
        L.kgs_bench_kzg_open_cosets_many.argtypes = [c_vp, c_vp, c_u64, c_u64, c_u64, c_int, c_int, c_int, c_int, c_dp]
        L.kgs_bench_kzg_recover_cosets.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_u64, c_u64, c_vp, c_int, c_int,
                                                   c_int, c_dp]
        L.kgs_bench_coset_interp_fold.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_u64, c_int, c_dp]
        L.kgs_bench_ntt.argtypes = [c_vp, c_vp, c_int, c_int, c_dp]
        L.kgs_bench_msm.argtypes = [c_vp, c_vp, c_u64, c_int, c_dp]
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        hip = ctypes.CDLL(path)
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipFree.argtypes = [ctypes.c_void_p]

        self.ctx = K.Context(0)
        ptau = f"/tmp/kgs_test_timing_helpers_p{POWER}.{os.getpid()}.ptau"
        try:
            self.ctx.write_synthetic_ptau(ptau, POWER, common.tau())
            self.ctx.load_ptau(ptau, POWER)
        finally:
            if os.path.exists(ptau):
                os.remove(ptau)

        rng = random.Random(2301)
        self.coefs = [Z.mont([rng.randrange(C.R) for _ in range(N)]) for _ in range(POLYS)]
        self.index, rows, _, _ = C.case_from(RC_INDEX, NBITS, LBITS, RC_LEN, rng)
        self.ys = Z.mont(C.flat(rows))
        self.weights = Z.mont([rng.randrange(C.R) for _ in RC_INDEX])
        self.points = self.ctx.kzg_open_all(self.coefs[0], NBITS)[:128]  # two points on the curve
        idx = (ctypes.c_uint64 * len(RC_INDEX))(*RC_INDEX)
        self.bufs = {"coef": DevBuf(hip, b"".join(self.coefs)), "points": DevBuf(hip, self.points),
                     "points_out": DevBuf(hip, bytes(128)), "index": DevBuf(hip, bytes(idx)), "ys": DevBuf(hip, self.ys),
                     "weights": DevBuf(hip, self.weights), "rc_coef": DevBuf(hip, bytes(32 * RC_LEN)),
                     "fr": DevBuf(hip, self.coefs[0])}

    def d(self, name):
        return self.bufs[name].p

    def close(self):
        for b in self.bufs.values():
            b.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def env():
    e = Env(common.load_pkg())
    yield e
    e.close()


# name -> (the legal `what` values (None: the helper has no `what`), helper(env, what, reps, ms) -> rc, the real call)
def _g1_ntt(e, what, reps, ms):
    return e.L.kgs_bench_g1_ntt(e.ctx.handle, e.d("points"), e.d("points_out"), 1, what, 0, reps, ms)


def _open_all(e, what, reps, ms):
    return e.L.kgs_bench_kzg_open_all(e.ctx.handle, e.d("coef"), N, NBITS, what, reps, ms)


def _open_cosets(e, what, reps, ms):
    return e.L.kgs_bench_kzg_open_cosets(e.ctx.handle, e.d("coef"), N, NBITS, LBITS, what, reps, ms)


def _open_many(e, what, reps, ms):
    return e.L.kgs_bench_kzg_open_cosets_many(e.ctx.handle, e.d("coef"), POLYS, N, N, NBITS, LBITS, what, reps, ms)


def _recover(e, what, reps, ms):
    return e.L.kgs_bench_kzg_recover_cosets(e.ctx.handle, NBITS, LBITS, e.d("index"), e.d("ys"), len(RC_INDEX), RC_LEN,
                                            e.d("rc_coef"), what, 0, reps, ms)


def _interp_fold(e, what, reps, ms):
    return e.L.kgs_bench_coset_interp_fold(e.ctx.handle, NBITS, LBITS, e.d("index"), e.d("ys"), e.d("weights"),
                                           len(RC_INDEX), reps, ms)


HELPERS = {
    "g1_ntt": (range(3), _g1_ntt, lambda e: e.ctx.g1_ntt(e.points)),
    "kzg_open_all": (range(3), _open_all, lambda e: e.ctx.kzg_open_all(e.coefs[0], NBITS, evals=True)),
    "kzg_open_cosets": (range(6), _open_cosets, lambda e: e.ctx.kzg_open_cosets(e.coefs[0], NBITS, LBITS, evals=True)),
    "kzg_open_cosets_many": (range(6), _open_many,
                             lambda e: e.ctx.kzg_open_cosets_many(e.coefs, NBITS, LBITS, evals=True)),
    "kzg_recover_cosets": (range(4), _recover,
                           lambda e: e.ctx.kzg_recover_cosets(NBITS, LBITS, e.index, e.ys, RC_LEN, evals=True)),
    "coset_interp_fold": ([None], _interp_fold,
                          lambda e: e.ctx.coset_interp_fold(NBITS, LBITS, e.index, e.ys, e.weights)),
}
LEGS = [(name, what) for name, (whats, _, _) in HELPERS.items() for what in whats]


def timed(e, helper, what, reps=REPS):
    ms = (ctypes.c_double * max(reps, 1))(*([float("nan")] * max(reps, 1)))
    rc = helper(e, what, reps, ms)
    return rc, list(ms)


@pytest.mark.parametrize("name,what", LEGS)
def test_every_leg_times_and_leaves_the_context_as_it_was(env, name, what):
    _, helper, real = HELPERS[name]
    before = real(env)
    rc, ms = timed(env, helper, what)
    assert rc == KGS_OK, env.L.kgs_last_error().decode()
    assert all(math.isfinite(t) and t > 0 for t in ms), ms
    assert env.ctx.idle()
    assert real(env) == before and env.ctx.idle()


@pytest.mark.parametrize("name", HELPERS)
def test_a_refused_call_launches_nothing(env, name):
    """reps = 0, and where the helper has one a `what` past its table: refused on the arguments alone"""
    whats, helper, real = HELPERS[name]
    before = real(env)
    refused = [(whats[0], 0)] + ([(len(whats), REPS)] if whats[0] is not None else [])
    for what, reps in refused:
        rc, ms = timed(env, helper, what, reps)
        assert rc == KGS_E_ARG, (what, reps)
        assert all(math.isnan(t) for t in ms)  # nothing was written
        assert env.ctx.idle()
    assert real(env) == before and env.ctx.idle()


# ------------------------------------------------------------------ the two that time one interval around all reps
def test_ntt_pairs_in_one_interval(env):
    before = env.ctx.kzg_open_all(env.coefs[0], NBITS, evals=True)
    ms = ctypes.c_double(float("nan"))
    rc = env.L.kgs_bench_ntt(env.ctx.handle, env.d("fr"), NBITS, REPS, ctypes.byref(ms))
    assert rc == KGS_OK, env.L.kgs_last_error().decode()
    assert math.isfinite(ms.value) and ms.value > 0 and env.ctx.idle()
    assert env.L.kgs_bench_ntt(None, env.d("fr"), NBITS, REPS, ctypes.byref(ms)) == KGS_E_ARG
    assert env.ctx.kzg_open_all(env.coefs[0], NBITS, evals=True) == before and env.ctx.idle()


def test_msm_in_one_interval(env):
    before = env.ctx.msm(env.coefs[0])
    ms = ctypes.c_double(float("nan"))
    rc = env.L.kgs_bench_msm(env.ctx.handle, env.d("coef"), N, REPS, ctypes.byref(ms))
    assert rc == KGS_OK, env.L.kgs_last_error().decode()
    assert math.isfinite(ms.value) and ms.value > 0 and env.ctx.idle()
    assert env.L.kgs_bench_msm(None, env.d("coef"), N, REPS, ctypes.byref(ms)) == KGS_E_ARG
    assert env.ctx.msm(env.coefs[0]) == before and env.ctx.idle()
