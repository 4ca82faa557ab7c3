"""Variable-base MSM on the GPU (kgs_msm_points, kgs_msm_points_device): byte for byte against the closed
form over the bases tau^i G at every window the sort takes another path for, the edges of the
signed-digit recoding, skewed and cancelling inputs, scalars above r, the fixed-base MSM over the same
points, and the context contract (the resident SRS, its MSM and a proof are untouched; the context is
idle after a successful and after a failing call)."""
import ctypes
import os

import pytest

import common
import degenerate_cases as D
import msm_points_cases as M
from oracle import ptau as opt

pytestmark = pytest.mark.gpu
R = M.R
KGS_E_ARG = -1
POWER = 16  # 2^17 - 1 points tau^i G
BIG = 1 << 16


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ctx(K):
    c = K.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases(ctx):
    """the points tau^i G (common.tau()), written by the GPU writer into a file of the module's own"""
    path = f"/tmp/kgs_test_msm_points_p{POWER}.{os.getpid()}.ptau"
    try:
        ctx.write_synthetic_ptau(path, POWER, common.tau())
        return opt.PTau(path).g1_bytes
    finally:
        if os.path.exists(path):
            os.remove(path)


@pytest.fixture(scope="module")
def rand_big():
    s = D.random_scalars(BIG, 4242)
    return s, M.scalar_bytes(s), M.closed_form(s)


def run(ctx, points, scalars, c=0):
    return ctx.msm_points(points, M.scalar_bytes(scalars), window_c=c)


# ------------------------------------------------------------------ shapes x windows
@pytest.mark.parametrize("c", M.WINDOWS)
@pytest.mark.parametrize("n", [1, 2, 3, 17, 255, 256, 257, 513, 4097])
def test_shapes(ctx, bases, n, c):
    """one scalar to several blocks of the sort passes (512 scalars each), around the 256-thread block,
    at every window: c = 16 uses the whole 2^19 key space and the 2048-partition sort already at n = 1"""
    s = D.random_scalars(n, 31 * n + c)
    assert run(ctx, bases[:64 * n], s, c) == M.closed_form(s)


@pytest.mark.parametrize("c", M.WINDOWS)
def test_digit_edges(ctx, bases, c):
    n = 257
    for what, s in M.digit_edge_scalars(c or M.auto_window(n)):
        v = [s] * n
        want = M.closed_form(v)
        if what == "zero":
            assert want == bytes(64)
        assert run(ctx, bases[:64 * n], v, c) == want, what
        # and among random scalars
        v = D.random_scalars(n, 11)
        v[0] = v[100] = v[256] = s
        assert run(ctx, bases[:64 * n], v, c) == M.closed_form(v), what


# ------------------------------------------------------------------ skew and cancellation
def test_all_scalars_equal_2p16(ctx, bases):
    """65,536 entries in one bucket per window: thousands of segment partials per bucket, all three
    combine levels"""
    s = D.random_scalars(1, 99) * BIG
    assert run(ctx, bases[:64 * BIG], s) == M.closed_form(s)


@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_bases(ctx, name):
    """all points equal, P / -P alternating, a 4-cycle, G then zero points: equal and opposite points
    meet inside the bucket runs and in the combine; with all scalars equal over `alt` the sum cancels
    to the identity (even n) or collapses to one point (odd n)"""
    n = 4097
    pts = D.srs_bytes(name, 12)[:64 * n]
    s = D.random_scalars(n, 5)
    assert run(ctx, pts, s) == D.expected(name, s)
    assert run(ctx, pts, s, 16) == D.expected(name, s)
    eq = [s[0]] * n
    assert run(ctx, pts, eq) == D.expected(name, eq)
    assert run(ctx, pts[:64 * 4096], eq[:4096]) == D.expected(name, eq[:4096])
    if name == "alt":
        assert D.expected(name, eq[:4096]) == bytes(64)
        assert D.expected(name, eq) == D.expected(name, eq[:1])


def test_identities_among_real_bases(ctx, bases):
    n = 4097
    s = D.random_scalars(n, 8)
    pts = bytearray(bases[:64 * n])
    kept = list(s)
    for i in range(0, n, 3):
        pts[64 * i:64 * i + 64] = bytes(64)
        kept[i] = 0
    assert run(ctx, bytes(pts), s) == M.closed_form(kept)
    assert run(ctx, bytes(64 * n), s) == bytes(64)


def test_scalars_above_r(ctx, bases):
    n = 513
    s = D.random_scalars(n, 12)
    big = [v + R * k for k, v in zip([0, 1, 2, 3, 4] * n, s)]
    big[5] = (1 << 256) - 1
    big[6], big[7] = R, R + 1
    assert all(v < 1 << 256 for v in big)
    reduced = [v % R for v in big]
    for c in (0, 16):
        got = run(ctx, bases[:64 * n], big, c)
        assert got == run(ctx, bases[:64 * n], reduced, c) == M.closed_form(reduced)


# ------------------------------------------------------------------ the other entry points
def test_agrees_with_fixed_base_and_host(K, ctx, bases, rand_big):
    s, sb, want = rand_big
    pts = bases[:64 * BIG]
    assert ctx.msm_points(pts, sb) == want
    assert K.msm_points(pts[:64 * 4097], sb[:32 * 4097], device=None) == M.closed_form(s[:4097])
    other = K.Context(0)
    try:
        buf = ctypes.create_string_buffer(pts, len(pts))
        assert K.lib().kgs_srs_load_points(other.handle, buf, BIG, 15, 15) == 0
        assert other.msm(common.mont_bytes(s)) == want
    finally:
        other.close()


def _hip(K):
    K.lib()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


def test_device_entry(K, ctx, bases):
    n = 4097
    s = D.random_scalars(n, 21)
    pts, sb = bases[:64 * n], M.scalar_bytes(s)
    hip = _hip(K)
    dp, ds = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dp), len(pts)) == 0 and hip.hipMalloc(ctypes.byref(ds), len(sb)) == 0
    try:
        assert hip.hipMemcpy(dp, pts, len(pts), 1) == 0 and hip.hipMemcpy(ds, sb, len(sb), 1) == 0
        for c in (0, 13):
            assert ctx.msm_points_device(dp.value, ds.value, n, c) == ctx.msm_points(pts, sb, c) == M.closed_form(s)
        back_p, back_s = ctypes.create_string_buffer(len(pts)), ctypes.create_string_buffer(len(sb))
        assert hip.hipMemcpy(back_p, dp, len(pts), 2) == 0 and hip.hipMemcpy(back_s, ds, len(sb), 2) == 0
        assert back_p.raw == pts and back_s.raw == sb  # the caller's buffers are read only
    finally:
        hip.hipFree(dp)
        hip.hipFree(ds)


# ------------------------------------------------------------------ the context contract
def test_context_state_is_left_alone(K, bases):
    c = K.Context(0)
    try:
        c.load_ptau(common.oracle_ptau(11), 10)
        info = c.srs_info()
        sm = common.mont_bytes(D.random_scalars(1 << 10, 1))
        A = c.msm(sm)
        Fs, Ts, sF, sT = common.make_inputs(33, 10, 2, True)
        proof = c.prove(K.GRANDSUM, 10, Fs, Ts, sF, sT, mont_out=False)[:2]
        s = D.random_scalars(777, 2)
        for w in (0, 16):
            assert run(c, bases[:64 * 777], s, w) == M.closed_form(s)
            assert c.idle()
        assert c.srs_info() == info
        assert c.msm(sm) == A
        assert c.prove(K.GRANDSUM, 10, Fs, Ts, sF, sT, mont_out=False)[:2] == proof
        with pytest.raises(K.KgsError) as e:
            run(c, bases[:64 * 777], s, 17)
        assert e.value.code == KGS_E_ARG and c.idle()
        assert c.srs_info() == info and c.msm(sm) == A
    finally:
        c.close()


def test_argument_errors_on_a_context(K, ctx, bases):
    s = D.random_scalars(4, 3)
    L = K.lib()
    out = ctypes.create_string_buffer(64)
    sb = ctypes.create_string_buffer(M.scalar_bytes(s), 128)
    assert L.kgs_msm_points(ctx.handle, None, sb, 4, 0, out) == KGS_E_ARG
    assert L.kgs_msm_points_device(ctx.handle, None, None, 4, 0, out) == KGS_E_ARG
    assert L.kgs_msm_points(ctx.handle, sb, sb, (1 << 26) + 1, 0, out) == KGS_E_ARG
    assert ctx.idle()
    assert run(ctx, b"", []) == bytes(64)  # n == 0
    other = K.Context(0)
    try:
        other.set_shard(0, 2, lambda b: b + b)
        with pytest.raises(K.KgsError) as e:
            run(other, bases[:256], s)
        assert e.value.code == KGS_E_ARG and "shard" in str(e.value)
        other.set_shard(0, 1)
        grp = K.Group.local(2)
        other.set_group(grp, 0)
        with pytest.raises(K.KgsError) as e:
            run(other, bases[:256], s)
        assert e.value.code == KGS_E_ARG and "rank group" in str(e.value)
        other.set_group(None)
        assert run(other, bases[:256], s) == M.closed_form(s)  # a context without an SRS
        assert other.idle()
    finally:
        other.close()
