"""The G1 transform on the GPU (kgs_g1_ntt, kgs_g1_ntt_device), the Lagrange-basis SRS (kgs_srs_lagrange)
and commitments from evaluations (kgs_commit_evals, kgs_commit_evals_device): byte for byte against the
closed forms over tau^i G at every size 2^0 .. 2^10, the Fr transform in the exponent for general and
degenerate inputs, round trips and a random functional at 2^12 .. 2^16, the coefficient path of the
prover for commit_evals, and the context contract."""
import ctypes
import json
import os
import random

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
from oracle import ptau as opt

pytestmark = pytest.mark.gpu
R = N.R
KGS_E_ARG, KGS_E_SRS = -1, -7
POWER = 16  # 2^17 - 1 points tau^i G
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ptau16(K):
    """a ptau of the module's own with the points tau^i G (common.tau()), written by the GPU writer"""
    path = f"/tmp/kgs_test_g1_ntt_p{POWER}.{os.getpid()}.ptau"
    c = K.Context(0)
    try:
        c.write_synthetic_ptau(path, POWER, common.tau())
        yield path
    finally:
        c.close()
        if os.path.exists(path):
            os.remove(path)


@pytest.fixture(scope="module")
def bases(ptau16):
    return opt.PTau(ptau16).g1_bytes


@pytest.fixture(scope="module")
def ctx(K, ptau16):
    """a context with the 2^16 SRS resident"""
    c = K.Context(0)
    c.load_ptau(ptau16, POWER)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain(K):
    """a context without an SRS"""
    c = K.Context(0)
    yield c
    c.close()


def gpu_points(ctx, scalars):
    """a_i G made on the GPU: one-term segments of kgs_g1_lincomb over the generator"""
    n = len(scalars)
    return ctx.g1_lincomb(N.point(1) * n, N.scalar_bytes(scalars), list(range(n + 1)))


def _hip(K):
    K.lib()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


class DevBuf:
    def __init__(self, hip, data):
        self.hip, self.n, self.p = hip, len(data), ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(self.p), max(self.n, 64)) == 0
        assert hip.hipMemcpy(self.p, bytes(data), self.n, 1) == 0

    def read(self):
        out = ctypes.create_string_buffer(self.n)
        assert self.hip.hipMemcpy(out, self.p, self.n, 2) == 0
        return out.raw

    def free(self):
        self.hip.hipFree(self.p)


# ------------------------------------------------------------------ every size, closed forms
@pytest.mark.parametrize("logm", range(11))
def test_every_size_over_tau_powers(plain, bases, logm):
    """2^0 .. 2^10 covers every stage shape: the copy (logm 0), the twiddle-free first stage, and from
    logm = 8 on the stages with at least 64 butterfly groups, which take the per-wave twiddle mapping
    (stage h, 2 <= h <= 2^(logm - 7)); below logm = 8 every stage runs the per-lane mapping. There is
    no other switch of kernel or path at any size."""
    x = bases[:64 << logm]
    assert plain.g1_ntt(x) == N.expected_forward(logm)
    assert plain.g1_ntt(x, inverse=True) == N.expected_inverse(logm)
    assert plain.idle()


# ------------------------------------------------------------------ general scalars, host and device entry
@pytest.mark.parametrize("logm", [1, 3, 7, 9])
def test_general_scalars_host_and_device(K, plain, logm):
    n = 1 << logm
    a = D.random_scalars(n, 500 + logm)
    x = gpu_points(plain, a)
    want_f = N.points(N.transform_scalars(a))
    want_i = N.points(N.transform_scalars(a, inverse=True))
    assert plain.g1_ntt(x) == want_f
    assert plain.g1_ntt(x, inverse=True) == want_i
    hip = _hip(K)
    din, dout = DevBuf(hip, x), DevBuf(hip, bytes(64 * n))
    try:
        plain.g1_ntt_device(din.p.value, dout.p.value, logm)
        assert dout.read() == want_f and din.read() == x  # the input is only read
        plain.g1_ntt_device(din.p.value, dout.p.value, logm, inverse=True)
        assert dout.read() == want_i and din.read() == x
        plain.g1_ntt_device(din.p.value, din.p.value, logm)  # aliased
        assert din.read() == want_f
        plain.g1_ntt_device(din.p.value, din.p.value, logm, inverse=True)
        assert din.read() == x
    finally:
        din.free()
        dout.free()


# ------------------------------------------------------------------ degenerate inputs
@pytest.mark.parametrize("logm", [2, 6, 8])
@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_points(plain, name, logm):
    """all points equal (the a + b of every butterfly is a doubling, every a - b the identity), P / -P
    alternating, the 4-cycle, G then zero points"""
    n = 1 << logm
    x = D.srs_bytes(name, 8)[:64 * n]
    k = D.multipliers(name, n)
    assert plain.g1_ntt(x) == N.points(N.transform_scalars(k))
    assert plain.g1_ntt(x, inverse=True) == N.points(N.lagrange_scalars(logm, D.TAUS[name]))


@pytest.mark.parametrize("logm", [2, 6, 8])
def test_identities(plain, logm):
    n = 1 << logm
    assert plain.g1_ntt(bytes(64 * n)) == bytes(64 * n) == plain.g1_ntt(bytes(64 * n), inverse=True)
    a = D.random_scalars(n, 70 + logm)
    rnd = random.Random(logm)
    for i in rnd.sample(range(n), n // 3):
        a[i] = 0
    a[0] = a[n - 1] = 0
    x = gpu_points(plain, a)
    assert x[:64] == bytes(64)
    assert plain.g1_ntt(x) == N.points(N.transform_scalars(a))


# ------------------------------------------------------------------ larger sizes
@pytest.mark.parametrize("logm", [12, 14, 16])
def test_larger_sizes(plain, bases, logm):
    """round trip, and a random functional of the output against the closed form in the exponent"""
    n = 1 << logm
    x = bases[:64 * n]
    y = plain.g1_ntt(x)
    assert plain.g1_ntt(y, inverse=True) == x
    r = D.random_scalars(n, 900 + logm)
    s = N.forward_scalars(logm)
    assert plain.msm_points(y, N.scalar_bytes(r)) == N.point(sum(a * b for a, b in zip(r, s)) % R)
    z = plain.g1_ntt(x, inverse=True)
    s = N.lagrange_scalars(logm)
    assert plain.msm_points(z, N.scalar_bytes(r)) == N.point(sum(a * b for a, b in zip(r, s)) % R)


# ------------------------------------------------------------------ srs_lagrange
@pytest.mark.parametrize("nbits", range(1, 11))
def test_srs_lagrange_closed_form(ctx, plain, bases, nbits):
    n = 1 << nbits
    L = ctx.srs_lagrange(nbits)
    assert L == N.expected_inverse(nbits)
    assert L == plain.g1_ntt(bases[:64 * n], inverse=True)
    assert plain.msm_points(L, N.scalar_bytes([1] * n)) == N.point(1)  # partition of unity
    assert ctx.srs_lagrange(nbits) == L  # from the cache
    assert ctx.srs_lagrange(nbits, fetch=False) is None
    assert ctx.idle()


def test_srs_lagrange_is_shared_on_the_device(K, ctx, ptau16):
    other = K.Context(0)
    try:
        other.load_ptau(ptau16, POWER)
        assert other.srs_lagrange(9) == ctx.srs_lagrange(9) == N.expected_inverse(9)
    finally:
        other.close()


@pytest.mark.parametrize("name", list(D.TAUS))
def test_srs_lagrange_degenerate_tau(K, name):
    """tau in {1, r - 1, a 4th root of unity, 0}: the table row holds equal, opposite and zero points"""
    c = K.Context(0)
    try:
        with D.ptau_file(name, 8, "_g1ntt") as path:
            c.load_ptau(path, 8)
            for nbits in (0, 1, 2, 6, 8):
                assert c.srs_lagrange(nbits) == N.points(N.lagrange_scalars(nbits, D.TAUS[name])), nbits
            e = D.random_scalars(256, 17)
            want = N.point(sum(a * b for a, b in zip(e, N.lagrange_scalars(8, D.TAUS[name]))) % R)
            assert c.commit_evals(N.scalar_bytes(e)) == want
    finally:
        c.close()


def test_srs_lagrange_refusals(K, ctx, plain, ptau16):
    for nbits in (-1, POWER + 1, 25):
        with pytest.raises(K.KgsError) as e:
            ctx.srs_lagrange(nbits)
        assert e.value.code == KGS_E_ARG and "nbits" in str(e.value) and ctx.idle()
    with pytest.raises(K.KgsError) as e:
        plain.srs_lagrange(3)
    assert e.value.code == KGS_E_SRS and "no SRS loaded" in str(e.value) and plain.idle()
    with pytest.raises(K.KgsError) as e:
        plain.commit_evals(bytes(64))
    assert e.value.code == KGS_E_SRS
    small = K.Context(0)
    try:
        small.load_ptau(common.oracle_ptau(11), 8)  # loaded for a smaller domain than the file holds
        with pytest.raises(K.KgsError) as e:
            small.srs_lagrange(9)
        assert e.value.code == KGS_E_ARG and "nbits_max" in str(e.value)
        assert small.srs_lagrange(8) == N.expected_inverse(8)
        small.load_ptau(ptau16, 10, slice=(0, 2))
        with pytest.raises(K.KgsError) as e:
            small.srs_lagrange(4)
        assert e.value.code == KGS_E_ARG and "slice" in str(e.value) and small.idle()
        with pytest.raises(K.KgsError) as e:
            small.commit_evals(bytes(32 * 16))
        assert e.value.code == KGS_E_ARG and "slice" in str(e.value)
    finally:
        small.close()


# ------------------------------------------------------------------ commit_evals
def _eval_families(n, seed):
    rnd = random.Random(seed)
    big = [min(v + R * k, (1 << 256) - 1) for k, v in zip([1, 2, 3, 4, 5] * n, D.random_scalars(n, seed + 1))]
    big[0] = (1 << 256) - 1
    big[n - 1] = R
    return {"random": D.random_scalars(n, seed), "selector": [1] * (n - 1) + [0],
            "16-bit": [rnd.randrange(1 << 16) for _ in range(n)], "above-r": big, "zeros": [0] * n,
            "first": [rnd.randrange(1, R)] + [0] * (n - 1), "last": [0] * (n - 1) + [rnd.randrange(1, R)]}


@pytest.mark.parametrize("nbits", [1, 2, 5, 10, 13, 16])
def test_commit_evals_is_the_coefficient_path(K, ctx, nbits):
    n = 1 << nbits
    hip = _hip(K)
    for what, e in _eval_families(n, 1000 + nbits).items():
        eb = N.scalar_bytes(e)
        want = ctx.msm(ctx.ntt(ctx.fr_to_mont(N.scalar_bytes([v % R for v in e])), inverse=True))
        if what == "above-r":  # the conversion of the coefficient path takes any 256-bit value too
            assert ctx.msm(ctx.ntt(ctx.fr_to_mont(eb), inverse=True)) == want
        assert ctx.commit_evals(eb) == want, what
        assert ctx.commit_evals(eb, nbits) == want, what
        if what == "zeros":
            assert want == bytes(64)
        d = DevBuf(hip, eb)
        try:
            assert ctx.commit_evals_device(d.p.value, nbits) == want, what
            assert d.read() == eb
        finally:
            d.free()
    assert ctx.idle()


def test_module_level_entry_points(K, ptau16, bases):
    e = D.random_scalars(32, 5)
    want = N.point(sum(a * b for a, b in zip(e, N.lagrange_scalars(5))) % R)
    assert K.commit_evals(ptau16, N.scalar_bytes(e)) == want
    assert K.commit_evals(ptau16, K.Evaluations(N.scalar_bytes(e))) == want
    assert K.g1_ntt(bases[:64 * 32]) == N.expected_forward(5) == K.g1_ntt(bases[:64 * 32], device=None)


# ------------------------------------------------------------------ the context contract
def _golden_proof(K):
    case = min((x for x in GOLD["cases"] if x["kind"] == "grandsum"), key=lambda x: (x["nbits"], x["npols"]))
    Fs, Ts, sF, sT = common.make_inputs(case["seed"], case["nbits"], case["npols"], case["selected"])
    eF, eT = [K.Evaluations(x) for x in Fs], [K.Evaluations(x) for x in Ts]
    proof = K.grandsum_prover(common.oracle_ptau(11), eF if case["npols"] > 1 else eF[0],
                              eT if case["npols"] > 1 else eT[0],
                              K.Evaluations(sF) if sF else None, K.Evaluations(sT) if sT else None)
    got = {sec: {k: v.hex() for k, v in proof[sec].items()} for sec in ("commitments", "evaluations")}
    return got, case["proof"], case["nbits"]


def test_context_state_is_left_alone(K, bases):
    got, want, nbits = _golden_proof(K)
    assert got == want
    c = K._context(0)  # the context the module-level prover keeps the SRS on
    info = c.srs_info()
    sm = common.mont_bytes(D.random_scalars(1 << nbits, 1))
    A = c.msm(sm)
    assert c.g1_ntt(bases[:64 * 256]) == N.expected_forward(8) and c.idle()
    assert c.srs_lagrange(nbits) == N.expected_inverse(nbits) and c.idle()
    e = D.random_scalars(1 << nbits, 2)
    assert c.commit_evals(N.scalar_bytes(e)) == c.msm(c.ntt(c.fr_to_mont(N.scalar_bytes(e)), inverse=True))
    assert c.idle()
    with pytest.raises(K.KgsError) as err:
        c.srs_lagrange(25)
    assert err.value.code == KGS_E_ARG and c.idle()
    with pytest.raises(K.KgsError) as err:
        c.commit_evals(bytes(32 << 12), 12)  # above the domain the SRS was loaded for
    assert err.value.code == KGS_E_ARG and c.idle()
    assert c.srs_info() == info and c.msm(sm) == A
    assert _golden_proof(K)[0] == want


def test_rank_group_and_sharding_are_refused(K, ptau16, bases):
    c = K.Context(0)
    try:
        c.load_ptau(ptau16, 10)
        calls = (lambda: c.g1_ntt(bases[:128]), lambda: c.srs_lagrange(3), lambda: c.commit_evals(bytes(64)))
        c.set_shard(0, 2, lambda b: b + b)
        for f in calls:
            with pytest.raises(K.KgsError) as e:
                f()
            assert e.value.code == KGS_E_ARG and "shard" in str(e.value)
        c.set_shard(0, 1)
        grp = K.Group.local(2)
        c.set_group(grp, 0)
        for f in calls:
            with pytest.raises(K.KgsError) as e:
                f()
            assert e.value.code == KGS_E_ARG and "rank group" in str(e.value)
        c.set_group(None)
        assert c.srs_lagrange(3) == N.expected_inverse(3) and c.idle()
    finally:
        c.close()
