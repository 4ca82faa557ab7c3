"""Openings on the GPU: kgs_g1_mul_each (the per-point multiplication) as a primitive, kgs_kzg_open_all
(every opening on the domain at once, FK20) byte for byte against the closed form over tau^i G at every
size 2^0 .. 2^8, short and structured polynomials, degenerate SRS, a random functional at 2^12 and 2^14,
kgs_kzg_open (one opening) against it and against kgs_kzg_verify, the cache and the context contract."""
import ctypes
import json
import os
import random

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
import kzg_open_cases as Z
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
    path = f"/tmp/kgs_test_kzg_open_p{POWER}.{os.getpid()}.ptau"
    c = K.Context(0)
    try:
        c.write_synthetic_ptau(path, POWER, common.tau())
        yield path
    finally:
        c.close()
        if os.path.exists(path):
            os.remove(path)


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


@pytest.fixture(scope="module")
def tau_g2():
    return Z.tau_g2()


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


def coefs(nbits, count, seed=0):
    rnd = random.Random(7000 + 100 * nbits + count + seed)
    return [rnd.randrange(R) for _ in range(count)]


# ------------------------------------------------------------------ g1_mul_each as a primitive
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_g1_mul_each(K, plain, n):
    """a partial wave, a whole 64-thread block, one lane of a second block, several blocks; identities
    among the points; the edge scalars of the recoding and scalars above r"""
    mult, s = Z.mul_each_case(n, 40 + n)
    pts, sc = N.points(mult), N.scalar_bytes(s)
    want = Z.mul_each_expected(mult, s)
    assert plain.g1_mul_each(pts, sc) == want
    assert K.g1_mul_each(pts, sc, device=None) == want
    hip = _hip(K)
    dp, ds, do = DevBuf(hip, pts), DevBuf(hip, sc), DevBuf(hip, bytes(64 * n))
    try:
        plain.g1_mul_each_device(dp.p.value, ds.p.value, n, do.p.value)
        assert do.read() == want and dp.read() == pts and ds.read() == sc  # the inputs are only read
        plain.g1_mul_each_device(dp.p.value, ds.p.value, n, dp.p.value)  # aliased
        assert dp.read() == want
    finally:
        for b in (dp, ds, do):
            b.free()
    assert plain.idle()


def test_g1_mul_each_arguments(K, plain):
    assert plain.g1_mul_each(b"", b"") == b""
    L = K.lib()
    b = ctypes.create_string_buffer(128)
    assert L.kgs_g1_mul_each(plain.handle, None, b, 2, b) == KGS_E_ARG
    assert L.kgs_g1_mul_each(plain.handle, b, b, (1 << 26) + 1, b) == KGS_E_ARG
    assert plain.idle()


# ------------------------------------------------------------------ every size, byte for byte
@pytest.mark.parametrize("nbits", range(9))
def test_every_size_against_the_closed_form(ctx, nbits):
    """nbits 0 .. 5: 2n < 64 points, a partial wave in the pointwise pass and per-lane stages only;
    nbits >= 6: the transform of 2n points has stages with 64 butterfly groups (the per-wave mapping)"""
    n = 1 << nbits
    c = coefs(nbits, n)
    proofs, ev = ctx.kzg_open_all(Z.mont(c), nbits, evals=True)
    assert proofs == Z.expected_proofs(c, nbits)
    assert ev == Z.mont(Z.evals(c, nbits))
    assert ctx.kzg_open_all(Z.mont(c)) == proofs  # nbits from the length, no evaluations
    assert ctx.idle()


@pytest.mark.parametrize("nbits", [3, 6, 8])
def test_short_polynomials(ctx, nbits):
    n = 1 << nbits
    for count in (0, 1, n // 2 + 1):
        c = coefs(nbits, count, 3)
        proofs, ev = ctx.kzg_open_all(Z.mont(c), nbits, evals=True)
        assert proofs == Z.expected_proofs(c, nbits), count
        assert ev == Z.mont(Z.evals(c, nbits)), count
        if count < 2:
            assert proofs == bytes(64 * n)


@pytest.mark.parametrize("nbits", [2, 6, 8])
def test_structured_polynomials(ctx, nbits):
    n = 1 << nbits
    # p = 0 with all n coefficients given: every c^_i is zero
    assert ctx.kzg_open_all(Z.mont([0] * n), nbits) == bytes(64 * n)
    # p = r - 1: every c^_i is nonzero, every proof the identity by cancellation in the inverse transform
    proofs, ev = ctx.kzg_open_all(Z.mont([R - 1] + [0] * (n - 1)), nbits, evals=True)
    assert proofs == bytes(64 * n) and ev == Z.mont([R - 1] * n)
    # p = X^(n - 1): q_i = sum_k w^(i (n - 2 - k)) X^k
    c = [0] * (n - 1) + [1]
    assert ctx.kzg_open_all(Z.mont(c), nbits) == Z.expected_proofs(c, nbits)
    # a root at w^3: p = (X - w^3) g
    w3 = N.omegas(nbits)[3]
    g = coefs(nbits, n - 1, 11)
    c = [((g[i - 1] if i else 0) - w3 * (g[i] if i < n - 1 else 0)) % R for i in range(n)]
    proofs, ev = ctx.kzg_open_all(Z.mont(c), nbits, evals=True)
    assert ev[32 * 3:32 * 4] == bytes(32)
    assert proofs == Z.expected_proofs(c, nbits)
    y, proof = ctx.kzg_open(Z.mont(c), Z.mont([w3]))
    assert y == bytes(32) and proof == proofs[64 * 3:64 * 4] == N.point(Z.poly_eval(g, common.tau()))


# ------------------------------------------------------------------ agreement with the single opening
@pytest.mark.parametrize("nbits", [4, 8, 10])
def test_single_openings_agree_and_verify(K, ctx, tau_g2, nbits):
    n = 1 << nbits
    c = coefs(nbits, n, 21)
    cm = Z.mont(c)
    proofs, ev = ctx.kzg_open_all(cm, nbits, evals=True)
    C = ctx.msm(cm)
    assert C == Z.commitment(c)
    ws = N.omegas(nbits)
    rnd = random.Random(nbits)
    for i in [0, n - 1] + rnd.sample(range(1, n - 1), 6):
        z = Z.mont([ws[i]])
        y, proof = ctx.kzg_open(cm, z)
        assert y == ev[32 * i:32 * i + 32] and proof == proofs[64 * i:64 * i + 64], i
        assert K.kzg_verify(tau_g2, C, z, y, proof) is True
    for zi in (rnd.randrange(R), 0, 2):  # off the domain
        z = Z.mont([zi])
        y, proof = ctx.kzg_open(cm, z)
        assert y == Z.mont([Z.poly_eval(c, zi)])
        assert proof == N.point(Z.quotient_form(c, zi, common.tau()))
        assert K.kzg_verify(tau_g2, C, z, y, proof) is True
        bad = bytearray(proof)
        bad[9] ^= 0x10
        assert K.kzg_verify(tau_g2, C, z, y, bytes(bad)) is False
        assert K.kzg_verify(tau_g2, C, z, y, proofs[:64]) is False  # a valid point, another opening
    assert ctx.idle()


def test_single_opening_edge_lengths(ctx):
    z = Z.mont([5])
    assert ctx.kzg_open(b"", z) == (bytes(32), bytes(64))
    assert ctx.kzg_open(Z.mont([9]), z) == (Z.mont([9]), bytes(64))
    assert ctx.kzg_open(Z.mont([9, 4]), z) == (Z.mont([29]), N.point(4))
    c = coefs(12, 5000)  # more than one Horner tile, not a power of two
    y, proof = ctx.kzg_open(Z.mont(c), z)
    assert y == Z.mont([Z.poly_eval(c, 5)]) and proof == N.point(Z.quotient_form(c, 5, common.tau()))


# ------------------------------------------------------------------ degenerate SRS
@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_srs(K, name):
    """tau = 1: all SRS points equal; r - 1: P / -P; a 4th root of unity; 0: G, then zero points. The equal,
    opposite and identity branches of both transforms and of the pointwise pass are on this path."""
    tau = D.TAUS[name]
    c = K.Context(0)
    try:
        with D.ptau_file(name, 8, "_kzg") as path:
            c.load_ptau(path, 8)
            for nbits in (2, 6):
                p = coefs(nbits, 1 << nbits, 31)
                assert c.kzg_open_all(Z.mont(p), nbits) == N.points(Z.quotient_scalars(p, nbits, tau)), nbits
                y, proof = c.kzg_open(Z.mont(p), Z.mont([N.omegas(nbits)[1]]))
                assert proof == N.point(Z.quotient_form(p, N.omegas(nbits)[1], tau))
            assert c.idle()
    finally:
        c.close()


# ------------------------------------------------------------------ larger sizes
@pytest.mark.parametrize("nbits", [12, 14])
def test_larger_sizes(K, ctx, nbits):
    """a random functional of all proofs against the closed form in the exponent, and 16 sampled proofs
    byte for byte (a functional could hide a permutation of equal weight; the samples bound that)"""
    n = 1 << nbits
    c = coefs(nbits, n, 41)
    hip = _hip(K)
    dc, dp, de = DevBuf(hip, Z.mont(c)), DevBuf(hip, bytes(64 * n)), DevBuf(hip, bytes(32 * n))
    try:
        ctx.kzg_open_all_device(dc.p.value, n, nbits, dp.p.value, de.p.value)
        proofs, ev = dp.read(), de.read()
        assert dc.read() == Z.mont(c)  # the input is only read
    finally:
        for b in (dc, dp, de):
            b.free()
    want = Z.closed_form(c, nbits)
    assert ev == Z.mont(Z.evals(c, nbits))
    r = D.random_scalars(n, 900 + nbits)
    assert ctx.msm_points(proofs, N.scalar_bytes(r)) == N.point(sum(a * b for a, b in zip(r, want)) % R)
    for i in [0, 1, n - 1] + random.Random(nbits).sample(range(2, n - 1), 13):
        assert proofs[64 * i:64 * i + 64] == N.point(want[i]), i
    assert ctx.idle()


# ------------------------------------------------------------------ cache and contract
def test_cached_row_is_reused_and_shared(K, ctx, ptau16):
    c = coefs(9, 512, 51)
    first = ctx.kzg_open_all(Z.mont(c), 9)
    assert ctx.kzg_open_all(Z.mont(c), 9) == first  # from the cache
    other = K.Context(0)
    try:
        other.load_ptau(ptau16, POWER)
        assert other.kzg_open_all(Z.mont(c), 9) == first
        assert first[64 * 5:64 * 6] == N.point(Z.closed_form(c, 9)[5])
    finally:
        other.close()
    # the Lagrange cache of the same SRS is another row and stays correct
    assert ctx.srs_lagrange(4) == N.expected_inverse(4)


def _golden_proof(K):
    case = min((x for x in GOLD["cases"] if x["kind"] == "grandsum"), key=lambda x: (x["nbits"], x["npols"]))
    Fs, Ts, sF, sT = common.make_inputs(case["seed"], case["nbits"], case["npols"], case["selected"])
    eF, eT = [K.Evaluations(x) for x in Fs], [K.Evaluations(x) for x in Ts]
    proof = K.grandsum_prover(common.oracle_ptau(11), eF if case["npols"] > 1 else eF[0],
                              eT if case["npols"] > 1 else eT[0],
                              K.Evaluations(sF) if sF else None, K.Evaluations(sT) if sT else None)
    got = {sec: {k: v.hex() for k, v in proof[sec].items()} for sec in ("commitments", "evaluations")}
    return got, case["proof"], case["nbits"]


def test_context_state_is_left_alone(K):
    got, want, nbits = _golden_proof(K)
    assert got == want
    c = K._context(0)  # the context the module-level prover keeps the SRS on
    info = c.srs_info()
    sm = common.mont_bytes(D.random_scalars(1 << nbits, 1))
    A = c.msm(sm)
    p = coefs(nbits, 1 << nbits, 61)
    assert c.kzg_open_all(Z.mont(p), nbits) == Z.expected_proofs(p, nbits) and c.idle()
    y, proof = c.kzg_open(Z.mont(p), Z.mont([3]))
    assert proof == N.point(Z.quotient_form(p, 3, common.tau())) and c.idle()
    with pytest.raises(K.KgsError) as err:
        c.kzg_open_all(Z.mont(p), 24)
    assert err.value.code == KGS_E_ARG and c.idle()
    with pytest.raises(K.KgsError) as err:
        c.kzg_open_all(Z.mont(p), 12)  # above the domain the SRS was loaded for
    assert err.value.code == KGS_E_ARG and c.idle()
    assert c.srs_info() == info and c.msm(sm) == A
    assert _golden_proof(K)[0] == want


def test_refusals(K, ctx, plain, ptau16):
    p = Z.mont(coefs(3, 8))
    for nbits in (-1, 24, 25):
        with pytest.raises(K.KgsError) as e:
            ctx.kzg_open_all(p, nbits)
        assert e.value.code == KGS_E_ARG and "nbits" in str(e.value) and ctx.idle()
    with pytest.raises(K.KgsError) as e:
        ctx.kzg_open_all(p, POWER + 1)
    assert e.value.code == KGS_E_ARG and "nbits_max" in str(e.value) and ctx.idle()
    with pytest.raises(K.KgsError) as e:
        ctx.kzg_open_all(p, 2)
    assert e.value.code == KGS_E_ARG and "len" in str(e.value) and ctx.idle()
    L = K.lib()
    out = ctypes.create_string_buffer(64 * 8)
    assert L.kgs_kzg_open_all(ctx.handle, None, 8, 3, out, None) == KGS_E_ARG  # a NULL buffer with work to do
    assert L.kgs_kzg_open_all(ctx.handle, p, 8, 3, None, None) == KGS_E_ARG and ctx.idle()
    for call in (lambda: plain.kzg_open_all(p, 3), lambda: plain.kzg_open(p, bytes(32))):
        with pytest.raises(K.KgsError) as e:
            call()
        assert e.value.code == KGS_E_SRS and "no SRS loaded" in str(e.value) and plain.idle()
    c = K.Context(0)
    try:
        c.load_ptau(ptau16, 10)
        calls = (lambda: c.kzg_open_all(p, 3), lambda: c.kzg_open(p, bytes(32)),
                 lambda: c.g1_mul_each(N.point(1), bytes(32)))
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
        assert c.kzg_open_all(p, 3) == Z.expected_proofs(Z.from_mont(p), 3) and c.idle()
        c.load_ptau(ptau16, 10, slice=(0, 2))
        for f in calls[:2]:
            with pytest.raises(K.KgsError) as e:
                f()
            assert e.value.code == KGS_E_ARG and "slice" in str(e.value) and c.idle()
    finally:
        c.close()


def test_module_level_entry_points(K, ptau16, tau_g2):
    c = coefs(5, 20, 71)  # 20 coefficients: the domain of 32 points
    proofs, ev = K.kzg_open_all(ptau16, Z.mont(c))
    assert proofs == Z.expected_proofs(c, 5) and ev == Z.mont(Z.evals(c, 5))
    mult, s = Z.mul_each_case(9, 3)
    assert K.g1_mul_each(N.points(mult), N.scalar_bytes(s)) == Z.mul_each_expected(mult, s)
    z = Z.mont([N.omegas(5)[7]])
    assert K.kzg_verify(ptau16, Z.commitment(c), z, ev[32 * 7:32 * 8], proofs[64 * 7:64 * 8]) is True
    assert K.kzg_verify(tau_g2, Z.commitment(c), z, ev[32 * 7:32 * 8], proofs[64 * 8:64 * 9]) is False
