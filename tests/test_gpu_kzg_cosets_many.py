"""kgs_kzg_open_cosets_many on the GPU: the coset openings of many polynomials in one call, byte for byte what
kgs_kzg_open_cosets ("the single call") gives for each polynomial alone on the same context, and against the
closed form on the CPU. One polynomial at every (nbits, lbits) up to 2^8; a few polynomials up to 2^6; the
seams of the batched stage's thread mapping (polys * G around 64, per-twiddle chunks that are no multiple of
64); zero, equal and opposite polynomials, short lengths, a stride with garbage in the gap; degenerate SRS; the
threshold of the grouped multiply-sum; Fr block transforms of several passes; the device twin; the cache and
the context contract; the module-level entry."""
import ctypes
import json
import os
import random

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
import kzg_coset_cases as C
import kzg_open_cases as Z

pytestmark = pytest.mark.gpu
R = N.R
KGS_E_ARG, KGS_E_SRS = -1, -7
POWER = 13
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ptau13(K):
    """a ptau of the module's own with the points tau^i G (common.tau()), written by the GPU writer"""
    path = f"/tmp/kgs_test_kzg_cosets_many_p{POWER}.{os.getpid()}.ptau"
    c = K.Context(0)
    try:
        c.write_synthetic_ptau(path, POWER, common.tau())
        yield path
    finally:
        c.close()
        if os.path.exists(path):
            os.remove(path)


@pytest.fixture(scope="module")
def ctx(K, ptau13):
    c = K.Context(0)
    c.load_ptau(ptau13, POWER)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain(K):
    """a context without an SRS"""
    c = K.Context(0)
    yield c
    c.close()


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


def polys_of(nbits, polys, seed, count=None):
    """`polys` random polynomials of `count` (default 2^nbits) coefficients, as integers"""
    rnd = random.Random(7000 + 1000 * nbits + 10 * polys + seed)
    count = (1 << nbits) if count is None else count
    return [[rnd.randrange(R) for _ in range(count)] for _ in range(polys)]


def single(ctx, c, nbits, lbits):
    """the single call on the same context: (proofs, evals)"""
    return ctx.kzg_open_cosets(Z.mont(c), nbits, lbits, evals=True)


def raw_many(K, ctx, buf, polys, stride, length, nbits, lbits, evals=True):
    """the C entry on a host buffer as it is: (proofs, evals) as whole byte strings"""
    n, m = 1 << nbits, 1 << (nbits - lbits)
    proofs = ctypes.create_string_buffer(max(64 * m * polys, 1))
    ev = ctypes.create_string_buffer(max(32 * n * polys, 1)) if evals else None
    src = ctypes.create_string_buffer(bytes(buf), max(len(buf), 1))
    rc = K.lib().kgs_kzg_open_cosets_many(ctx.handle, src, polys, stride, length, nbits, lbits, proofs, ev)
    assert rc == 0, K.lib().kgs_last_error().decode()
    return proofs.raw[:64 * m * polys], (ev.raw[:32 * n * polys] if evals else None)


def fold(ctx, proofs, rho):
    """sum_b rho_b proofs[b], column by column (kgs_g1_mul_sum, rows = polys, cols = m)"""
    m = len(proofs[0]) // 64
    return ctx.g1_mul_sum(b"".join(proofs), N.scalar_bytes([r for r in rho for _ in range(m)]), len(proofs))


def combine(ps, rho):
    return [sum(r * p[j] for r, p in zip(rho, ps) if j < len(p)) % R for j in range(max(len(p) for p in ps))]


# ------------------------------------------------------------------ against the single call, byte for byte
@pytest.mark.parametrize("nbits", range(9))
def test_one_polynomial_is_the_single_call(ctx, nbits):
    """polys = 1 at every lbits 0 .. nbits: lbits = 0 (kzg_open_all's path), m = 1, m = 2, evaluations included"""
    c = polys_of(nbits, 1, 1)[0]
    for lbits in range(nbits + 1):
        proofs, ev = ctx.kzg_open_cosets_many([Z.mont(c)], nbits, lbits, evals=True)
        assert (proofs[0], ev[0]) == single(ctx, c, nbits, lbits), lbits
        assert ctx.kzg_open_cosets_many([Z.mont(c)], nbits, lbits) == proofs  # no evaluations
    assert ctx.idle()


@pytest.mark.parametrize("polys", [2, 3, 5])
def test_a_few_polynomials(ctx, polys):
    """nbits 0 .. 6 x every lbits, random polynomials: each equals its single call, and the last one the closed
    form on the CPU"""
    for nbits in range(7):
        ps = polys_of(nbits, polys, 2)
        for lbits in range(nbits + 1):
            proofs, ev = ctx.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits, evals=True)
            assert len(proofs) == len(ev) == polys
            for b, p in enumerate(ps):
                assert (proofs[b], ev[b]) == single(ctx, p, nbits, lbits), (nbits, lbits, b)
            assert proofs[-1] == C.expected_proofs(ps[-1], nbits, lbits), (nbits, lbits)
    assert ctx.idle()


@pytest.mark.parametrize("polys", [31, 32, 33, 63, 64, 65, 130])
def test_mapping_seams_of_the_batched_stage(ctx, polys):
    """(nbits, lbits) = (3, 1) and (4, 2): m = 4, transforms of 8 and 4 points. With G = 2 groups in the second-last
    and G = 1 in the last stage of the inverse, polys * G crosses 64 at polys = 32 and 64: below it the per-lane
    mapping, from it on one twiddle per block, whose per-twiddle chunk (polys * G butterflies) is a multiple of
    64 only at polys = 32 and 64. Every proof against the closed form on the CPU."""
    for nbits, lbits in ((3, 1), (4, 2)):
        ps = polys_of(nbits, polys, 3)
        proofs = ctx.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits)
        for b, p in enumerate(ps):
            assert proofs[b] == N.points(C.closed_scalars(p, nbits, lbits)), (nbits, lbits, b)
    assert ctx.idle()


@pytest.mark.parametrize("nbits,lbits", [(3, 0), (4, 1), (5, 2)])
def test_the_four_stage_pass_of_the_fr_side(ctx, nbits, lbits):
    """m = 8 and 130 polynomials: the Fr side is l * 130 blocks of 2m = 16 over an array of 2^12, 2^13, 2^14
    elements, one LDS pass of four stages (two register rounds of two), which no whole transform and no shape above
    launches. Every proof against the closed form on the CPU."""
    polys = 130
    ps = polys_of(nbits, polys, 6)
    proofs = ctx.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits)
    for b, p in enumerate(ps):
        assert proofs[b] == N.points(C.closed_scalars(p, nbits, lbits)), (nbits, lbits, b)
    assert ctx.idle()


def test_the_four_stage_pass_of_the_evaluations(ctx):
    """(4, 1) with the evaluations: 130 blocks of n = 16 over an array of 2^12 as well; against the single call"""
    nbits, lbits, polys = 4, 1, 130
    ps = polys_of(nbits, polys, 6)
    proofs, ev = ctx.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits, evals=True)
    assert len(proofs) == len(ev) == polys
    for b, p in enumerate(ps):
        assert (proofs[b], ev[b]) == single(ctx, p, nbits, lbits), b
        assert ev[b] == Z.mont(Z.evals(p, nbits)), b  # and the integer transform
    assert ctx.idle()


# ------------------------------------------------------------------ contents
def test_zero_equal_and_opposite_polynomials(ctx):
    """a zero polynomial among others (its points are the identity through every stage), the same polynomial
    twice, p and r - p"""
    nbits, lbits = 5, 2
    n, l, m = C.sizes(nbits, lbits)
    p, q = polys_of(nbits, 2, 4)
    neg = [(R - x) % R for x in p]
    ps = [p, [0] * n, p, neg, q, [0] * n]
    proofs, ev = ctx.kzg_open_cosets_many([Z.mont(x) for x in ps], nbits, lbits, evals=True)
    want = [C.expected_proofs(x, nbits, lbits) for x in (p, q)]
    assert proofs[0] == proofs[2] == want[0] and proofs[4] == want[1]
    assert proofs[1] == proofs[5] == bytes(64 * m) and ev[1] == ev[5] == bytes(32 * n)
    assert proofs[3] == N.points([(R - s) % R for s in C.closed_scalars(p, nbits, lbits)])
    for b, x in enumerate(ps):
        assert (proofs[b], ev[b]) == single(ctx, x, nbits, lbits), b
    assert ctx.idle()


@pytest.mark.parametrize("length", [0, 1, 21, 64])
def test_lengths_and_a_stride_with_garbage_in_the_gap(K, ctx, length):
    """len = 0, 1, an odd one and n, with stride > len and nonzero bytes between len and stride: not a byte of the
    output depends on them (the host entry packs the rows, the device twin reads past the gap)"""
    nbits, lbits, polys = 6, 2, 3
    n, l, m = C.sizes(nbits, lbits)
    ps = polys_of(nbits, polys, 5, length)
    packed = b"".join(Z.mont(p) for p in ps)
    want = raw_many(K, ctx, packed, polys, length, length, nbits, lbits)
    for b, p in enumerate(ps):
        assert (want[0][64 * m * b:64 * m * (b + 1)], want[1][32 * n * b:32 * n * (b + 1)]) == single(ctx, p, nbits, lbits)
    assert want[0][:64 * m] == C.expected_proofs(ps[0], nbits, lbits)
    stride = length + 5
    rnd = random.Random(length)
    gaps = [bytes([0xFF]) * 160, rnd.randbytes(160), Z.mont([R - 1] * 5)]
    spaced = b"".join(Z.mont(p) + g for p, g in zip(ps, gaps))
    assert raw_many(K, ctx, spaced, polys, stride, length, nbits, lbits) == want
    hip = _hip(K)
    dc, dp, de = DevBuf(hip, spaced), DevBuf(hip, bytes(64 * m * polys)), DevBuf(hip, bytes(32 * n * polys))
    try:
        ctx.kzg_open_cosets_many_device(dc.p.value, polys, stride, length, nbits, lbits, dp.p.value, de.p.value)
        assert (dp.read(), de.read()) == want
        assert dc.read() == spaced
    finally:
        for b in (dc, dp, de):
            b.free()
    assert ctx.idle()


@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_srs(K, name):
    """equal, opposite and identity operands in the butterflies and in the column sums: every tau of
    degenerate_cases.TAUS, against the long division, which holds for tau in the domain"""
    tau = D.TAUS[name]
    c = K.Context(0)
    try:
        with D.ptau_file(name, 4, "_cosets_many") as path:
            c.load_ptau(path, 4)
            nbits = 4
            ps = polys_of(nbits, 3, 6)
            for lbits in (0, 2, 4):
                proofs = c.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits)
                for b, p in enumerate(ps):
                    assert proofs[b] == N.points(C.division_scalars(p, nbits, lbits, tau)), (lbits, b)
            assert c.idle()
    finally:
        c.close()


# ------------------------------------------------------------------ larger shapes
def check_by_samples_and_functional(K, ctx, ps, nbits, lbits, evals, seed, verify=False):
    """the first, the last and two random polynomials against the single call, and all of them at once through a
    random functional: sum_b rho_b proofs[b] is the single call on sum_b rho_b p_b"""
    polys = len(ps)
    n, l, m = C.sizes(nbits, lbits)
    out = ctx.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits, evals=evals)
    proofs, ev = out if evals else (out, None)
    assert len(proofs) == polys and all(len(x) == 64 * m for x in proofs)
    rnd = random.Random(seed)
    sample = sorted({0, polys - 1} | set(rnd.sample(range(polys), min(2, polys))))
    for b in sample:
        want = single(ctx, ps[b], nbits, lbits)
        assert proofs[b] == want[0], b
        if evals:
            assert ev[b] == want[1], b
        if verify:
            i = rnd.randrange(m)
            ys = C.coset_values(Z.from_mont(want[1]), nbits, lbits, i)
            args = (C.tau_l_g2(lbits), C.srs_g1(lbits), Z.commitment(ps[b]), nbits, lbits, i)
            assert K.kzg_verify_coset(*args, Z.mont(ys), proofs[b][64 * i:64 * i + 64]) is True
            ys[rnd.randrange(l)] += 1
            assert K.kzg_verify_coset(*args, Z.mont(ys), proofs[b][64 * i:64 * i + 64]) is False
    rho = D.random_scalars(polys, seed)
    comb = single(ctx, combine(ps, rho), nbits, lbits)
    assert fold(ctx, proofs, rho) == comb[0]
    if evals:
        es = [Z.from_mont(e) for e in ev]
        assert Z.mont([sum(r * e[k] for r, e in zip(rho, es)) % R for k in range(n)]) == comb[1]
    assert ctx.idle()


@pytest.mark.parametrize("polys", [63, 64, 65])
def test_threshold_of_the_grouped_multiply_sum(K, ctx, polys):
    """nbits 10, lbits 6: polys * 2n terms, below, at and above the 2^17 from which a lane takes two rows of a
    column; polys * 2m columns, an odd count of blocks of 64 at 63 and 65"""
    check_by_samples_and_functional(K, ctx, polys_of(10, polys, 7), 10, 6, False, 100 + polys)


@pytest.mark.parametrize("nbits,lbits,polys,half", [(12, 6, 3, False), (12, 6, 16, False), (13, 6, 5, True)])
def test_block_transforms_of_several_passes(K, ctx, nbits, lbits, polys, half):
    """the batched Fr transforms beyond one LDS pass (evaluations: blocks of 2^12 and 2^13), block counts that are
    no power of two (192 and 320 rows padded to 256 and 512; 3 and 5 blocks of evaluations to 4 and 8), len = n / 2"""
    count = (1 << nbits) // 2 if half else None
    check_by_samples_and_functional(K, ctx, polys_of(nbits, polys, 8, count), nbits, lbits, True, 200 + polys, verify=True)


def test_device_twin(K, ctx):
    nbits, lbits, polys = 7, 3, 5
    n, l, m = C.sizes(nbits, lbits)
    ps = polys_of(nbits, polys, 9, n - 3)
    packed = b"".join(Z.mont(p) for p in ps)
    want = raw_many(K, ctx, packed, polys, n - 3, n - 3, nbits, lbits)
    hip = _hip(K)
    dc, dp, de = DevBuf(hip, packed), DevBuf(hip, bytes(64 * m * polys)), DevBuf(hip, bytes(32 * n * polys))
    try:
        ctx.kzg_open_cosets_many_device(dc.p.value, polys, n - 3, n - 3, nbits, lbits, dp.p.value, de.p.value)
        assert (dp.read(), de.read()) == want
        assert dc.read() == packed  # the input is only read
        ctx.kzg_open_cosets_many_device(dc.p.value, polys, n - 3, n - 3, nbits, lbits, dp.p.value)  # no evaluations
        assert dp.read() == want[0]
    finally:
        for b in (dc, dp, de):
            b.free()
    assert want[0][:64 * m] == C.expected_proofs(ps[0], nbits, lbits)
    assert ctx.idle()


# ------------------------------------------------------------------ cache and contract
def test_the_cached_rows_are_the_single_calls(K, ctx, ptau13):
    """one row per (SRS, nbits, lbits) for both calls: either warms it for the other"""
    ps = polys_of(9, 3, 10)
    mont = [Z.mont(p) for p in ps]
    assert not ctx.kzg_open_cosets_cached(9, 4) and not ctx.kzg_open_cosets_cached(9, 2)
    first = ctx.kzg_open_cosets_many(mont, 9, 4)  # builds the row
    assert ctx.kzg_open_cosets_cached(9, 4) and not ctx.kzg_open_cosets_cached(9, 2)
    assert [ctx.kzg_open_cosets(x, 9, 4) for x in mont] == first  # the single call finds it
    assert first[0] == N.points(C.closed_scalars(ps[0], 9, 4))
    assert ctx.kzg_open_cosets_many(mont, 9, 4) == first
    one = [ctx.kzg_open_cosets(x, 9, 2) for x in mont]  # the reverse: the single call builds
    assert ctx.kzg_open_cosets_cached(9, 2)
    assert ctx.kzg_open_cosets_many(mont, 9, 2) == one and ctx.kzg_open_cosets_cached(9, 2)
    assert ctx.kzg_open_cosets_many(mont, 9, 2) == one
    assert ctx.kzg_open_cosets_many(mont, 9, 9) == [bytes(64)] * 3 and not ctx.kzg_open_cosets_cached(9, 9)  # m = 1
    assert ctx.kzg_open_cosets_many([b"", b""], 9, 5) == [bytes(64 * 16)] * 2 and not ctx.kzg_open_cosets_cached(9, 5)
    other = K.Context(0)
    try:
        other.load_ptau(ptau13, POWER)  # the same SRS tables: the rows are shared
        assert other.kzg_open_cosets_cached(9, 4)
        assert other.kzg_open_cosets_many(mont, 9, 4) == first
    finally:
        other.close()
    assert ctx.idle()


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
    lag = c.srs_lagrange(nbits)
    ps = polys_of(nbits, 3, 11)
    mont = [Z.mont(p) for p in ps]
    all_ = c.kzg_open_all(mont[0], nbits)
    for lbits in (0, 1, nbits - 1):
        proofs = c.kzg_open_cosets_many(mont, nbits, lbits)
        assert proofs == [Z.expected_proofs(p, nbits) if lbits == 0 else C.expected_proofs(p, nbits, lbits) for p in ps]
        assert c.idle()
    with pytest.raises(K.KgsError) as err:
        c.kzg_open_cosets_many(mont, 12, 2)  # above the domain the SRS was loaded for
    assert err.value.code == KGS_E_ARG and c.idle()
    assert c.srs_info() == info and c.srs_lagrange(nbits) == lag and c.kzg_open_all(mont[0], nbits) == all_
    assert _golden_proof(K)[0] == want


def test_refusals(K, ctx, plain, ptau13):
    """every refusal, each followed by a valid call on the same context"""
    ps = polys_of(3, 2, 12)
    mont = [Z.mont(p) for p in ps]
    good = [C.expected_proofs(p, 3, 1) for p in ps]
    L = K.lib()
    buf = ctypes.create_string_buffer(b"".join(mont), 512)
    out = ctypes.create_string_buffer(64 * 8 * 2)

    def refused(c, args, word, code=KGS_E_ARG):
        assert L.kgs_kzg_open_cosets_many(c.handle, *args) == code
        assert word in L.kgs_last_error().decode(), (word, L.kgs_last_error().decode())
        assert c.idle()
        if c is ctx:
            assert c.kzg_open_cosets_many(mont, 3, 1) == good and c.idle()

    # (coef, polys, stride, len, nbits, lbits, proofs, evals)
    for nbits in (-1, 24, 25):
        refused(ctx, (buf, 2, 8, 8, nbits, 0, out, None), "nbits")
    refused(ctx, (buf, 2, 8, 8, POWER + 1, 1, out, None), "nbits_max")
    for lbits in (-1, 4):
        refused(ctx, (buf, 2, 8, 8, 3, lbits, out, None), "lbits")
    refused(ctx, (buf, 2, 8, 8, 2, 1, out, None), "len")  # len > n
    refused(ctx, (buf, 2, 7, 8, 3, 1, out, None), "stride")  # stride < len
    refused(ctx, (buf, (1 << 21) + 1, 8, 8, 3, 1, out, None), "polys")  # polys * n > 2^24
    refused(ctx, (buf, 1 << 62, 8, 8, 3, 1, out, None), "polys")
    refused(ctx, (None, 2, 8, 8, 3, 1, out, None), "NULL")  # a NULL buffer with work to do
    refused(ctx, (buf, 2, 8, 8, 3, 1, None, None), "NULL")
    assert L.kgs_kzg_open_cosets_many(ctx.handle, None, 0, 0, 0, 3, 1, None, None) == 0  # polys == 0: nothing to do
    assert L.kgs_kzg_open_cosets_many(ctx.handle, None, 2, 0, 0, 3, 1, out, None) == 0 and out.raw == bytes(64 * 16)
    assert L.kgs_kzg_open_cosets_many(plain.handle, None, 0, 0, 0, 3, 1, None, None) == 0
    refused(plain, (buf, 2, 8, 8, 3, 1, out, None), "no SRS loaded", KGS_E_SRS)
    with pytest.raises(K.KgsError) as e:
        plain.kzg_open_cosets_many(mont, 3, 1)
    assert e.value.code == KGS_E_SRS and plain.idle()
    c = K.Context(0)
    try:
        c.load_ptau(ptau13, 10)
        call = lambda: c.kzg_open_cosets_many(mont, 3, 1)
        c.set_shard(0, 2, lambda b: b + b)
        with pytest.raises(K.KgsError) as e:
            call()
        assert e.value.code == KGS_E_ARG and "shard" in str(e.value)
        c.set_shard(0, 1)
        assert call() == good and c.idle()
        grp = K.Group.local(2)
        c.set_group(grp, 0)
        with pytest.raises(K.KgsError) as e:
            call()
        assert e.value.code == KGS_E_ARG and "rank group" in str(e.value)
        c.set_group(None)
        assert call() == good and c.idle()
        c.load_ptau(ptau13, 10, slice=(0, 2))
        with pytest.raises(K.KgsError) as e:
            call()
        assert e.value.code == KGS_E_ARG and "slice" in str(e.value) and c.idle()
        c.load_ptau(ptau13, 10)
        assert call() == good and c.idle()
    finally:
        c.close()


def test_module_level_entry_point(K, ptau13):
    """unequal lengths: the domain of the longest, the shorter ones zero-padded"""
    ps = [polys_of(5, 1, 13, count)[0] for count in (20, 32, 7, 1)]
    proofs, ev = K.kzg_open_cosets_many(ptau13, [Z.mont(p) for p in ps], 2)
    for b, p in enumerate(ps):
        assert proofs[b] == C.expected_proofs(p, 5, 2) and ev[b] == Z.mont(Z.evals(p, 5)), b
    assert K.kzg_open_cosets_many(ptau13, [], 2) == ([], [])
