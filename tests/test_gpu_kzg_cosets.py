"""Coset openings on the GPU: kgs_g1_mul_sum (the multiply-sum pass) as a primitive, with one case per branch of
the column sum; kgs_kzg_open_cosets byte for byte against the closed form over tau^i G at every (nbits, lbits)
up to 2^8, short polynomials, lbits = 0 against kgs_kzg_open_all, inputs built so that a column's terms are
equal or opposite, degenerate SRS, 2^12 by samples, a random functional and kgs_kzg_verify_coset, the cache
and the context contract."""
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
    path = f"/tmp/kgs_test_kzg_cosets_p{POWER}.{os.getpid()}.ptau"
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


def coefs(nbits, count, seed=0):
    rnd = random.Random(9000 + 100 * nbits + count + seed)
    return [rnd.randrange(R) for _ in range(count)]


# ------------------------------------------------------------------ g1_mul_sum as a primitive
SHAPES = [(rows, cols) for cols in (1, 63, 64, 65, 200) for rows in (1, 2, 3, 5, 8, 64) if rows * cols <= 1 << 12]
assert len(SHAPES) == 28 and (64, 64) in SHAPES and (64, 65) not in SHAPES


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 200])
def test_g1_mul_sum(K, plain, cols):
    """a partial wave, a whole block, one lane of a second block, several blocks; 1 .. 64 rows, not only powers
    of two: one pass of the sum by eights with a short last group (3, 5), one full group (8), two passes (64);
    identities among the points, the edge scalars of the recoding, scalars above r"""
    for rows in [r for r, c in SHAPES if c == cols]:
        mult, s = C.mul_sum_case(rows, cols, 40 + rows + cols)
        pts, sc = N.points(mult), N.scalar_bytes(s)
        want = C.mul_sum_expected(mult, s, rows)
        assert plain.g1_mul_sum(pts, sc, rows) == want, rows
        assert plain.idle()


def test_g1_mul_sum_paths_of_the_sum(K, plain):
    """a column whose terms are all equal (the doubling branch of add at the first sum, and at every level of
    the sum by eights: 2T + 2T ..), a column of pairs k P, (r - k) P (the sum passes through the identity), a
    column of identities only, a column of one term among identities"""
    for rows in (2, 8, 9, 64):
        mult, s = [], []
        for r in range(rows):
            mult += [3, 5, 0, 7 if r == rows - 1 else 0]
            s += [11, 9 if r % 2 == 0 else R - 9, 4 + r, 2]
        want = N.point(33 * rows) + (N.point(45) if rows % 2 else bytes(64)) + bytes(64) + N.point(14)
        assert plain.g1_mul_sum(N.points(mult), N.scalar_bytes(s), rows) == want, rows
        assert K.g1_mul_sum(N.points(mult), N.scalar_bytes(s), rows, device=None) == want
    assert plain.idle()


@pytest.mark.parametrize("rows", [1024, 1025])
def test_g1_mul_sum_two_rows_per_lane(K, plain, rows):
    """2^17 terms and more take the kernel that gives a lane two rows of a column (the shapes above take one row
    per lane): an even number of rows, and an odd one whose last group holds a single row. 16 distinct points,
    the identity among them, and few columns, so that the oracle's work is the 128 expected sums; a column of
    equal terms, one of opposite pairs and one of identities as above; three passes of the sum by eights."""
    cols = 128
    assert rows * cols >= 1 << 17
    rnd = random.Random(rows)
    base = [0, 1, 2, R - 1] + [rnd.randrange(R) for _ in range(12)]
    mult = [base[rnd.randrange(16)] for _ in range(rows * cols)]
    s = D.random_scalars(rows * cols, 600 + rows)
    for j, e in enumerate(Z.EDGE_SCALARS):
        s[(1 + 977 * j) % (rows * cols)] = e
    for r in range(rows):
        mult[r * cols:r * cols + 3] = [3, 5, 0]
        s[r * cols:r * cols + 3] = [11, 9 if r % 2 == 0 else R - 9, 4 + r]
    want = C.mul_sum_expected(mult, s, rows)
    assert want[:192] == N.point(33 * rows) + (N.point(45) if rows % 2 else bytes(64)) + bytes(64)
    assert plain.g1_mul_sum(N.points(mult), N.scalar_bytes(s), rows) == want
    assert plain.idle()


def test_g1_mul_sum_device_entry(K, plain):
    rows, cols = 5, 65
    mult, s = C.mul_sum_case(rows, cols, 7)
    pts, sc = N.points(mult), N.scalar_bytes(s)
    hip = _hip(K)
    dp, ds, do = DevBuf(hip, pts), DevBuf(hip, sc), DevBuf(hip, bytes(64 * cols))
    try:
        plain.g1_mul_sum_device(dp.p.value, ds.p.value, rows, cols, do.p.value)
        assert do.read() == C.mul_sum_expected(mult, s, rows)
        assert dp.read() == pts and ds.read() == sc  # the inputs are only read
    finally:
        for b in (dp, ds, do):
            b.free()
    assert plain.idle()


def test_g1_mul_sum_arguments(K, plain):
    assert plain.g1_mul_sum(b"", b"", 3) == b""
    L = K.lib()
    b = ctypes.create_string_buffer(128)
    assert L.kgs_g1_mul_sum(plain.handle, None, b, 2, 1, b) == KGS_E_ARG
    assert L.kgs_g1_mul_sum(plain.handle, b, b, 0, 2, b) == KGS_E_ARG
    assert L.kgs_g1_mul_sum(plain.handle, b, b, (1 << 13) + 1, 1 << 13, b) == KGS_E_ARG
    assert plain.idle()


# ------------------------------------------------------------------ every size, byte for byte
@pytest.mark.parametrize("nbits", range(9))
def test_every_size_against_the_closed_form(ctx, nbits):
    """every lbits 0 .. nbits: m = 1 (one identity), m = 2 (a transform of one stage), the partial transform of
    the cache with 1 .. nbits of its nbits + 1 stages, l Fr transforms of size 2 .. 2n"""
    n = 1 << nbits
    c = coefs(nbits, n)
    want_ev = Z.mont(Z.evals(c, nbits))
    for lbits in range(nbits + 1):
        proofs, ev = ctx.kzg_open_cosets(Z.mont(c), nbits, lbits, evals=True)
        assert proofs == N.points(C.closed_scalars(c, nbits, lbits)), lbits
        assert ev == want_ev, lbits
    assert ctx.idle()


def test_short_polynomials(ctx):
    nbits, lbits = 6, 2
    n, l, m = C.sizes(nbits, lbits)
    for count in (0, 1, l, l + 1, n - 1, n):
        c = coefs(nbits, count, 3)
        proofs, ev = ctx.kzg_open_cosets(Z.mont(c), nbits, lbits, evals=True)
        assert proofs == C.expected_proofs(c, nbits, lbits), count
        assert ev == Z.mont(Z.evals(c, nbits)), count
        if count <= l:
            assert proofs == bytes(64 * m)  # deg p < l: p is its own interpolant
    assert ctx.idle()


@pytest.mark.parametrize("nbits", range(9))
def test_lbits_zero_is_open_all(ctx, nbits):
    c = coefs(nbits, 1 << nbits, 5)
    a = ctx.kzg_open_all(Z.mont(c), nbits, evals=True)
    assert ctx.kzg_open_cosets(Z.mont(c), nbits, 0, evals=True) == a
    for lbits in range(1, nbits + 1):
        assert ctx.kzg_open_cosets(Z.mont(c), nbits, lbits, evals=True)[1] == a[1]
    assert ctx.kzg_open_cosets(Z.mont(c), nbits, 0) == a[0]  # no evaluations


# ------------------------------------------------------------------ structured inputs
def test_equal_and_opposite_columns_on_tau_one(K):
    """tau = 1: all s_k are G, so the l cached rows are the same points. Coefficients that do not depend on the
    row make every column's l terms equal; c_(ul+1) = -c_(ul) with the other rows zero makes them k P, -k P
    and identities. Against the long division, which holds for tau in the domain."""
    c = K.Context(0)
    try:
        with D.ptau_file("all_G", 5, "_cosets") as path:
            c.load_ptau(path, 5)
            for nbits, lbits in ((3, 1), (4, 2), (5, 3), (5, 4)):
                n, l, m = C.sizes(nbits, lbits)
                per = coefs(nbits, m, 13)
                same = [per[j // l] for j in range(n)]
                assert c.kzg_open_cosets(Z.mont(same), nbits, lbits) == \
                    N.points(C.division_scalars(same, nbits, lbits, 1)), (nbits, lbits)
                opp = [(per[j // l] if j % l == 0 else R - per[j // l] if j % l == 1 else 0) for j in range(n)]
                assert c.kzg_open_cosets(Z.mont(opp), nbits, lbits) == \
                    N.points(C.division_scalars(opp, nbits, lbits, 1)), (nbits, lbits)
            assert c.idle()
    finally:
        c.close()


@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_srs(K, name):
    tau = D.TAUS[name]
    c = K.Context(0)
    try:
        with D.ptau_file(name, 4, "_cosets") as path:
            c.load_ptau(path, 4)
            nbits = 3
            p = coefs(nbits, 1 << nbits, 31)
            for lbits in range(nbits + 1):
                assert c.kzg_open_cosets(Z.mont(p), nbits, lbits) == \
                    N.points(C.division_scalars(p, nbits, lbits, tau)), lbits
            assert c.idle()
    finally:
        c.close()


# ------------------------------------------------------------------ mid size
@pytest.mark.parametrize("lbits", [1, 6, 11, 12])
def test_mid_size(K, ctx, lbits):
    """16 sampled cosets byte for byte, a random functional of all m proofs in the exponent (the samples bound
    what a functional could hide), and every sampled proof through kgs_kzg_verify_coset"""
    nbits = 12
    n, l, m = C.sizes(nbits, lbits)
    c = coefs(nbits, n, 41)
    hip = _hip(K)
    dc, dp, de = DevBuf(hip, Z.mont(c)), DevBuf(hip, bytes(64 * m)), DevBuf(hip, bytes(32 * n))
    try:
        ctx.kzg_open_cosets_device(dc.p.value, n, nbits, lbits, dp.p.value, de.p.value)
        proofs, ev = dp.read(), de.read()
        assert dc.read() == Z.mont(c)  # the input is only read
    finally:
        for b in (dc, dp, de):
            b.free()
    want = C.closed_scalars(c, nbits, lbits)
    evals = Z.evals(c, nbits)
    assert ev == Z.mont(evals)
    r = D.random_scalars(m, 900 + lbits)
    assert ctx.msm_points(proofs, N.scalar_bytes(r)) == N.point(sum(a * b for a, b in zip(r, want)) % R)
    rnd = random.Random(lbits)
    sample = sorted({0, 1 % m, m - 1} | set(rnd.sample(range(m), min(13, m))))
    cm, t2, srs = Z.commitment(c), C.tau_l_g2(lbits), C.srs_g1(lbits)
    for i in sample:
        proof = proofs[64 * i:64 * i + 64]
        assert proof == N.point(want[i]), i
        ys = C.coset_values(evals, nbits, lbits, i)
        assert K.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, Z.mont(ys), proof) is True
        ys[rnd.randrange(l)] += 1
        assert K.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, Z.mont(ys), proof) is False
    assert ctx.idle()


# ------------------------------------------------------------------ cache and contract
def test_cached_rows_are_reused_and_coexist(K, ctx, ptau13):
    c = coefs(9, 512, 51)
    all9 = ctx.kzg_open_all(Z.mont(c), 9)  # the fk row of nbits 9
    assert ctx.kzg_open_cosets_cached(9, 0) and not ctx.kzg_open_cosets_cached(9, 3)
    first = ctx.kzg_open_cosets(Z.mont(c), 9, 3)
    assert first == N.points(C.closed_scalars(c, 9, 3))
    assert ctx.kzg_open_cosets_cached(9, 3) and not ctx.kzg_open_cosets_cached(9, 5)
    assert ctx.kzg_open_cosets(Z.mont(c), 9, 3) == first  # from the cache: a published row is never rebuilt
    assert ctx.kzg_open_cosets(Z.mont(c), 9, 9) == bytes(64) and not ctx.kzg_open_cosets_cached(9, 9)  # m = 1: no row
    assert ctx.kzg_open_cosets(b"", 9, 4) == bytes(64 * 32) and not ctx.kzg_open_cosets_cached(9, 4)  # len = 0: no row
    other9 = ctx.kzg_open_cosets(Z.mont(c), 9, 5)  # a second row of the same nbits
    assert other9 == N.points(C.closed_scalars(c, 9, 5))
    assert all(ctx.kzg_open_cosets_cached(9, lb) for lb in (0, 3, 5))
    assert ctx.kzg_open_cosets(Z.mont(c), 9, 3) == first and ctx.kzg_open_all(Z.mont(c), 9) == all9
    other = K.Context(0)
    try:
        other.load_ptau(ptau13, POWER)  # the same SRS tables: the rows are shared
        assert other.kzg_open_cosets_cached(9, 3)
        assert other.kzg_open_cosets(Z.mont(c), 9, 3) == first
    finally:
        other.close()
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
    lag = c.srs_lagrange(nbits)
    p = coefs(nbits, 1 << nbits, 61)
    all_ = c.kzg_open_all(Z.mont(p), nbits)
    for lbits in (1, nbits - 1):
        assert c.kzg_open_cosets(Z.mont(p), nbits, lbits) == C.expected_proofs(p, nbits, lbits) and c.idle()
    with pytest.raises(K.KgsError) as err:
        c.kzg_open_cosets(Z.mont(p), 12, 2)  # above the domain the SRS was loaded for
    assert err.value.code == KGS_E_ARG and c.idle()
    assert c.srs_info() == info and c.srs_lagrange(nbits) == lag and c.kzg_open_all(Z.mont(p), nbits) == all_
    assert _golden_proof(K)[0] == want


def test_refusals(K, ctx, plain, ptau13):
    p = Z.mont(coefs(3, 8))
    for nbits in (-1, 24, 25):
        with pytest.raises(K.KgsError) as e:
            ctx.kzg_open_cosets(p, nbits, 0)
        assert e.value.code == KGS_E_ARG and "nbits" in str(e.value) and ctx.idle()
    for lbits in (-1, 4):
        with pytest.raises(K.KgsError) as e:
            ctx.kzg_open_cosets(p, 3, lbits)
        assert e.value.code == KGS_E_ARG and "lbits" in str(e.value) and ctx.idle()
    with pytest.raises(K.KgsError) as e:
        ctx.kzg_open_cosets(p, POWER + 1, 1)
    assert e.value.code == KGS_E_ARG and "nbits_max" in str(e.value) and ctx.idle()
    with pytest.raises(K.KgsError) as e:
        ctx.kzg_open_cosets(p, 2, 1)
    assert e.value.code == KGS_E_ARG and "len" in str(e.value) and ctx.idle()
    L = K.lib()
    out = ctypes.create_string_buffer(64 * 8)
    assert L.kgs_kzg_open_cosets(ctx.handle, None, 8, 3, 1, out, None) == KGS_E_ARG  # a NULL buffer with work to do
    assert L.kgs_kzg_open_cosets(ctx.handle, p, 8, 3, 1, None, None) == KGS_E_ARG and ctx.idle()
    with pytest.raises(K.KgsError) as e:
        plain.kzg_open_cosets(p, 3, 1)
    assert e.value.code == KGS_E_SRS and "no SRS loaded" in str(e.value) and plain.idle()
    c = K.Context(0)
    try:
        c.load_ptau(ptau13, 10)
        calls = (lambda: c.kzg_open_cosets(p, 3, 1), lambda: c.g1_mul_sum(N.point(1), bytes(32), 1))
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
        assert c.kzg_open_cosets(p, 3, 1) == C.expected_proofs(Z.from_mont(p), 3, 1) and c.idle()
        c.load_ptau(ptau13, 10, slice=(0, 2))
        with pytest.raises(K.KgsError) as e:
            calls[0]()
        assert e.value.code == KGS_E_ARG and "slice" in str(e.value) and c.idle()
    finally:
        c.close()


def test_module_level_entry_points(K, ptau13):
    c = coefs(5, 20, 71)  # 20 coefficients: the domain of 32 points
    proofs, ev = K.kzg_open_cosets(ptau13, Z.mont(c), 2)
    assert proofs == C.expected_proofs(c, 5, 2) and ev == Z.mont(Z.evals(c, 5))
    mult, s = C.mul_sum_case(3, 9, 3)
    assert K.g1_mul_sum(N.points(mult), N.scalar_bytes(s), 3) == C.mul_sum_expected(mult, s, 3)
    ys = C.coset_values(Z.evals(c, 5), 5, 2, 7)
    args = (C.srs_g1(2), Z.commitment(c), 5, 2, 7, Z.mont(ys))
    assert K.kzg_verify_coset(C.tau_l_g2(2), *args, proofs[64 * 7:64 * 8]) is True
    assert K.kzg_verify_coset(C.tau_l_g2(2), *args, proofs[64 * 6:64 * 7]) is False
    with pytest.raises(K.KgsError):  # the synthetic ptau stores two G2 points: no [tau^4]_2 in it
        K.kzg_verify_coset(ptau13, *args, proofs[64 * 7:64 * 8])
