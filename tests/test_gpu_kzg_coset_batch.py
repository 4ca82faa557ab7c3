"""The batch verifier for coset openings on the GPU: kgs_coset_interp_fold against the integer
reference at every fused size, row count shape, index and weight edge; kgs_kzg_verify_cosets_batch on the GPU path
against the host path and the integer references byte for byte (openings made by kgs_kzg_open_cosets, the CPU
cases again, both routes of the point sums, a mid-size batch with tampered openings), the device twins, the
context contract and the refusals."""
import ctypes
import json
import os
import random

import pytest

import common
import g1_ntt_cases as N
import kzg_coset_batch_cases as B
import kzg_coset_cases as C
import kzg_open_cases as Z
import test_kzg_coset_batch_refs as T

pytestmark = pytest.mark.gpu
R = N.R
KGS_E_ARG = -1
POWER = 13
FUSED_MAX = 10  # kernels.hpp COSET_FOLD_LBITS_MAX
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(autouse=True)
def force_gpu(monkeypatch):
    """the folds of every batch in this module run on the GPU, however small"""
    monkeypatch.setenv("KGS_VERIFY_COSETS_FOLD", "gpu")
    monkeypatch.delenv("KGS_VERIFY_COSETS_MSM", raising=False)


@pytest.fixture(scope="module")
def ptau13(K):
    path = f"/tmp/kgs_test_kzg_coset_batch_p{POWER}.{os.getpid()}.ptau"
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
    """a context without an SRS: the verifier needs none on the device"""
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


# ------------------------------------------------------------------ kgs_coset_interp_fold
COUNTS = (1, 2, 3, 63, 64, 65, 200, 1000)
EDGE = (0, 1, R - 1)


def fold_case(nbits, lbits, count, seed):
    """indices 0, 1, m - 1, repeated and random; values 0, 1, r - 1 and random; weights 1, r - 1, 0 and random"""
    n, l, m = C.sizes(nbits, lbits)
    rnd = random.Random(seed)
    fixed = [0, 1 % m, m - 1, m - 1, 0]
    index = [fixed[k] if k < 5 else rnd.choice((0, 1 % m, m - 1, rnd.randrange(m))) for k in range(count)]
    rows = [[EDGE[(k + j) % 3] for j in range(l)] if k % 7 == 1 else [rnd.randrange(R) for _ in range(l)]
            for k in range(count)]
    weights = [(1, R - 1, 0)[k % 3] if k < 3 or k % 11 == 0 else rnd.randrange(R) for k in range(count)]
    return index, rows, weights


def flat(rows):
    return Z.mont([y for row in rows for y in row])


@pytest.mark.parametrize("lbits", range(FUSED_MAX + 1))
def test_interp_fold(plain, lbits):
    """every fused size at nbits = max(lbits, 12). A tile is max(1, 512 / l) rows: the counts give a partial tile,
    a whole one, one row of a second block and several blocks whose partial sums the second launch reduces (at
    l = 1 the 1000 rows, at l >= 512 every count above 1). count * l stays below 2^18 for the integer reference."""
    nbits = max(lbits, 12)
    l = 1 << lbits
    for count in [c for c in COUNTS if c * l <= 1 << 18]:
        index, rows, weights = fold_case(nbits, lbits, count, 100 * lbits + count)
        got = plain.coset_interp_fold(nbits, lbits, index, flat(rows), Z.mont(weights))
        assert got == Z.mont(B.interp_fold_reference_grouped(nbits, lbits, index, rows, weights)), count
        assert plain.idle()


def test_interp_fold_small_domains_and_host(K, plain):
    """lbits = nbits (m = 1, every index 0), nbits = 0, and the host path on the same inputs"""
    for nbits, lbits in ((0, 0), (1, 1), (3, 3), (6, 2), (10, 10)):
        index, rows, weights = fold_case(nbits, lbits, 5, nbits + lbits)
        want = Z.mont(B.interp_fold_reference(nbits, lbits, index, rows, weights))
        assert plain.coset_interp_fold(nbits, lbits, index, flat(rows), Z.mont(weights)) == want, (nbits, lbits)
        assert K.coset_interp_fold(nbits, lbits, index, flat(rows), Z.mont(weights), device=None) == want
    assert plain.coset_interp_fold(4, 2, [], b"", b"") == bytes(32 * 4) and plain.idle()


def test_interp_fold_blocks_that_take_several_tiles(plain):
    """more tiles than the 1024 blocks of a launch: l = 32, 16 rows a tile, 16 * 1024 + 5 rows. The rows cycle
    through three vectors, so the reference is three combinations"""
    nbits, lbits = 12, 5
    n, l, m = C.sizes(nbits, lbits)
    count = 16 * 1024 + 5
    rnd = random.Random(5)
    vecs = [[rnd.randrange(R) for _ in range(l)] for _ in range(3)]
    vb = [Z.mont(v) for v in vecs]
    index = [(0, 1, m - 1)[k % 3] for k in range(count)]
    weights = [rnd.randrange(R) for _ in range(count)]
    want = [0] * l
    for r in range(3):
        ws = sum(weights[r::3]) % R
        want = [(a + ws * b) % R for a, b in zip(want, C.interpolant(vecs[r], nbits, lbits, index[r]))]
    got = plain.coset_interp_fold(nbits, lbits, index, b"".join(vb[k % 3] for k in range(count)), Z.mont(weights))
    assert got == Z.mont(want) and plain.idle()


def test_interp_fold_above_the_fused_sizes(K, plain):
    """l = 2^11 is not built on the GPU: a context refuses it and stays idle, the host computes it"""
    nbits = lbits = FUSED_MAX + 1
    index, rows, weights = fold_case(nbits, lbits, 2, 3)
    with pytest.raises(K.KgsError) as e:
        plain.coset_interp_fold(nbits, lbits, index, flat(rows), Z.mont(weights))
    assert e.value.code == KGS_E_ARG and "lbits" in str(e.value) and plain.idle()
    assert K.coset_interp_fold(nbits, lbits, index, flat(rows), Z.mont(weights), device=None) == \
        Z.mont(B.interp_fold_reference(nbits, lbits, index, rows, weights))


def test_interp_fold_refusals(K, plain):
    index, rows, weights = fold_case(6, 2, 4, 9)
    ys, w = flat(rows), Z.mont(weights)
    big = bytearray(ys)
    big[32 * 5:32 * 6] = R.to_bytes(32, "little")
    for args in (([16] + index[1:], ys, w), (index, bytes(big), w), (index, ys, w[:32] + R.to_bytes(32, "little") + w[64:])):
        with pytest.raises(K.KgsError) as e:
            plain.coset_interp_fold(6, 2, *args)
        assert e.value.code == KGS_E_ARG and plain.idle()
    for nbits, lbits in ((24, 2), (3, 4), (3, -1)):
        with pytest.raises(K.KgsError) as e:
            plain.coset_interp_fold(nbits, lbits, [], b"", b"")
        assert e.value.code == KGS_E_ARG and plain.idle()


def test_interp_fold_device(K, plain):
    hip = _hip(K)
    nbits, lbits, count = 12, 6, 70
    index, rows, weights = fold_case(nbits, lbits, count, 77)
    ins = [b"".join(i.to_bytes(8, "little") for i in index), flat(rows), Z.mont(weights)]
    bufs = [DevBuf(hip, x) for x in ins]
    out = DevBuf(hip, bytes(32 << lbits))
    try:
        plain.coset_interp_fold_device(nbits, lbits, bufs[0].p, bufs[1].p, bufs[2].p, count, out.p)
        assert out.read() == Z.mont(B.interp_fold_reference_grouped(nbits, lbits, index, rows, weights))
        assert [b.read() for b in bufs] == ins and plain.idle()  # the inputs are only read
    finally:
        for b in bufs + [out]:
            b.free()


# ------------------------------------------------------------------ the batch on the GPU path
def run_gpu(c, batch, **kw):
    diag = {}
    got = c.kzg_verify_cosets_batch(batch.tau_l_g2(), batch.srs(), batch.nbits, batch.lbits, batch.commits(),
                                    batch.tuples(), diag=diag, **kw)
    assert c.idle()
    return got, diag


def same_as_host(c, batch, seed=None):
    """the GPU path and the host path agree byte for byte, and with the integer references"""
    g, gd = run_gpu(c, batch, seed=seed)
    h, hd = T.run(batch, seed=seed)
    assert gd["on_gpu"] == 1 and hd["on_gpu"] == 0
    assert g == h and all(gd[x] == hd[x] for x in ("rho", "interp", "folded", "pairing_checks"))
    T.check_against_references(batch, g, gd, seed=seed)
    assert run_gpu(c, batch, seed=seed, locate=False)[0] is all(h)
    return g, gd


def test_cpu_cases_on_the_gpu(plain):
    base = T.base_batch()
    ops = base.openings
    n, l, m = C.sizes(base.nbits, base.lbits)
    y1 = list(ops[3][2])
    y1[1] = (y1[1] + 1) % R
    big = list(ops[4][2])
    big[l - 1] = R
    delta = 999
    cases = {
        "valid": (base, 0),
        "one value off by one": (T.with_opening(base, 3, ys=y1), 1),
        "the neighbouring coset's proof": (T.with_opening(base, 5, pi=ops[6][3]), 1),
        "the other polynomial's commitment": (T.with_opening(base, 2, ci=1), 1),
        "errors that cancel without weights": (T.with_opening(T.with_opening(base, 1, pi=ops[1][3] + delta), 5,
                                                              pi=ops[5][3] - delta), 2),
        "a value of r": (T.with_opening(base, 4, ys=big), 1),
        "an index of m": (T.with_opening(base, 0, i=m), 1),
        "commit_of = ncommits": (T.with_opening(base, 7, ci=2), 1),
    }
    for name, (batch, bad) in cases.items():
        got, diag = same_as_host(plain, batch)
        assert got.count(False) == bad, name
    same_as_host(plain, base, seed=bytes(range(32)))
    low = T.coefs(4, 3, 3)  # identity proofs, and the zero polynomial under the identity commitment
    same_as_host(plain, B.valid_batch(4, 2, [low, []], [(0, 0), (0, 3), (1, 1), (1, 2)]))
    for nbits, lbits in ((3, 0), (3, 3), (5, 2)):  # count = 1
        c = T.coefs(nbits, 1 << nbits, 2)
        one = B.valid_batch(nbits, lbits, [c], [(0, (1 << (nbits - lbits)) - 1)])
        assert same_as_host(plain, one)[0] == [True]
        assert same_as_host(plain, T.with_opening(one, 0, pi=one.openings[0][3] + 1))[0] == [False]


def test_points_off_the_curve_on_the_gpu(K, plain):
    base = T.base_batch()
    t = base.tuples()
    off = bytearray(t[2][3])
    off[5] ^= 1
    t[2] = t[2][:3] + (bytes(off),)
    noncanon = (int.from_bytes(t[3][3][:32], "little") + N.bn.Q).to_bytes(32, "little") + t[3][3][32:]
    t[3] = t[3][:3] + (noncanon,)  # x + q: the same point, not canonical
    args = (base.tau_l_g2(), base.srs(), base.nbits, base.lbits)
    for tuples, cm, want in ((t, base.commits(), [j not in (2, 3) for j in range(len(t))]),
                             (base.tuples(), [base.commits()[0], bytes(off)], [ci == 0 for ci, _, _, _ in base.openings])):
        dg, dh = {}, {}
        got = plain.kzg_verify_cosets_batch(*args, cm, tuples, diag=dg)
        assert got == want and got == K.kzg_verify_cosets_batch(*args, cm, tuples, device=None, diag=dh)
        assert dg["on_gpu"] == 1 and dg["pairing_checks"] == dh["pairing_checks"] == 1
        assert all(dg[x] == dh[x] for x in ("rho", "interp", "folded")) and plain.idle()
    srs = bytearray(base.srs())
    srs[3] ^= 1
    assert plain.kzg_verify_cosets_batch(args[0], bytes(srs), *args[2:], base.commits(), base.tuples()) == \
        [False] * len(t) and plain.idle()
    assert plain.kzg_verify_cosets_batch(*args, base.commits(), []) == [] and plain.idle()


@pytest.fixture(scope="module")
def opened(ctx):
    """128 openings made by kgs_kzg_open_cosets: nbits 8, lbits 3, 4 polynomials, every coset; the commitment of
    polynomial 0 is in the list twice (entries 0 and 4) and polynomial 0's odd cosets point at the second"""
    nbits, lbits = 8, 3
    n, l, m = C.sizes(nbits, lbits)
    polys = [T.coefs(nbits, n, 80 + p) for p in range(4)]
    commits = [Z.commitment(c) for c in polys]
    commits.append(commits[0])
    tuples = []
    for p, c in enumerate(polys):
        proofs, ev = ctx.kzg_open_cosets(Z.mont(c), nbits, lbits, evals=True)
        for i in range(m):
            ys = b"".join(ev[32 * (i + m * j):32 * (i + m * j + 1)] for j in range(l))
            tuples.append((4 if p == 0 and i % 2 else p, i, ys, proofs[64 * i:64 * (i + 1)]))
    return nbits, lbits, commits, tuples


def both(K, c, nbits, lbits, commits, tuples, **kw):
    args = (C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits, tuples)
    dg, dh = {}, {}
    g = c.kzg_verify_cosets_batch(*args, diag=dg, **kw)
    assert c.idle()
    h = K.kzg_verify_cosets_batch(*args, device=None, diag=dh, **kw)
    assert g == h and dg["on_gpu"] == 1 and dh["on_gpu"] == 0
    assert all(dg[x] == dh[x] for x in ("rho", "interp", "folded", "pairing_checks"))
    return g, dg


def test_openings_of_kzg_open_cosets(K, ctx, opened):
    nbits, lbits, commits, tuples = opened
    g, d = both(K, ctx, nbits, lbits, commits, tuples)
    assert g == [True] * 128 and d["pairing_checks"] == 1
    bad = list(tuples)
    bad[77] = (bad[77][0], bad[77][1], bad[77][2], tuples[78][3])
    g, d = both(K, ctx, nbits, lbits, commits, bad)
    assert g == [k != 77 for k in range(128)] and 1 < d["pairing_checks"] <= B.check_bound(1, 128)


@pytest.mark.parametrize("count", [82, 83])
def test_both_routes_of_the_point_sums(K, ctx, opened, count, monkeypatch):
    """A and B by kgs_msm_points' buckets (what every size takes: measured faster everywhere) and,
    forced, by kgs_g1_lincomb's fold: the same bytes, at 254 and 257 terms (3 count + l)"""
    nbits, lbits, commits, tuples = opened
    g, d = both(K, ctx, nbits, lbits, commits, tuples[:count])
    assert g == [True] * count
    for route in ("fold", "points"):
        monkeypatch.setenv("KGS_VERIFY_COSETS_MSM", route)
        g2, d2 = both(K, ctx, nbits, lbits, commits, tuples[:count])
        assert g2 == g and d2["folded"] == d["folded"], route
    bad = list(tuples[:count])
    bad[7] = bad[7][:3] + (tuples[8][3],)
    monkeypatch.setenv("KGS_VERIFY_COSETS_MSM", "fold")  # the bisection's sub-ranges through the fold as well
    assert both(K, ctx, nbits, lbits, commits, bad)[0] == [k != 7 for k in range(count)]


def test_mid_size_batch(K, ctx):
    """nbits 12, lbits 6: all 64 cosets of 8 polynomials, 512 openings; valid, then three tampered (a value, a
    proof exchanged, a commitment exchanged) spread over the batch"""
    nbits, lbits = 12, 6
    n, l, m = C.sizes(nbits, lbits)
    polys = [T.coefs(nbits, n, 120 + p) for p in range(8)]
    commits = [Z.commitment(c) for c in polys]
    tuples = []
    for p, c in enumerate(polys):
        proofs, ev = ctx.kzg_open_cosets(Z.mont(c), nbits, lbits, evals=True)
        for i in range(m):
            ys = b"".join(ev[32 * (i + m * j):32 * (i + m * j + 1)] for j in range(l))
            tuples.append((p, i, ys, proofs[64 * i:64 * (i + 1)]))
    assert len(tuples) == 512
    g, d = both(K, ctx, nbits, lbits, commits, tuples)
    assert g == [True] * 512 and d["pairing_checks"] == 1
    bad = list(tuples)
    y = bytearray(bad[5][2])
    y[32 * 9:32 * 10] = Z.mont([7])
    bad[5] = bad[5][:2] + (bytes(y), bad[5][3])
    bad[300] = bad[300][:3] + (tuples[301][3],)
    bad[511] = (0,) + bad[511][1:]
    dg = {}
    got = ctx.kzg_verify_cosets_batch(C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits, bad, diag=dg)
    assert got == [k not in (5, 300, 511) for k in range(512)] and ctx.idle()
    assert dg["on_gpu"] == 1 and 1 < dg["pairing_checks"] <= B.check_bound(3, 512) == 55
    assert ctx.kzg_verify_cosets_batch(C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits, bad,
                                       locate=False) is False and ctx.idle()


def test_default_routing(K, plain, opened, monkeypatch):
    """without the override a context folds a batch below 24 terms on the host, a larger one on the GPU"""
    monkeypatch.delenv("KGS_VERIFY_COSETS_FOLD", raising=False)
    nbits, lbits, commits, tuples = opened
    args = (C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits)
    for count, on_gpu in ((5, 0), (6, 1)):  # 3 * 5 + 8 = 23, 3 * 6 + 8 = 26
        d = {}
        assert plain.kzg_verify_cosets_batch(*args, tuples[:count], diag=d) == [True] * count
        assert d["on_gpu"] == on_gpu and plain.idle()
    monkeypatch.setenv("KGS_VERIFY_COSETS_FOLD", "host")
    d = {}
    assert plain.kzg_verify_cosets_batch(*args, tuples, diag=d) == [True] * 128 and d["on_gpu"] == 0


def test_cosets_above_the_fused_sizes_fold_on_the_host(K, plain):
    nbits = lbits = FUSED_MAX + 1
    c = T.coefs(nbits, 5, 1)  # deg < l: the proof is the identity
    ys = Z.mont(Z.evals(c, nbits))
    d = {}
    got = plain.kzg_verify_cosets_batch(C.tau_l_g2(lbits), N.points(N.tau_powers(5)) + bytes(64 * ((1 << lbits) - 5)),
                                        nbits, lbits, [Z.commitment(c)], [(0, 0, ys, bytes(64))], diag=d)
    assert got == [True] and d["on_gpu"] == 0 and plain.idle()


# ------------------------------------------------------------------ the device twin
def test_device_twin(K, ctx, opened):
    hip = _hip(K)
    nbits, lbits, commits, tuples = opened
    bad = list(tuples)
    bad[100] = bad[100][:3] + (tuples[3][3],)
    seed = bytes(range(7, 39))
    for ts, want in ((tuples, [True] * 128), (bad, [k != 100 for k in range(128)])):
        ins = [b"".join(t[0].to_bytes(4, "little") for t in ts), b"".join(t[1].to_bytes(8, "little") for t in ts),
               b"".join(t[2] for t in ts), b"".join(t[3] for t in ts)]
        bufs = [DevBuf(hip, x) for x in ins]
        try:
            dg, dh = {}, {}
            got = ctx.kzg_verify_cosets_batch_device(C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits,
                                                     bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, 128, seed, diag=dg)
            assert got == want and ctx.idle() and dg["on_gpu"] == 1
            assert [b.read() for b in bufs] == ins  # the inputs are only read
            assert K.kzg_verify_cosets_batch(C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits, ts, device=None,
                                             seed=seed, diag=dh) == want
            assert all(dg[x] == dh[x] for x in ("rho", "interp", "folded", "pairing_checks"))
            assert dg["rho"] == B.rho_of(seed).to_bytes(32, "little")
        finally:
            for b in bufs:
                b.free()
    L = K.lib()
    t2, srs = C.tau_l_g2(lbits), C.srs_g1(lbits)
    assert L.kgs_kzg_verify_cosets_batch_device(ctx.handle, nbits, lbits, b"".join(commits), 5, 64, 64, 64, 64, 1, srs,
                                                t2, None, None, None) == KGS_E_ARG  # no seed
    assert "seed" in L.kgs_last_error().decode() and ctx.idle()


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


def test_context_state_is_left_alone(K):
    got, want, nbits = _golden_proof(K)
    assert got == want
    c = K._context(0)  # the context the module-level prover keeps the SRS on
    info = c.srs_info()
    lag = c.srs_lagrange(nbits)
    p = T.coefs(nbits, 1 << nbits, 61)
    lb = 1 if nbits >= 2 else 0  # lbits = 0: kgs_kzg_open_all's row
    row = c.kzg_open_cosets(Z.mont(p), nbits, lb)
    assert c.kzg_open_cosets_cached(nbits, lb)
    base = T.base_batch()
    assert run_gpu(c, base)[0] == [True] * len(base.openings)
    assert run_gpu(c, T.with_opening(base, 3, pi=5))[0] == [k != 3 for k in range(len(base.openings))]
    index, rows, weights = fold_case(12, 4, 40, 1)
    assert c.coset_interp_fold(12, 4, index, flat(rows), Z.mont(weights)) == \
        Z.mont(B.interp_fold_reference_grouped(12, 4, index, rows, weights)) and c.idle()
    with pytest.raises(K.KgsError) as err:
        c.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), 24, 2, base.commits(), base.tuples())
    assert err.value.code == KGS_E_ARG and c.idle()
    assert c.srs_info() == info and c.srs_lagrange(nbits) == lag and c.kzg_open_cosets_cached(nbits, lb)
    assert c.kzg_open_cosets(Z.mont(p), nbits, lb) == row
    assert _golden_proof(K)[0] == want


def test_refusals(K, ptau13):
    base = T.base_batch()
    index, rows, weights = fold_case(6, 2, 4, 9)
    c = K.Context(0)
    try:
        calls = (lambda: c.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), base.nbits, base.lbits, base.commits(),
                                                   base.tuples()),
                 lambda: c.coset_interp_fold(6, 2, index, flat(rows), Z.mont(weights)))
        c.load_ptau(ptau13, 10)
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
        assert c.idle() and calls[0]() == [True] * len(base.openings) and c.idle()
        off = bytearray(base.tau_l_g2())
        off[3] ^= 1
        with pytest.raises(K.KgsError) as e:
            c.kzg_verify_cosets_batch(bytes(off), base.srs(), base.nbits, base.lbits, base.commits(), base.tuples())
        assert e.value.code == KGS_E_ARG and c.idle()
    finally:
        c.close()
