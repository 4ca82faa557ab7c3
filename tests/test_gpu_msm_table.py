"""The fixed-base MSM's scaled window table on the GPU (csrc/msm.hip msm_build_table, scalar_digits,
k_accumulate<*, ZP>): row 0 holds 2^-256 P_i, the digits are read off the scalars' Montgomery words,
and a table without zero points runs the bucket accumulation without its affine-infinity test.

Every `ctx.msm(Montgomery words)` is compared byte for byte with `ctx.msm_points(points, standard
forms)`: the variable-base MSM has no table, takes standard forms and reduces them itself, so it
shares neither the scaling of the table nor the digit change.

The files are synthetic ptau files of power 8 (511 points, window 7) and 11 (4095 points, window 8)
from the product's own writer; the power-11 points are loaded a second time under KGS_MSM_C=17, the
headline window, from a copy of the file (the table cache is keyed by the file, not by the window).
"""
import contextlib
import ctypes
import json
import os
import random
import shutil

import pytest

import common
from oracle import bn254 as bn
from oracle import ptau as opt
from test_gpu_dist import run_group, single

pytestmark = pytest.mark.gpu
R = bn.R
Q = bn.Q
MONT = 1 << 256
RHO = pow(MONT, -1, R)
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))
# (power, KGS_MSM_C or None, expected window)
LOADS = [(8, None, 7), (11, None, 8), (11, 17, 17)]
LOAD_IDS = ["p8", "p11", "p11-c17"]


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ref_ctx(K):
    """the context of the reference side (msm_points): no SRS of its own"""
    c = K.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(K, ref_ctx):
    """{(power, c): path} and {power: points bytes}; the c = 17 load reads a copy of the file"""
    paths, points = {}, {}
    try:
        for power in (8, 11):
            p = f"/tmp/kgs_test_msm_table_p{power}.{os.getpid()}.ptau"
            ref_ctx.write_synthetic_ptau(p, power, common.tau())
            paths[(power, None)] = p
            points[power] = opt.PTau(p).g1_bytes
        paths[(11, 17)] = paths[(11, None)] + ".c17"
        shutil.copyfile(paths[(11, None)], paths[(11, 17)])
        yield paths, points
    finally:
        for p in paths.values():
            if os.path.exists(p):
                os.remove(p)


@contextlib.contextmanager
def loaded(K, path, c_env, monkeypatch, want_c=None, **kw):
    if c_env is None:
        monkeypatch.delenv("KGS_MSM_C", raising=False)
    else:
        monkeypatch.setenv("KGS_MSM_C", str(c_env))
    ctx = K.Context(0)
    try:
        ctx.load_ptau(path, **kw)
        if want_c is not None:
            assert ctx.srs_info()[2] == want_c
        yield ctx
    finally:
        ctx.close()


def zero_points(K, ctx):
    """kgs_srs_zero_points: whether the resident table is flagged as holding a zero point"""
    z = ctypes.c_int(-2)
    assert K.lib().kgs_srs_zero_points(ctx._h, ctypes.byref(z)) == 0
    return z.value


def words(vals):
    """integers below 2^256 as 32 B little-endian words, as they are"""
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def windows(c):
    return (255 + c - 1) // c


def scalar_sets(n, c):
    """(id, Montgomery integers s_i of n scalars); the standard forms are k_i = s_i 2^-256 mod r.

    `half`: every window below the top of the Montgomery integer holds 2^(c-1), the one digit that is
    key B, without a carry. `most-negative`: window 0 holds 2^(c-1) + 1 and every other one below the
    top 2^(c-1), so each becomes the digit -(2^(c-1) - 1) with a carry into the next, up to the top
    window's +1: the recoding's digits lie in [-(2^(c-1) - 1), 2^(c-1)], so -2^(c-1) itself does not
    occur."""
    rnd = random.Random(1000 * c + n)
    half = 1 << (c - 1)
    low = range(windows(c) - 1)
    s_half = sum(half << (c * j) for j in low)
    s_neg = s_half + 1
    assert 0 < s_half < s_neg < R
    mont = lambda k: k * MONT % R
    one_hot = lambda i: [mont(rnd.randrange(1, R)) if j == i else 0 for j in range(n)]
    return [
        ("random", [mont(rnd.randrange(R)) for _ in range(n)]),
        ("zeros", [0] * n),
        ("ones", [mont(1)] * n),
        ("r-1", [mont(R - 1)] * n),
        ("half", [s_half] * n),
        ("most-negative", [s_neg] * n),
        ("half-among-random", [s_half if i % 3 == 0 else s_neg if i % 3 == 1 else mont(rnd.randrange(R))
                               for i in range(n)]),
        ("first-only", one_hot(0)),
        ("last-only", one_hot(n - 1)),
    ]


def check(ctx, ref_ctx, pts, s, what):
    """ctx.msm over the Montgomery integers s == msm_points over their standard forms, on a two-lane
    (k_accumulate<2, *>) and on a one-lane (k_accumulate<3, *>) context"""
    n = len(s)
    want = ref_ctx.msm_points(pts[:64 * n], words([x * RHO % R for x in s]))
    for lanes in (2, 1):
        ctx.set_msm_lanes(lanes)
        assert ctx.msm(words(s)) == want, (what, n, lanes)
    ctx.set_msm_lanes(2)
    return want


# ------------------------------------------------------------------ clean SRS: the flag-free kernel
@pytest.mark.parametrize("power,c_env,c", LOADS, ids=LOAD_IDS)
def test_scaled_table_matches_msm_points(K, ref_ctx, files, monkeypatch, power, c_env, c):
    paths, points = files
    npts = (2 << power) - 1
    with loaded(K, paths[(power, c_env)], c_env, monkeypatch, c) as ctx:
        assert ctx.srs_info()[1] == npts
        assert zero_points(K, ctx) == 0  # tau^i G: no zero point, the test-free accumulate runs
        seen = set()
        for n in (npts, 513 if power > 8 else 257, 1):  # every point; past one sort block (512 scalars); one
            for what, s in scalar_sets(n, c):
                got = check(ctx, ref_ctx, points[power], s, what)
                seen.add(got)
                if what == "zeros":
                    assert got == bytes(64)
        assert len(seen) > 6  # the sets are not all the same point


@pytest.mark.parametrize("power,c_env,c", LOADS[:2], ids=LOAD_IDS[:2])
def test_two_lane_tail_matches_msm_points(K, ref_ctx, files, monkeypatch, power, c_env, c):
    """a two-lane context reduces its buckets with the block-tree k_rowcol on a grid of one window
    (gridDim.y = 1), msm_points with k_rowcol16 on a grid of W windows: the same tail kernels, and the
    same bytes, for both parities of c (c = 7: l = 3, h = 3; c = 8: l = 4, h = 3)"""
    paths, points = files
    npts = (2 << power) - 1
    rnd = random.Random(77 + c)
    with loaded(K, paths[(power, c_env)], c_env, monkeypatch, c) as ctx:
        ctx.set_msm_lanes(2)
        k = rnd.randrange(1, R)
        for what, s in (("random", [rnd.randrange(R) for _ in range(npts)]), ("all-equal", [k] * npts)):
            want = ref_ctx.msm_points(points[power][:64 * npts], words([x * RHO % R for x in s]))
            assert want != bytes(64)
            assert ctx.msm(words(s)) == want, (what, c)


# ------------------------------------------------------------------ degenerate SRS: the flagged kernel
def neg_lem(p):
    y = int.from_bytes(p[32:], "little")
    return p[:32] + ((Q - y) % Q).to_bytes(32, "little")


def degenerate_points(pts, npts):
    """the file's points with a zero point at index 0, in the middle and at the last index, a repeated
    pair (5, 6) and an opposite pair (9, 10); -> bytes"""
    P = [pts[64 * i:64 * i + 64] for i in range(npts)]
    for i in (0, npts // 2, npts - 1):
        P[i] = bytes(64)
    P[6] = P[5]
    P[10] = neg_lem(P[9])
    return b"".join(P)


def patched_file(path, old, new, tag):
    """a copy of the ptau at `path` whose G1 section `old` is replaced by `new`"""
    data = open(path, "rb").read()
    at = data.index(old)
    assert data.count(old) == 1 and len(old) == len(new)
    out = f"{path}.{tag}"
    with open(out, "wb") as fh:
        fh.write(data[:at] + new + data[at + len(old):])
    return out


@pytest.mark.parametrize("power,c_env,c", LOADS, ids=LOAD_IDS)
def test_zero_repeated_and_opposite_points(K, ref_ctx, files, monkeypatch, power, c_env, c):
    paths, points = files
    npts = (2 << power) - 1
    bad = degenerate_points(points[power], npts)
    path = patched_file(paths[(power, None)], points[power], bad, f"degen{c_env}")
    try:
        with loaded(K, path, c_env, monkeypatch, c) as ctx:
            assert zero_points(K, ctx) == 1  # the accumulate with the affine-infinity test runs
            for what, s in scalar_sets(npts, c):
                check(ctx, ref_ctx, bad, s, what)
            # the same scalar on the repeated and on the opposite pair: the equal and the opposite
            # branch of the add, whatever order the sort leaves
            k = 0x1234567 * MONT % R
            s = [0] * 16
            s[5] = s[6] = s[9] = s[10] = k
            check(ctx, ref_ctx, bad, s, "pairs")
            s[9] = s[10] = 0
            check(ctx, ref_ctx, bad, s, "repeated")
            # nothing but zero points selected
            s = [0] * npts
            s[0] = s[npts // 2] = s[npts - 1] = k
            assert check(ctx, ref_ctx, bad, s, "only-zero-points") == bytes(64)
        # a single zero point anywhere raises the flag
        for i in (0, npts - 1):
            one = points[power][:64 * i] + bytes(64) + points[power][64 * i + 64:]
            p1 = patched_file(paths[(power, None)], points[power], one, f"zero{i}_{c_env}")
            try:
                with loaded(K, p1, c_env, monkeypatch, c) as ctx:
                    assert zero_points(K, ctx) == 1
                    check(ctx, ref_ctx, one, scalar_sets(npts, c)[0][1], "random")
            finally:
                os.remove(p1)
    finally:
        os.remove(path)


# ------------------------------------------------------------------ slices, a whole proof
@pytest.mark.parametrize("power,c_env,c", [LOADS[0], LOADS[2]], ids=[LOAD_IDS[0], LOAD_IDS[2]])
def test_sliced_tables_sum_to_the_whole(K, files, monkeypatch, power, c_env, c):
    """one SRS slice per rank (load_ptau(slice=(rank, 2)): the points rank + 2 j, scaled and expanded on
    their own). kgs_msm refuses a slice, so the partials are summed where the product sums them: every
    commitment of a two-rank proof is the all-gathered sum of the ranks' MSMs over their slices, and
    the proof equals the one of a context that holds the whole table."""
    paths, _ = files
    nbits = power - 1
    if c_env is None:
        monkeypatch.delenv("KGS_MSM_C", raising=False)
    else:
        monkeypatch.setenv("KGS_MSM_C", str(c_env))
    Fs, Ts, sF, sT = common.make_inputs(4100 + power, nbits, 2, True)
    want = single(K, paths[(power, c_env)], K.GRANDSUM, nbits, Fs, Ts, sF, sT)
    g = K.Group.local(2)
    ctxs = [K.Context(0) for _ in range(2)]
    try:
        for r, ctx in enumerate(ctxs):
            ctx.load_ptau(paths[(power, c_env)], nbits, slice=(r, 2))
            assert ctx.srs_info()[2] == c and ctx.srs_slice_info()[:2] == (r, 2)
        got, err = run_group(K, g, 2, paths[(power, c_env)], K.GRANDSUM, nbits, Fs, Ts, sF, sT, ctxs=ctxs)
    finally:
        for ctx in ctxs:
            ctx.close()
        g.close()
    assert not any(err), err
    assert got[0] == want and got[1] == want


def test_smallest_golden_proof(K):
    """the smallest committed grand-sum fixture through the prover: commitments and evaluations equal"""
    case = min((x for x in GOLD["cases"] if x["kind"] == "grandsum"), key=lambda x: (x["nbits"], x["npols"]))
    Fs, Ts, sF, sT = common.make_inputs(case["seed"], case["nbits"], case["npols"], case["selected"])
    assert common.inputs_digest(Fs, Ts, sF, sT) == case["inputs_sha256"]
    eF = [K.Evaluations(x) for x in Fs]
    eT = [K.Evaluations(x) for x in Ts]
    proof = K.grandsum_prover(common.oracle_ptau(11), eF if case["npols"] > 1 else eF[0],
                              eT if case["npols"] > 1 else eT[0],
                              K.Evaluations(sF) if sF else None, K.Evaluations(sT) if sT else None)
    got = {sec: {k: v.hex() for k, v in proof[sec].items()} for sec in ("commitments", "evaluations")}
    assert got == case["proof"]
