"""GPU MSM, prover and ptau writer on degenerate SRS files: points that coincide, cancel or are the
zero point (tests/degenerate_cases.py), byte for byte against the closed form (sum s_i k_i) G.

On an SRS of distinct points tau^i G with random scalars the bucket accumulation never adds two equal
points, two opposite points or a zero point from the table, so the rare paths of g1_acc29::add_aff and
g1_acc29::add (csrc/field29.hpp, behind PP.maybe_zero8()) never run. Here the SRS is the test's own,
so every family below forces one of them whatever order the sort leaves inside a bucket.

Every case runs at the file's natural window (c = 9 at power 12) and at the headline window
(KGS_MSM_C=17), on a two-lane context (k_accumulate<2>, k_rowcol's block tree) and on a one-lane
context (k_accumulate<3>, k_rowcol16's shuffle tree). tests/test_degenerate_oracle.py pins the closed
form against the Python and the C MSM on the same files.
"""
import contextlib
import os
import threading

import pytest

import common
import degenerate_cases as D
from oracle import bn254 as bn
from oracle import protocol as P

pytestmark = pytest.mark.gpu
R = bn.R
POWER = 12  # 8191 points; natural window 9
WINDOWS = ["natural", "c17"]


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(params=WINDOWS)
def win(request, monkeypatch):
    """the window of the tables loaded by the test: the file's own, or KGS_MSM_C=17"""
    if request.param == "c17":
        monkeypatch.setenv("KGS_MSM_C", "17")
    else:
        monkeypatch.delenv("KGS_MSM_C", raising=False)
    return request.param


@contextlib.contextmanager
def loaded(K, name, win, nctx=1):
    """`nctx` contexts with the pattern's SRS resident (a file of the test's own) -> (contexts, c)"""
    ctxs = []
    with D.ptau_file(name, POWER, "_" + win) as path:
        try:
            for _ in range(nctx):
                ctx = K.Context(0)
                ctxs.append(ctx)
                ctx.load_ptau(path, POWER)
            c = ctxs[0].srs_info()[2]
            assert c == (17 if win == "c17" else 9)
            yield ctxs, c
        finally:
            for ctx in ctxs:
                ctx.close()


def check(ctx, name, v, what):
    """ctx.msm == closed form, on a two-lane and on a one-lane context"""
    want = D.expected(name, v)
    mb = common.mont_bytes(v)
    for lanes in (2, 1):
        ctx.set_msm_lanes(lanes)
        assert ctx.msm(mb) == want, (what, len(v), lanes)
    ctx.set_msm_lanes(2)


def test_equal_points_in_a_run(K, win):
    """add_aff's doubling branch. N equal scalars d < 2^(c-1) over `all_G`: bucket d of window 0 holds
    N copies of G and nothing else, so the second add of its first run is G + G in every order (the
    entries are indistinguishable). Scalar 2^c - d has digits (-d, +1): bucket d holds N copies of -G,
    the doubling with `negy` set, and bucket 1 N copies of 2^c G from the second window table."""
    with loaded(K, "all_G", win) as ((ctx,), c):
        assert D.D < 1 << (c - 1)
        for n in (2, 3, 4, 5, 64):
            check(ctx, "all_G", D.equal_small(c, n), "equal")
            check(ctx, "all_G", D.equal_small(c, n, True), "equal-neg")


def test_equal_partials_in_the_combine(K, win):
    """add's doubling branch, in k_combine_level and k_combine. 4096 equal scalars d over `all_G`: one
    bucket of 4096 copies of G, cut into segments of L = 4 entries, so each of the 1024 run records is
    4 G and every combine level adds equal accumulators, whichever segments it pairs. L is
    max(4, ceil(N W / resident threads)) with 512 resident threads per CU (msm_run), so L stays 4
    while N W <= 2048 * CUs: asserted for a 64-CU device, a quarter of an MI355X."""
    n = 4096
    with loaded(K, "all_G", win) as ((ctx,), c):
        assert n * D.windows(c) <= 2048 * 64
        check(ctx, "all_G", D.equal_small(c, n), "equal")
        check(ctx, "all_G", D.equal_small(c, n, True), "equal-neg")
        # a run that ends inside a segment: the last record is 3 G, G + G + G
        check(ctx, "all_G", D.equal_small(c, n - 1), "equal")


def test_opposite_points_cancel(K, win):
    """the opposite-point branch (inf = true) of add_aff or add. k scalars d and k scalars 2^c - d over
    `all_G`: bucket d holds k copies of G and k of -G. Its partial sums move by +-G from 0 back to 0,
    so in every order some add meets the exact opposite of the accumulator: inside a run (add_aff) or
    between run records (add; k = 512 spans 256 segments). [d, 2^c - d, d] and its mirror restart the
    accumulator after a cancellation inside one run (the `if (inf)` branch, with and without `negy`)
    when the bucket keeps the input order, and double then subtract otherwise. All-equal scalars over
    `alt` (G, -G, G, ...) with N even cancel in every bucket of every window: the zero point."""
    with loaded(K, "all_G", win) as ((ctx,), c):
        for k in (1, 2, 3, 512):
            check(ctx, "all_G", D.cancel(c, k), "cancel")
            check(ctx, "all_G", D.cancel(c, k)[::-1], "cancel-reversed")
        check(ctx, "all_G", D.cancel_restart(c), "restart")
        check(ctx, "all_G", [(1 << c) - D.D, D.D, (1 << c) - D.D], "restart-neg")
    with loaded(K, "alt", win) as ((ctx,), c):
        s = D.random_scalars(1, 7)[0]
        for n in (2, 64, 4096):
            assert D.expected("alt", [s] * n) == bytes(64)
            check(ctx, "alt", [s] * n, "identity")
            check(ctx, "alt", [D.D] * n, "identity-small")
        check(ctx, "alt", [s] * 4095, "all-but-one-cancel")


def test_one_point_per_bucket(K, win):
    """add's doubling branch at every level of the bucket tail. Scalars 1..N over `all_G` put exactly
    one G into each of the buckets 1..N (N <= 2^(c-1)), so all bucket totals are equal: every add of
    k_rowcol's block tree (two lanes), of k_rowcol16's sequential part and shuffle tree (one lane) and
    of k_bitsum_rc adds two equal sums of the same number of buckets, a doubling, up to the lines that
    hold bucket 0 or lie past N. N = 2^(c-1) fills bucket B, the T_(c-1) term. Past 2^(c-1) the digits
    wrap (2^(c-1) + i has digits (i - 2^(c-1), +1)): opposite points meet in the buckets too."""
    with loaded(K, "all_G", win) as ((ctx,), c):
        sizes = {255, 256, 4096}
        if (1 << (c - 1)) <= 4096:  # c = 9: 256, listed already; 2^16 points at c = 17 need a larger file
            sizes.add(1 << (c - 1))
        for n in sorted(sizes):
            check(ctx, "all_G", D.ramp(n), "ramp")


def test_identity_buckets_through_the_trees(K, win):
    """the trees with `inf` operands everywhere. Scalars i and 2^c - i for every i in 1..m (m = 255 at
    c = 9, 2047 at c = 17) over `all_G`: every bucket 2..m holds G and -G and sums to the zero point in
    either order (the opposite branch of add_aff, or of add across a segment boundary), and bucket 1
    holds G, -G and the m copies of 2^c G of window 1, whose total is the whole result."""
    with loaded(K, "all_G", win) as ((ctx,), c):
        m = 2047 if c == 17 else 255
        check(ctx, "all_G", D.identity_buckets(c, m), "identity-buckets")


@pytest.mark.parametrize("name", ["all_G", "w4"])
def test_digit_edges(K, win, name):
    """the signed-digit recoding at its edges, over coincident points: 2^(c-1) (the one positive digit
    that is bucket B), 2^(c-1) + 1 (the first that wraps), 2^c - 1, 2^c, r - 1, r - 2^(c-1), and the
    maximal top-window digit without and with a carry rippling into it. Together (one bucket run per
    window over equal or opposite points) and each alone."""
    with loaded(K, name, win) as ((ctx,), c):
        edges = D.digit_edges(c)
        assert all(0 < s < R for s in edges)
        check(ctx, name, edges, "edges")
        check(ctx, name, edges * 8, "edges-x8")
        for s in edges:
            check(ctx, name, [s], "edge-alone")
            check(ctx, name, [s] * 5, "edge-x5")


@pytest.mark.parametrize("name", D.PATTERNS)
def test_random_scalars(K, win, name):
    """random scalars over every pattern: four or eight distinct points, so every bucket run of more
    than a few entries meets equal and opposite points; `zero_tail` and `mixed` add the table's
    affine-infinity entries (add_aff's early return; k_tab_dbl and k_batch_affine with ZZ = 0 when the
    window tables are built)."""
    with loaded(K, name, win) as ((ctx,), c):
        for n in (1, 2, 777, 4096):
            check(ctx, name, D.random_scalars(n, 5000 + n), "random")
        if name in ("zero_tail", "mixed"):
            # nothing but zero points selected: the zero point
            v = [0 if k else s for k, s in zip(D.multipliers(name, 777), D.random_scalars(777, 1))]
            assert D.expected(name, v) == bytes(64)
            check(ctx, name, v, "only-zero-points")


@pytest.mark.parametrize("name", ["all_G", "alt"])
def test_sharded_msm(K, win, name):
    """equal, opposite and zero rank partials in the host combine (combine_partials). Two ranks, each
    over its half of the points: N equal scalars d give both ranks the same bit sums T_k (the host
    add's doubling); d on one half and 2^c - d on the other give opposite T_k for the bits of d (its
    opposite-point branch); over `alt` each rank's half cancels to the zero point."""
    world = 2
    grp = K.ThreadGroup(world)
    with loaded(K, name, win, nctx=world) as (ctxs, c):
        for r, ctx in enumerate(ctxs):
            ctx.set_shard(r, world, grp.allgather(r))
        vs = [D.equal_small(c, 4096), [D.D] * 2048 + [(1 << c) - D.D] * 2048, D.equal_small(c, 2),
              D.random_scalars(777, 31), D.ramp(256)]
        out, err = [None] * world, [None] * world

        def run(r):
            try:
                out[r] = [ctxs[r].msm(common.mont_bytes(v)) for v in vs]
            except Exception as e:  # pragma: no cover
                err[r] = e
                grp._bar.abort()
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(err), err
        want = [D.expected(name, v) for v in vs]
        for r in range(world):
            assert out[r] == want, r


# ------------------------------------------------------------------ whole proofs, the writer
def _proof_dict(K, kk, npols, sel, coms, evs):
    cn, en = K.proof_names(kk, npols, sel)
    return {"commitments": dict(zip(cn, coms)), "evaluations": dict(zip(en, evs))}


@pytest.mark.parametrize("name", list(D.TAUS))
def test_proofs_on_degenerate_tau(K, name):
    """grand-sum and grand-product proofs (k = 2, selectors) with tau in {1, r-1, a 4th root of unity,
    0}: 2^5 against the Python oracle on the same file, 2^11 against the C restatement; commitments and
    evaluations byte-equal. The selector polynomials' equal coefficients over repeated points put runs
    of one point into one bucket in the prover's own flow; with tau = 0 every commitment is p(0) G."""
    from oracle import cbackend as C
    tau = D.TAUS[name]
    with D.ptau_file(name, POWER, "_proof") as path:
        ctx = K.Context(0)
        try:
            ctx.load_ptau(path, POWER)
            srs = P.SRS(path, tau)
            _, sb = C.load_srs_bytes(path)
            for kind, kk in (("grandsum", K.GRANDSUM), ("grandproduct", K.GRANDPRODUCT)):
                Fs, Ts, sF, sT = common.make_inputs(7000 + kk, 5, 2, True)
                coms, evs = ctx.prove(kk, 5, Fs, Ts, sF, sT, mont_out=False)[:2]
                exp = P.prove(kind, srs, [P.EvalBuffer(x) for x in Fs], [P.EvalBuffer(x) for x in Ts],
                              P.EvalBuffer(sF), P.EvalBuffer(sT))
                assert _proof_dict(K, kk, 2, True, coms, evs) == exp, kind
                Fs, Ts, sF, sT = common.make_inputs(7100 + kk, 11, 2, True)
                got = ctx.prove(kk, 11, Fs, Ts, sF, sT, mont_out=False)[:2]
                assert got == tuple(C.prove_raw(kk, 11, Fs, Ts, sF, sT, sb, 0)), kind
        finally:
            ctx.close()


@pytest.mark.parametrize("name", list(D.TAUS))
def test_writer_on_degenerate_tau(K, name):
    """kgs_ptau_write_synthetic with tau in {1, r-1, a 4th root of unity, 0}, byte-equal to the
    oracle's writer: k_fixed_base with the scalars 0 (no table entry added: the zero point) and 1, and
    k_batch_affine with ZZ = 0 entries inside its batch inversion."""
    from oracle import ptau as opt
    tau = D.TAUS[name]
    ctx = K.Context(0)
    mine = f"/tmp/kgs_test_degen_writer_{name}.{os.getpid()}.ptau"
    theirs = mine + ".oracle"
    try:
        for power in (3, 9):
            ctx.write_synthetic_ptau(mine, power, tau)
            opt.write_synthetic_ptau(theirs, power, tau)
            assert open(mine, "rb").read() == open(theirs, "rb").read(), power
    finally:
        ctx.close()
        for p in (mine, theirs):
            if os.path.exists(p):
                os.remove(p)
