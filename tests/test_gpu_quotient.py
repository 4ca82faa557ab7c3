"""Round 3's pointwise kernels and the linear combination as primitives: kgs_quotient_ex, kgs_divcheck and
kgs_lincomb (include/kgs.h) run k_quotient<PROD,SEL>, k_quotient_multi, k_divcheck<PROD,SEL>, the
1/(n(x - 1)) table of get_nxm1 and k_lincomb through the host functions the round engine itself calls
(run_quotient, run_divcheck, run_lincomb), against the Python-integer references of quotient_cases.py
(pinned to the protocol by test_quotient_refs.py). Byte equality everywhere.

Whole honest proofs leave most of these kernels' inputs unvisited: challenges are hash outputs (never 0, 1
or r - 1), S is the true running sum (no zero factor, the numerator always divisible), selectors are binary
(sel - sel^2 is identically zero, so its alpha^2 / alpha^3 weights and the lookup's alpha_t = 0 go unseen), and
more than 32 terms or 8 arguments occur in one proof shape each. Here the arrays are arbitrary field
elements, so every term of the formulas carries weight.
"""
import json
import os
import subprocess
import sys

import pytest

import common
import ntt_cases as N
import quotient_cases as Q

pytestmark = pytest.mark.gpu
R = Q.R
E_ARG = -1
M = common.mont_bytes
SHAPES = [(1, 1), (1, 2), (3, 4), (7, 8), (8, 8), (8, 9), (9, 10)]  # 2 points .. four blocks; rot 1 and 2
CROSSED = [(1, 2), (8, 9)]  # every alpha and gamma value meets every build here
ALPHAS = [0, 1, R - 1, None]  # None: random
GAMMAS = [0, R - 1, None]


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ctx(K):
    c = K.Context(0)
    yield c
    c.close()


def _native(a):
    return (a["kind"], M(a["S"]), M(a["F"]), M(a["T"]), M(a["sel_f"]) if a["sel_f"] is not None else None,
            M(a["sel_t"]) if a["sel_t"] is not None else None)


def _quot(ctx, nbits, lcs, native, alpha, gamma, delta=None, flags=0):
    return ctx.quotient_ex(nbits, lcs, native, M([alpha]), M([gamma]), None if delta is None else M([delta]), flags)


# ------------------------------------------------------------------ 1. one argument, every build
def _single_cases(build, nbits, lcs):
    """[(name, argument, alpha, gamma)]"""
    rnd = Q.seeded(1000 * Q.BUILD_NAMES.index(build) + 10 * lcs + nbits)
    cs = 1 << lcs
    sel = Q.BUILDS[build][1]
    out = [("random", Q.quot_arg(rnd, build, cs), rnd.randrange(R), rnd.randrange(R))]
    for const in ("r-1", "0", "1"):
        a = Q.quot_arg(rnd, build, cs, const)
        out.append(("all " + const, a, R - 1, R - 1))
        out.append(("all " + const + ", random challenges", a, rnd.randrange(R), rnd.randrange(R)))
    if sel:
        out.append(("selectors random non-binary", Q.quot_arg(rnd, build, cs, "sel-random"), rnd.randrange(R), rnd.randrange(R)))
        out.append(("selectors all r-1", Q.quot_arg(rnd, build, cs, "sel-r-1"), rnd.randrange(R), rnd.randrange(R)))
    # a zero factor: gamma = -F[p0] and gamma = -T[p0], the last point included
    a = Q.quot_arg(rnd, build, cs, "sel-random" if sel else "random")
    for p0 in sorted({0, cs // 2, cs - 1}):
        out.append(("gamma = -F[%d]" % p0, a, rnd.randrange(R), (R - a["F"][p0]) % R))
        out.append(("gamma = -T[%d]" % p0, a, rnd.randrange(R), (R - a["T"][p0]) % R))
    # the extreme challenges; crossed at the two shapes that need it, one row and one column elsewhere
    if (nbits, lcs) in CROSSED:
        pairs = [(al, ga) for al in ALPHAS for ga in GAMMAS]
    else:
        pairs = [(al, None) for al in ALPHAS[:3]] + [(None, ga) for ga in GAMMAS[:2]]
    for al, ga in pairs:
        out.append(("alpha %s gamma %s" % (al, ga), a, rnd.randrange(R) if al is None else al,
                    rnd.randrange(R) if ga is None else ga))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-cs%d" % s)
@pytest.mark.parametrize("build", Q.BUILD_NAMES)
def test_single_argument(ctx, K, build, shape):
    """k_quotient<PROD,SEL> and, with KGS_QUOT_FUSED, k_quotient_multi on the same argument."""
    nbits, lcs = shape
    assert K.QUOT_FUSED == Q.QUOT_FUSED  # the package's constant is the header's
    native = {}
    for name, a, alpha, gamma in _single_cases(build, nbits, lcs):
        if id(a) not in native:
            native[id(a)] = _native(a)
        want = M(Q.ref_quotient(nbits, lcs, [a], alpha, gamma))
        plain = _quot(ctx, nbits, lcs, [native[id(a)]], alpha, gamma)
        assert plain == want, name
        # delta is ignored for one argument
        fused = _quot(ctx, nbits, lcs, [native[id(a)]], alpha, gamma, delta=R - 2, flags=Q.QUOT_FUSED)
        assert fused == plain, name + " (fused)"


# ------------------------------------------------------------------ 2. the 1/(n(x - 1)) table
def _nxm1_call(ctx, nbits, lcs, seed=77):
    """alpha = 0, a grand-sum, S = 1: q[p] = 1/(cs n (x_i - 1)), whatever F, T and gamma are"""
    rnd = Q.seeded(seed + lcs)
    cs = 1 << lcs
    a = (Q.GRANDSUM, M([1] * cs), M(Q.rand_vec(rnd, cs)), M(Q.rand_vec(rnd, cs)), None, None)
    return _quot(ctx, nbits, lcs, [a], 0, rnd.randrange(R))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-cs%d" % s)
def test_nxm1_table(ctx, shape):
    nbits, lcs = shape
    want = M(Q.ref_nxm1(nbits, lcs))
    assert _nxm1_call(ctx, nbits, lcs) == want
    assert _nxm1_call(ctx, nbits, lcs, seed=78) == want  # from the cache


_CHILD = """
import json, sys
sys.path.insert(0, {tests!r})
import common
import ntt_cases as N
import quotient_cases as Q
import test_gpu_quotient as T
K = common.load_pkg()
out = {{}}
want = {{s: common.mont_bytes(Q.ref_nxm1(*s)) for s in T.SHAPES + [(3, 3)]}}
# a fresh context per shape, nothing else alive in this process: its domain is exactly 2^lcs (stride 1)
for s in T.SHAPES:
    c = K.Context(0)
    out["equal/%d/%d" % s] = T._nxm1_call(c, *s) == want[s]
    c.close()
# a context whose domain is 2^12 before the first table is built: every shape strides the twiddles
c = K.Context(0)
c.ntt_ex(N.random_elements(1, 1 << 12), 12, N.COSET | N.BITREV)
for s in T.SHAPES:
    out["larger/%d/%d" % s] = T._nxm1_call(c, *s) == want[s]
c.close()
# the cache across a growing domain: tables built on a 2^4 domain, the domain grown to 2^9, the same shapes again
c = K.Context(0)
a = [T._nxm1_call(c, 3, 4), T._nxm1_call(c, 3, 3)]
c.ntt_ex(N.random_elements(2, 1 << 9), 9, N.COSET | N.BITREV)
b = [T._nxm1_call(c, 3, 4), T._nxm1_call(c, 3, 3)]
out["grown"] = a == b == [want[3, 4], want[3, 3]]
# and a shape first asked for after the growth
out["grown/new"] = T._nxm1_call(c, 8, 9) == want[8, 9]
c.close()
print(json.dumps(out))
"""
_CHILD_OUT = []


def _child():
    """one fresh process (what a context's domain is depends on every other context alive), run once"""
    if not _CHILD_OUT:
        code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        _CHILD_OUT.append(json.loads(out.stdout.strip().splitlines()[-1]))
    return _CHILD_OUT[0]


def test_nxm1_on_fresh_contexts():
    """the table's twiddle stride: a domain equal to the coset (stride 1) and a larger one"""
    res = _child()
    for kind in ("equal", "larger"):
        got = {k: v for k, v in res.items() if k.startswith(kind + "/")}
        assert len(got) == len(SHAPES) and all(got.values()), got


def test_nxm1_cache_survives_a_growing_domain():
    res = _child()
    assert res["grown"] is True and res["grown/new"] is True


# ------------------------------------------------------------------ 3. several arguments
CYCLE = ["gs", "gp-sel", "lookup", "gs-sel", "gp"]  # both launches of a split see every build
COUNTS = [2, 7, 8, 9, 15, 16]
MULTI_SHAPES = [(2, 3), (8, 9)]
_MULTI = {}


def _multi_args(count, lcs, builds=None, pattern="sel-random"):
    key = (count, lcs, tuple(builds or ()), pattern)
    if key not in _MULTI:
        rnd = Q.seeded(3000 + 100 * count + lcs)
        args = []
        for j in range(count):
            b = (builds or CYCLE)[j % len(builds or CYCLE)]
            pat = pattern if Q.BUILDS[b][1] or pattern not in ("sel-random", "sel-r-1") else "random"
            args.append(Q.quot_arg(rnd, b, 1 << lcs, pat))
        _MULTI[key] = args, [_native(a) for a in args]
    return _MULTI[key]


@pytest.mark.parametrize("shape", MULTI_SHAPES, ids=lambda s: "n%d-cs%d" % s)
@pytest.mark.parametrize("count", COUNTS)
def test_several_arguments(ctx, count, shape):
    """k_quotient_multi: one launch up to 8 arguments, two (the second accumulating) from 9 on."""
    nbits, lcs = shape
    args, native = _multi_args(count, lcs)
    rnd = Q.seeded(3100 + count)
    alpha, gamma = rnd.randrange(R), rnd.randrange(R)
    for delta in (rnd.randrange(R), 0, 1, R - 1):
        want = M(Q.ref_quotient(nbits, lcs, args, alpha, gamma, delta))
        got = _quot(ctx, nbits, lcs, native, alpha, gamma, delta)
        assert got == want, delta
        if delta == 0:  # 0^0 = 1: argument 0 alone
            assert got == _quot(ctx, nbits, lcs, native[:1], alpha, gamma)


@pytest.mark.parametrize("count", [8, 16])
@pytest.mark.parametrize("nbits", [2, 8])
def test_unselected_grand_products_on_the_small_coset(ctx, count, nbits):
    args, native = _multi_args(count, nbits, builds=["gp"], pattern="random")
    rnd = Q.seeded(3200 + count + nbits)
    alpha, gamma, delta = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    assert _quot(ctx, nbits, nbits, native, alpha, gamma, delta) == M(Q.ref_quotient(nbits, nbits, args, alpha, gamma, delta))


@pytest.mark.parametrize("shape", MULTI_SHAPES, ids=lambda s: "n%d-cs%d" % s)
def test_longest_lazy_sums(ctx, shape):
    """16 arguments, every array all r - 1, alpha = gamma = delta = r - 1: every lazy sum of eight terms at
    the top of its range in both launches."""
    nbits, lcs = shape
    args, native = _multi_args(16, lcs, pattern="r-1")
    want = M(Q.ref_quotient(nbits, lcs, args, R - 1, R - 1, R - 1))
    assert _quot(ctx, nbits, lcs, native, R - 1, R - 1, R - 1) == want
    # and with random arrays under the same challenges
    args, native = _multi_args(16, lcs)
    assert _quot(ctx, nbits, lcs, native, R - 1, R - 1, R - 1) == M(Q.ref_quotient(nbits, lcs, args, R - 1, R - 1, R - 1))


@pytest.mark.parametrize("shape", MULTI_SHAPES, ids=lambda s: "n%d-cs%d" % s)
def test_linearity_in_the_arguments(ctx, shape):
    """Independent of the reference: the fused quotient of nine arguments is the field sum of delta^j times
    argument j's own quotient (its L1 term included), from nine single-argument launches."""
    nbits, lcs = shape
    args, native = _multi_args(9, lcs)
    rnd = Q.seeded(3300 + lcs)
    alpha, gamma, delta = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    total = [0] * (1 << lcs)
    for j in range(9):
        single = Q.unmont(_quot(ctx, nbits, lcs, [native[j]], alpha, gamma))
        dj = pow(delta, j, R)
        total = [(x + dj * y) % R for x, y in zip(total, single)]
    assert _quot(ctx, nbits, lcs, native, alpha, gamma, delta) == M(total)


# ------------------------------------------------------------------ 4. between the prover's transforms
FWD_COSET = N.COSET | N.BITREV
INV_COSET = N.INVERSE | N.COSET | N.BITREV | N.NO_SCALE | N.INPLACE


@pytest.mark.parametrize("build", Q.BUILD_NAMES)
def test_composition_with_the_transforms(ctx, build):
    """coset_fwd of the oracle's coefficient vectors, the quotient, coset_inv_prescaled: the oracle's Q. The
    primitive's point order, rotation and 1/cs are the prover's own."""
    case = Q.honest_case(build, 5, 9500 + Q.BUILD_NAMES.index(build))
    nbits, lcs = 5, case["lcs"]
    cos = {k: (ctx.ntt_ex(M(v), lcs, FWD_COSET) if v is not None else None) for k, v in case["coef"].items()}
    q = _quot(ctx, nbits, lcs, [(case["kind"], cos["S"], cos["F"], cos["T"], cos["sel_f"], cos["sel_t"])],
              case["alpha"], case["gamma"])
    cs = 1 << lcs
    assert not any(case["Q_coef"][cs:]) and any(case["Q_coef"])
    assert ctx.ntt_ex(q, lcs, INV_COSET) == M((list(case["Q_coef"]) + [0] * cs)[:cs])


# ------------------------------------------------------------------ 5. divisibility
DIV_N = [1, 2, 255, 256, 257, 1024, 1000]


def _div_data(build, n, seed, s0=None, closing=False, bad_sel=None):
    """Honest by construction: arbitrary f, t and selectors, S by the recurrence, the true continuation.
    closing: t and sel_t are f and sel_f rotated by one, so the run returns to S[0]. bad_sel = (name, i):
    that selector is not binary at i (the run stays honest: only the binary constraint is broken)."""
    kind, sel = Q.BUILDS[build]
    rnd = Q.seeded(seed)
    gamma = rnd.randrange(R)
    f = Q.rand_vec(rnd, n)
    t = [f[i - 1] for i in range(n)] if closing else Q.rand_vec(rnd, n)
    sf = st = None
    if sel:
        sf = [rnd.randrange(2) for _ in range(n)]
        st = [sf[i - 1] for i in range(n)] if closing else [rnd.randrange(4 if kind == Q.LOOKUP else 2) for _ in range(n)]
        for i in () if closing else _change_at(n):  # rows that a test changes are switched on (one switched off is free)
            sf[i] = st[i] = 1
        if bad_sel:
            (sf if bad_sel[0] == "sel_f" else st)[bad_sel[1]] = rnd.randrange(2, R)
    S, s_next = Q.honest_run(kind, n, f, t, sf, st, gamma, s0)
    return {"kind": kind, "S": S, "f": f, "t": t, "sel_f": sf, "sel_t": st, "gamma": gamma, "s_next": s_next}


def _change_at(n):
    return sorted({i for i in (0, n - 1, 255, 256, n // 2) if 0 <= i < n})


def _div(ctx, d, alpha, s_next="true", gbase=0, **changed):
    v = dict(d, **changed)
    nxt = d["s_next"] if s_next == "true" else s_next
    got = ctx.divcheck(v["kind"], M(v["S"]), M(v["f"]), M(v["t"]), M([alpha]), M([v["gamma"]]),
                       M(v["sel_f"]) if v["sel_f"] is not None else None, M(v["sel_t"]) if v["sel_t"] is not None else None,
                       None if nxt is None else M([nxt]), gbase)
    want = Q.ref_divcheck(v["kind"], v["S"], v["f"], v["t"], v["sel_f"], v["sel_t"], alpha, v["gamma"], nxt, gbase)
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("n", DIV_N)
@pytest.mark.parametrize("build", Q.BUILD_NAMES)
def test_divisibility(ctx, build, n):
    """k_divcheck<PROD,SEL> answers "divisible" on honest inputs of any length and notices one changed
    element anywhere, the wrap included. Every answer is also the reference's (_div)."""
    seed = 5000 + 10 * n + Q.BUILD_NAMES.index(build)
    d = _div_data(build, n, seed)
    alpha = Q.seeded(seed).randrange(1, R)
    assert _div(ctx, d, alpha) == 0
    for name in ("S", "f", "t"):
        for i in _change_at(n):
            v = list(d[name])
            v[i] = (v[i] + 1) % R
            assert _div(ctx, d, alpha, **{name: v}) == 1, (name, i)
    # the continuation
    assert _div(ctx, d, alpha, s_next=(d["s_next"] + 1) % R) == 1
    assert _div(ctx, d, alpha, s_next=None) == _div(ctx, d, alpha, s_next=d["S"][0])
    c = _div_data(build, n, seed + 1, closing=True)
    assert c["s_next"] == c["S"][0]
    assert _div(ctx, c, alpha, s_next=None) == 0 and _div(ctx, c, alpha, s_next=c["S"][0]) == 0
    # gbase: the L1 term belongs to natural index 0 only
    off = _div_data(build, n, seed + 2, s0=12345)
    assert _div(ctx, off, alpha, gbase=0) == 1
    assert _div(ctx, off, alpha, gbase=5) == 0
    # alpha = 0: nothing away from index 0 counts, and index 0 is decided by L1 alone
    rnd = Q.seeded(seed + 3)
    junk = dict(d, S=Q.rand_vec(rnd, n), f=Q.rand_vec(rnd, n), t=Q.rand_vec(rnd, n))
    assert _div(ctx, junk, 0, gbase=5) == 0
    assert _div(ctx, junk, 0, gbase=0) == 1
    start = 1 if d["kind"] == Q.GRANDPRODUCT else 0
    assert _div(ctx, dict(junk, S=[start] + junk["S"][1:]), 0, gbase=0) == 0
    assert _div(ctx, junk, alpha, gbase=5) == 1


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("build", ["gs-sel", "gp-sel", "lookup"])
def test_divisibility_sees_non_binary_selectors(ctx, build, n):
    """The alpha^2 (selF - selF^2) and alpha^3 (selT - selT^2) terms on an otherwise honest run; a lookup's
    selT holds multiplicities and is free."""
    seed = 6000 + 10 * n + Q.BUILD_NAMES.index(build)
    alpha = Q.seeded(seed).randrange(1, R)
    for name in ("sel_f", "sel_t"):
        for i in sorted({0, n // 2, n - 1}):
            d = _div_data(build, n, seed, bad_sel=(name, i))
            want = 0 if (build == "lookup" and name == "sel_t") else 1
            assert _div(ctx, d, alpha) == want, (name, i)


# ------------------------------------------------------------------ 6. linear combination
LC_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 256]
LC_OUT = [1, 255, 256, 257, 1000]
_POOL = []


def _pool():
    """eight source vectors of 1007 elements (Montgomery bytes, values): seven random, one all r - 1"""
    if not _POOL:
        for j in range(7):
            b = N.random_elements(7000 + j, 1007)
            _POOL.append((b, Q.unmont(b)))
        _POOL.append((M([R - 1]) * 1007, [R - 1] * 1007))
    return _POOL


def _lc_case(count, out_len, shift, c0):
    rnd = Q.seeded(7100 + count)
    choices = [0, 1, out_len - 1, out_len, out_len + 7]
    lens = [choices[(k + shift) % 5] for k in range(count)]
    special = [0, 1, R - 1]
    coefs = [special[k % 4] if k % 4 < 3 else rnd.randrange(R) for k in range(count)]
    pool = _pool()
    which = [(7 * k + 3) % 8 for k in range(count)]
    srcs = [pool[w][0][:32 * ln] for w, ln in zip(which, lens)]
    want = Q.ref_lincomb([pool[w][1] for w in which], lens, coefs, c0, out_len)
    return srcs, lens, coefs, want


@pytest.mark.parametrize("count", LC_COUNTS)
def test_lincomb(ctx, count):
    """run_lincomb: 32 terms to a launch, the later launches re-reading out; a term's own length in every
    launch. With lens[k] cycling through {0, 1, out_len - 1, out_len, out_len + 7} from every starting point,
    each length occurs in the first launch and (from 33 terms on) in a later one."""
    for out_len in LC_OUT:
        for shift in range(5 if count < 100 else 2):
            c0 = (0, R - 1)[shift % 2]
            srcs, lens, coefs, want = _lc_case(count, out_len, shift, c0)
            if count >= 37:
                assert set(lens[:32]) == set(lens[32:]) == {0, 1, out_len - 1, out_len, out_len + 7}
            got = ctx.lincomb(srcs, M(coefs), M([c0]), out_len, lens)
            assert got == M(want), (out_len, shift)


def test_lincomb_one_buffer_many_times(ctx):
    """every term reads the same device buffer (as S does in round 5), 65 terms over three launches"""
    rnd = Q.seeded(7200)
    buf, vals = _pool()[0]
    for out_len in (257, 1000):
        lens = [(out_len + 7, out_len, 1, out_len - 1)[k % 4] for k in range(65)]
        coefs = [R - 1 if k % 3 == 0 else rnd.randrange(R) for k in range(65)]
        got = ctx.lincomb([buf] * 65, M(coefs), M([R - 1]), out_len, lens)
        assert got == M(Q.ref_lincomb([vals] * 65, lens, coefs, R - 1, out_len))


def test_lincomb_all_r_minus_1(ctx):
    """32 and 64 terms of r - 1 times r - 1: the longest lazy sums, with c0 = r - 1 on top"""
    buf, vals = _pool()[7]
    for count in (32, 64):
        got = ctx.lincomb([buf] * count, M([R - 1] * count), M([R - 1]), 300, [300] * count)
        assert got == M(Q.ref_lincomb([vals] * count, [300] * count, [R - 1] * count, R - 1, 300))


# ------------------------------------------------------------------ 7. argument errors
def _arg_error(K, fn, *a, **kw):
    with pytest.raises(K.KgsError) as e:
        fn(*a, **kw)
    assert e.value.code == E_ARG and str(e.value), (a, kw)


def test_argument_errors(K, ctx):
    rnd = Q.seeded(8000)
    x = M(Q.rand_vec(rnd, 16))
    one, sc = M([1] * 16), M([5])
    gs = (Q.GRANDSUM, x, x, x, None, None)
    # kgs_quotient_ex
    for nbits, lcs in ((0, 0), (0, 1), (28, 28), (28, 29), (3, 5), (4, 3), (3, 2), (-1, 0)):
        _arg_error(K, ctx.quotient_ex, nbits, lcs, [gs], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs] * 17, sc, sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs, gs], sc, sc, None)              # several arguments need delta
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs], sc, sc, flags=2)
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs], sc, sc, flags=Q.QUOT_FUSED | 4)
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs], None, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs], sc, None)
    _arg_error(K, ctx.quotient_ex, 3, 4, [(3, x, x, x, None, None)], sc, sc)   # unknown kind
    _arg_error(K, ctx.quotient_ex, 3, 4, [(Q.GRANDSUM, None, x, x, None, None)], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [(Q.GRANDSUM, x, x, None, None, None)], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [(Q.GRANDSUM, x, x, x, one, None)], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [(Q.GRANDPRODUCT, x, x, x, None, one)], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [(Q.LOOKUP, x, x, x, None, None)], sc, sc)
    _arg_error(K, ctx.quotient_ex, 3, 4, [gs, (Q.LOOKUP, x, x, x, None, None)], sc, sc, sc)
    with pytest.raises(ValueError):
        ctx.quotient_ex(3, 4, [(Q.GRANDSUM, x, x[:64], x, None, None)], sc, sc)
    # kgs_divcheck
    _arg_error(K, ctx.divcheck, Q.GRANDSUM, b"", b"", b"", sc, sc)             # n = 0
    _arg_error(K, ctx.divcheck, 7, x, x, x, sc, sc)
    _arg_error(K, ctx.divcheck, Q.GRANDSUM, x, None, x, sc, sc)
    _arg_error(K, ctx.divcheck, Q.GRANDSUM, x, x, x, None, sc)
    _arg_error(K, ctx.divcheck, Q.GRANDSUM, x, x, x, sc, None)
    _arg_error(K, ctx.divcheck, Q.GRANDSUM, x, x, x, sc, sc, sel_f=one)
    _arg_error(K, ctx.divcheck, Q.GRANDPRODUCT, x, x, x, sc, sc, sel_t=one)
    _arg_error(K, ctx.divcheck, Q.LOOKUP, x, x, x, sc, sc)
    with pytest.raises(ValueError):
        ctx.divcheck(Q.GRANDSUM, x, x[:32], x, sc, sc)
    # kgs_lincomb
    _arg_error(K, ctx.lincomb, [x] * 257, M([1] * 257), sc, 4)
    _arg_error(K, ctx.lincomb, [x], sc, sc, 0)
    _arg_error(K, ctx.lincomb, [x], sc, sc, (1 << 28) + 1)
    _arg_error(K, ctx.lincomb, [x], sc, None, 4)
    with pytest.raises(ValueError):
        ctx.lincomb([x], sc, sc, 4, lens=[17])
    with pytest.raises(ValueError):
        ctx.lincomb([x, x], sc, sc, 4)
    # the context works afterwards
    a = Q.quot_arg(rnd, "gs-sel", 16, "sel-random")
    assert _quot(ctx, 3, 4, [_native(a)], 11, 12) == M(Q.ref_quotient(3, 4, [a], 11, 12))
    d = _div_data("gp-sel", 16, 8001)
    assert _div(ctx, d, 9) == 0
    v = Q.unmont(x)
    assert ctx.lincomb([x, x], M([2, 3]), M([4]), 16) == M(Q.ref_lincomb([v, v], [16, 16], [2, 3], 4, 16))
