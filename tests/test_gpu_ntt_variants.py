"""Every NTT launch shape of the provers, through kgs_ntt_ex (include/kgs.h), against the references of
tests/ntt_cases.py: Python integers up to 2^12, the C restatement above. Byte equality everywhere.

kgs_ntt (test_gpu_parity.py::test_ntt) runs a full-length DIF without scalings and a DIT from natural
order with 1/m, in the default pass build. The provers also launch: the coset evaluation, a DIF whose first
pass multiplies by g^idx and skips waves that lie past a short input; the quotient's DIT in place from
bit-reversed order, times g^-idx and no 1/m; g^-idx and 1/m together (distributed prover); a short input
without the coset (reference replay); and all of them in the pass build of one-lane contexts
(k_ntt_lds_pass<.., WV = 3, ..>: dynamic LDS, no twiddle prefetch). ntt.hip lds_plan gives the passes:

  logm 11  12  13  14  15  16  17  18  19     20     21     22     23     24
  plan 6+5 6+6 6+7 6+8 6+9 7+9 8+9 9+9 6+6+7  6+6+8  6+6+9  7+6+9  8+6+9  8+7+9

(DIF in this order, DIT reversed; below 2^11 radix-8/4/2 kernels with the same pre / post arguments).

The proof tests reach the coset transforms at 2n (n for an unselected grand product) only: LDS sizes
2^11 .. 2^15, 2^17, 2^20, 2^21, 2^23, 2^25 in the default build and 2^14, 2^15, 2^23, 2^25 in the one-lane
build, always with in_len = m/2 or m. No proof runs them at 2^16, 2^18, 2^19, 2^22 or 2^24, and 2^16,
2^22 (7 stages) and 2^18 (9 stages) are the only sizes whose first DIF pass, the one with the fused
pre-scaling, has 7 or 9 stages.
"""
import json
import os
import subprocess
import sys

import pytest

import common
import ntt_cases as N

pytestmark = pytest.mark.gpu
R = N.R
FWD_COSET = N.COSET | N.BITREV                                  # prover.cpp coset_fwd
INV_COSET = N.INVERSE | N.COSET | N.BITREV | N.NO_SCALE | N.INPLACE  # prover.cpp coset_inv_prescaled
BUILDS = [0, N.INFLIGHT]
BUILD_IDS = ["wv2", "wv3"]


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ctx(K):
    c = K.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. every size, every production variant
_SET = {}


def _variant_set(logm):
    """[(name, input, flags, expected)] of one size, computed once and shared by both builds (the last
    size only: 2^22 elements are 128 MiB a vector). The inverse transforms take forward images as
    their input, as in the prover, so two of them are expected to return the forward input itself."""
    if logm not in _SET:
        _SET.clear()
        m = 1 << logm
        c = N.random_elements(1000 + logm, m)
        half = c[:32 * (m // 2)]
        ev_coset = N.ref(c, logm, N.COSET)  # natural order
        ev_coset_rev = N.ref(c, logm, FWD_COSET)
        ev_plain_rev = N.ref(c, logm, N.BITREV)
        quot = N.ref(ev_coset_rev, logm, INV_COSET)
        # the prescaled inverse of the coset evaluations is m times the polynomial: spot check of the reference
        cv, qv = N.unmont(c[:32 * 3] + c[-32:]), N.unmont(quot[:32 * 3] + quot[-32:])
        assert qv == [x * m % R for x in cv]
        _SET[logm] = [
            ("coset_fwd in_len=m/2", half, FWD_COSET, N.ref(half, logm, FWD_COSET)),
            ("coset_fwd in_len=m", c, FWD_COSET, ev_coset_rev),
            ("coset_inv_prescaled in place", ev_coset_rev, INV_COSET, quot),
            ("inverse coset with 1/m", ev_coset, N.INVERSE | N.COSET, c),
            ("forward bitrev", c, N.BITREV, ev_plain_rev),
            ("inverse from bitrev", ev_plain_rev, N.INVERSE | N.BITREV, c),
        ]
        if logm == 0:
            assert ev_coset == ev_coset_rev == ev_plain_rev == quot == c and half == b""
    return _SET[logm]


def _run_variant_set(ctx, logm, build):
    for name, x, flags, want in _variant_set(logm):
        got = ctx.ntt_ex(x, logm, flags | build)
        assert got == want, name


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("logm", list(range(0, 23)))
def test_production_variants(ctx, logm, build):
    """2^19 .. 2^22 take seconds, not milliseconds like the sizes below them: their time is the C
    reference's four transforms and the 32 B x 2^logm host copies, paid once per size (wv2), not the GPU's."""
    _run_variant_set(ctx, logm, build)


# ------------------------------------------------------------------ 7. opt-in sizes
@pytest.mark.skipif(not os.environ.get("KGS_TEST_NTT_BIG"), reason="opt-in (KGS_TEST_NTT_BIG=1): 2^23 and 2^24, the "
                    "sizes with a 7-stage middle pass; tens of seconds of oracle/c each")
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("logm", [23, 24])
def test_production_variants_big(ctx, logm, build):
    _run_variant_set(ctx, logm, build)
    _SET.clear()


# ------------------------------------------------------------------ 2. input-length edges
def _edge_lengths(m):
    want = [0, 1, 2, 63, 64, 65, m // 2 - 1, m // 2 + 1, m // 2 + 33, m - 1]
    return sorted({x for x in want if 0 <= x <= m})


_EDGE = {}


def _edge_refs(logm):
    if logm not in _EDGE:
        _EDGE.clear()
        x = N.random_elements(2000 + logm, 1 << logm)
        _EDGE[logm] = x, {(L, f): N.ref(x[:32 * L], logm, f) for L in _edge_lengths(1 << logm)
                          for f in (FWD_COSET, N.BITREV)}
    return _EDGE[logm]


# one size per stage count of the first LDS pass (6, 7, 8, 9 stages) and two radix-kernel sizes
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("logm", [3, 10, 11, 16, 17, 18])
def test_input_length_edges(ctx, logm, build):
    """in_len off the powers of two: waves that straddle the end of the input (the wave-uniform skip of
    the pre-scaling branch must not drop a lane that still has input), with the coset scaling and
    without it (the reference replay's launch)."""
    x, refs = _edge_refs(logm)
    assert len(refs) >= 6
    for (L, flags), want in refs.items():
        assert ctx.ntt_ex(x[:32 * L], logm, flags | build) == want, (L, flags)


# ------------------------------------------------------------------ 3. field edges through the fused products
_EXT = {}


def _extreme_refs(logm, kind):
    if (logm, kind) not in _EXT:
        _EXT.clear()
        x = common.ntt_extreme_input(kind, 1 << logm)
        _EXT[logm, kind] = x, N.ref(x, logm, FWD_COSET), N.ref(x, logm, INV_COSET), \
            N.ref(x, logm, N.INVERSE | N.COSET)
    return _EXT[logm, kind]


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("kind", ["all", "raw_r-1", "raw_low_ones", "raw_cycle"])
@pytest.mark.parametrize("logm", [5, 11, 18])
def test_field_edges(ctx, logm, kind, build):
    """The scalings multiply butterfly outputs in [0, 2r) (post, post_s) and inputs at the top of the
    canonical range (pre): a missing reduction after them shows on these vectors."""
    x, fwd, inv, inv_scaled = _extreme_refs(logm, kind)
    assert ctx.ntt_ex(x, logm, FWD_COSET | build) == fwd
    assert ctx.ntt_ex(x, logm, INV_COSET | build) == inv
    assert ctx.ntt_ex(x, logm, N.INVERSE | N.COSET | build) == inv_scaled


# ------------------------------------------------------------------ 4. + 5. fresh processes
_CHILD = """
import hashlib, json, sys
sys.path.insert(0, {tests!r})
import common
import ntt_cases as N
K = common.load_pkg()
c = K.Context(0)
FWD = N.COSET | N.BITREV
INV = N.INVERSE | N.COSET | N.BITREV | N.NO_SCALE | N.INPLACE
out = {{}}
# this process's domain is 2^18 from here on: the smaller transforms below stride its tables
c.ntt_ex(N.random_elements(5, 1 << 18), 18, FWD)
for logm in (11, 14):
    x = N.random_elements(300 + logm, 1 << logm)
    for build in (0, N.INFLIGHT):
        y = c.ntt_ex(c.ntt_ex(x, logm, FWD | build), logm, INV | build)
        out["trip%d/%d" % (logm, build)] = y == common.mont_bytes([(v << logm) % N.R for v in N.unmont(x)])
for logm in (11, 16, 17, 18, 19, 22):
    x = N.random_elements(400 + logm, 1 << logm)
    for build in (0, N.INFLIGHT):
        out["h%d/%d" % (logm, build)] = [hashlib.sha256(c.ntt_ex(x, logm, f | build)).hexdigest() for f in (FWD, INV)]
print(json.dumps(out))
"""
_CHILD_OUT = {}


def _child(t29):
    """one fresh process per KGS_NTT_T29 setting (the knob is read once per process), run once"""
    if t29 not in _CHILD_OUT:
        code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, KGS_NTT_T29=t29)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        _CHILD_OUT[t29] = json.loads(out.stdout.strip().splitlines()[-1])
    return _CHILD_OUT[t29]


@pytest.mark.parametrize("t29", ["1", "0"])
def test_round_trip_on_a_larger_domain(t29):
    """inverse-coset(forward-coset(c)) = m c at 2^11 and 2^14 on a context whose domain is 2^18: the
    twiddle stride of logm < logM together with the coset tables (read at stride 1)."""
    res = _child(t29)
    trips = {k: v for k, v in res.items() if k.startswith("trip")}
    assert len(trips) == 4 and all(trips.values()), trips


def test_8x32_twiddles_identical():
    """The coset transforms with 29-bit twiddle / scaling records (the default) and with 8 x 32-bit
    words (KGS_NTT_T29=0) are the same bytes, per size and build; test_production_variants pins the
    default to the oracle, so this pins the 8 x 32 instantiations too. One size per first-pass stage
    count (11, 16, 17, 18) and two three-pass plans (19, 22)."""
    a, b = _child("1"), _child("0")
    hashes = {k: v for k, v in a.items() if k.startswith("h")}
    assert len(hashes) == 12
    assert a == b
    # and the two pass builds agree with each other
    for logm in (11, 16, 17, 18, 19, 22):
        assert a["h%d/0" % logm] == a["h%d/%d" % (logm, N.INFLIGHT)]


# ------------------------------------------------------------------ 6. argument errors
def test_argument_errors(K, ctx):
    x = N.random_elements(9, 8)
    bad = [(x, 3, N.INVERSE | N.INPLACE),                # would gather from the buffer it writes
           (x, 3, N.INVERSE | N.INPLACE | N.COSET),
           (x, 3, 64), (x, 3, N.COSET | 1 << 20), (x, 3, -1),  # unknown flag bits
           (x, -1, 0), (x, 29, 0), (x, 29, N.INVERSE),   # bad logm
           (x, 2, N.BITREV)]                             # forward input longer than the transform
    for data, logm, flags in bad:
        with pytest.raises(K.KgsError) as e:
            ctx.ntt_ex(data, logm, flags)
        assert e.value.code == -1, (logm, flags)  # KGS_E_ARG
    with pytest.raises(ValueError):
        ctx.ntt_ex(x[:64], 3, N.INVERSE)  # an inverse takes 2^logm elements
    for flags in (FWD_COSET, INV_COSET, N.INVERSE | N.INPLACE | N.BITREV, 0, N.INVERSE):
        assert ctx.ntt_ex(x, 3, flags) == N.ref(x, 3, flags), flags
    assert ctx.ntt_ex(x, 3, 0) == ctx.ntt(x, False) and ctx.ntt_ex(x, 3, N.INVERSE) == ctx.ntt(x, True)
