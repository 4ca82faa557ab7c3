"""The batched block transforms (ntt.hip ntt_dif_blocks / ntt_dit_blocks) through kgs_ntt_blocks (include/kgs.h),
against ntt_cases.ref_blocks: Python integers for blocks up to 2^12, oracle/c above. Byte equality everywhere.

The coset openings and the recovery reach these transforms only inside compound calls, at the shapes their tests
happen to use. The dispatch has four routes by (logtotal, s), s the log of the block size, at a tile of 2^11:

  R1  logtotal < 11 or s <= 3    the radix-8/4/2 kernels alone, on arrays of any size
  R2  logtotal >= 11, 4 <= s <= 9   one LDS pass of K = s contiguous stages; K = 4 is k_ntt_lds_pass<2, 2, 0, 0, ..>,
                                    which no whole transform launches (lds_plan gives no pass below 5 stages)
  R3  logtotal >= 11, s == 10    a 9-stage LDS pass and a radix-2 pass beside it (first in DIF; last in DIT, where it
                                 carries the 1/2^s)
  R4  logtotal >= 11, s >= 11    the passes of lds_plan(s) started at stage logtotal - s: 11 = 6+5, 12 = 6+6, 13 = 6+7,
                                 14 = 6+8, 15 = 6+9, 16 = 7+9, 17 = 8+9, 18 = 9+9, 19 = 6+6+7

Every route runs forward, inverse with 1/2^s and inverse without it, in both pass builds (2 and 3 waves per SIMD) and,
in fresh processes, with both twiddle formats; the domain tables of the context hold 2^s entries, not 2^logtotal.
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

import common
import ntt_cases as N

_NTT_HIP = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "csrc", "ntt.hip")
TILE_LOG = int(re.search(r"#define KGS_NTT_ELOG (\d+)", open(_NTT_HIP).read()).group(1))

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(TILE_LOG != 11, reason="the grid of (logtotal, s) below is written for the routes of a "
                                 "2^11-element tile; KGS_NTT_ELOG is %d" % TILE_LOG)]
KGS_E_ARG = -1
BUILDS = [0, N.INFLIGHT]
BUILD_IDS = ["wv2", "wv3"]
VARIANTS = [0, N.INVERSE, N.INVERSE | N.NO_SCALE]
VARIANT_IDS = ["fwd", "inv", "inv_noscale"]
KEEP_LOG = 16  # reference sets up to 2^KEEP_LOG elements stay cached; of the larger ones only the last


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ctx(K):
    c = K.Context(0)
    yield c
    c.close()


def seed_of(logtotal, s):
    return 7000 + 100 * logtotal + s


_REF = {}


class _Refs(dict):
    """{flags: expected} of one input, each direction computed when first asked for"""

    def __init__(self, x, logtotal, s):
        super().__init__()
        self.shape = x, logtotal, s

    def __missing__(self, flags):
        self[flags] = N.ref_blocks(*self.shape, flags)
        return self[flags]


def _cached(key, logtotal, s, make_input):
    """(input, {flags: expected}) of one shape, computed once and shared by both pass builds"""
    if key not in _REF:
        if logtotal > KEEP_LOG:
            for k in [k for k in _REF if k[0] > KEEP_LOG]:
                del _REF[k]
        x = make_input()
        _REF[key] = x, _Refs(x, logtotal, s)
    return _REF[key]


def refs(logtotal, s):
    return _cached((logtotal, s), logtotal, s, lambda: N.random_elements(seed_of(logtotal, s), 1 << logtotal))


def run(ctx, logtotal, s, build, x, want):
    for flags in VARIANTS:
        assert ctx.ntt_blocks(x, logtotal, s, flags | build) == want[flags], (logtotal, s, flags)


# ------------------------------------------------------------------ every route
def _grid():
    cells = [(0, 0), (11, 0)]
    for s in range(1, 11):  # R1 below a tile, at a tile and far above; R2 at every K; R3 at 2, 4 and 32 blocks
        cells += [(lt, s) for lt in sorted({s, s + 1, 10, 11, 12, 15}) if lt >= s]
    for s in (11, 12, 13):  # R4 with 1, 2 and 8 blocks
        cells += [(lt, s) for lt in (s, s + 1, s + 3)]
    for s in range(14, 19):
        cells += [(s, s), (s + 1, s)]
    return cells


GRID = _grid()


def test_the_grid_reaches_every_route():
    r1 = [c for c in GRID if c[0] < 11 or c[1] <= 3]
    r2 = [c for c in GRID if c[0] >= 11 and 4 <= c[1] <= 9]
    r3 = [c for c in GRID if c[0] >= 11 and c[1] == 10]
    r4 = [c for c in GRID if c[0] >= 11 and c[1] >= 11]
    assert len(r1) + len(r2) + len(r3) + len(r4) == len(GRID) == len(set(GRID)) == 78
    assert {(15, 1), (15, 2), (15, 3), (12, 3), (11, 1), (10, 10), (10, 4)} <= set(r1)
    assert {s for _, s in r2} == set(range(4, 10)) and all((lt, s) in r2 for s in range(4, 10) for lt in (11, 12, 15))
    assert sorted(lt - s for lt, s in r3) == [1, 2, 5]
    assert {s for _, s in r4} == set(range(11, 19)) and {lt - s for lt, s in r4} == {0, 1, 3}


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("flags", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("logtotal,s", GRID)
def test_every_route(ctx, logtotal, s, flags, build):
    """the time of a case is its reference's, paid once per shape and direction (wv2): one to two seconds at 2^15
    elements through the integer reference, milliseconds below 2^12"""
    x, want = refs(logtotal, s)
    if s == 0:
        assert want[flags] == x
    assert ctx.ntt_blocks(x, logtotal, s, flags | build) == want[flags]


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_the_three_pass_block_plan(ctx, build):
    """s = 19 (6+6+7) at two blocks: 2^20 elements, the largest case"""
    x, want = refs(20, 19)
    run(ctx, 20, 19, build, x, want)


# ------------------------------------------------------------------ field edges, one shape per route
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("kind", ["all", "raw_r-1", "raw_low_ones", "raw_cycle"])
@pytest.mark.parametrize("logtotal,s", [(12, 3), (12, 4), (13, 10), (13, 12)])
def test_field_edges(ctx, logtotal, s, kind, build):
    """inputs at the top of the canonical range; the 1/2^s of the inverse multiplies butterfly outputs in [0, 2r): a
    missing reduction shows on these vectors"""
    x, want = _cached((logtotal, s, kind), logtotal, s, lambda: common.ntt_extreme_input(kind, 1 << logtotal))
    run(ctx, logtotal, s, build, x, want)


# ------------------------------------------------------------------ fresh processes: the domain, the twiddle formats
# one (logtotal, s) per route and per K of the one-pass route, all of them cells of the grid above
HASHED = [(12, 3)] + [(12, k) for k in range(4, 10)] + [(12, 10), (12, 11), (15, 14)]
DOMAIN = (15, 4)
_CHILD = """
import hashlib, json, sys
sys.path.insert(0, {tests!r})
import common
import ntt_cases as N
K = common.load_pkg()
VARIANTS = [0, N.INVERSE, N.INVERSE | N.NO_SCALE]
def hashes(c, x, logtotal, s):
    return [hashlib.sha256(c.ntt_blocks(x, logtotal, s, f | b)).hexdigest() for b in (0, N.INFLIGHT) for f in VARIANTS]
out = {{}}
# the first call of this process: the tables of this context hold 2^s entries for an array of 2^logtotal
logtotal, s = {domain!r}
x = N.random_elements({domain_seed}, 1 << logtotal)
small = K.Context(0)
out["small"] = hashes(small, x, logtotal, s)
grown = K.Context(0)
grown.ntt_ex(N.random_elements(1, 1 << 16), 16, N.BITREV)  # tables of 2^16 entries
out["grown"] = hashes(grown, x, logtotal, s)
out["small again"] = hashes(small, x, logtotal, s)
for (logtotal, s), seed in {hashed!r}:
    out["%d/%d" % (logtotal, s)] = hashes(small, N.random_elements(seed, 1 << logtotal), logtotal, s)
print(json.dumps(out))
"""
_CHILD_OUT = {}


def _child(t29):
    """one fresh process per KGS_NTT_T29 setting (the knob is read once per process), run once"""
    if t29 not in _CHILD_OUT:
        code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)), domain=DOMAIN, domain_seed=seed_of(*DOMAIN),
                             hashed=[(c, seed_of(*c)) for c in HASHED])
        env = dict(os.environ, KGS_NTT_T29=t29)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        _CHILD_OUT[t29] = json.loads(out.stdout.strip().splitlines()[-1])
    return _CHILD_OUT[t29]


def _want_hashes(logtotal, s):
    want = refs(logtotal, s)[1]
    return [hashlib.sha256(want[f]).hexdigest() for _ in BUILDS for f in VARIANTS]


@pytest.mark.parametrize("t29", ["1", "0"])
def test_domain_tables_of_one_block(t29):
    """A fresh context in a fresh process, its first call the block transforms of (15, 4): kgs_ntt_blocks grows the
    domain to 2^4, as the compound calls grow theirs to 2^nbits below their arrays of 2^(logP + nbits); the stage
    tables are read by stage. (The context reports no domain size: the bytes are the check.) The same input on a
    context whose tables hold 2^16 entries, and on the first one again, gives the same bytes."""
    res = _child(t29)
    want = _want_hashes(*DOMAIN)
    assert res["small"] == want
    assert res["grown"] == want
    assert res["small again"] == want


def test_8x32_twiddles_identical():
    """29-bit twiddle records (the default) and 8 x 32-bit words (KGS_NTT_T29=0): the same bytes per shape, build and
    direction, and both the reference's"""
    a, b = _child("1"), _child("0")
    assert len(a) == len(HASHED) + 3 and all(len(v) == 6 for v in a.values())
    assert a == b
    for logtotal, s in HASHED:
        assert a["%d/%d" % (logtotal, s)] == _want_hashes(logtotal, s), (logtotal, s)


# ------------------------------------------------------------------ argument errors
def test_argument_errors(K, ctx):
    x = N.random_elements(9, 8)
    bad = [(x, 3, 2, N.COSET), (x, 3, 2, N.BITREV), (x, 3, 2, N.INVERSE | N.INPLACE), (x, 3, 2, 64), (x, 3, 2, 1 << 20),
           (x, 3, 2, -1),                       # flag bits the call does not take
           (x, -1, 0, 0), (x, 29, 3, 0), (x, 29, 29, N.INVERSE),  # logtotal outside 0 .. 28
           (x, 3, -1, 0), (x, 3, 4, 0), (x, 3, 4, N.INVERSE), (x[:32], 0, 1, 0)]  # s outside 0 .. logtotal
    for data, logtotal, s, flags in bad:
        with pytest.raises(K.KgsError) as e:
            ctx.ntt_blocks(data, logtotal, s, flags)
        assert e.value.code == KGS_E_ARG, (logtotal, s, flags)
    for data in (x[:-32], x + x[:32], b""):
        with pytest.raises(ValueError):
            ctx.ntt_blocks(data, 3, 2)
    L = K.lib()
    buf, out = ctypes.create_string_buffer(x, len(x)), ctypes.create_string_buffer(len(x))
    assert L.kgs_ntt_blocks(ctx.handle, None, out, 3, 2, 0) == KGS_E_ARG and "NULL" in L.kgs_last_error().decode()
    assert L.kgs_ntt_blocks(ctx.handle, buf, None, 3, 2, 0) == KGS_E_ARG and "NULL" in L.kgs_last_error().decode()
    assert L.kgs_ntt_blocks(None, buf, out, 3, 2, 0) == KGS_E_ARG
    assert out.raw == bytes(len(x))
    # a good call on the same context, every variant; one block is the whole transform
    for s in (0, 1, 2, 3):
        for flags in VARIANTS:
            assert ctx.ntt_blocks(x, 3, s, flags) == N.ref_blocks(x, 3, s, flags), (s, flags)
    assert ctx.ntt_blocks(x, 3, 3, 0) == ctx.ntt_ex(x, 3, N.BITREV)
    assert ctx.ntt_blocks(x, 3, 3, N.INVERSE) == ctx.ntt_ex(x, 3, N.INVERSE | N.BITREV)
