"""GPU checks of the CIOS rows that reduce by a multiple of the modulus that is -1 mod 2^32
(field29.hpp fq29::reduce_row_qstar in the MSM's adds, fr29.hpp mul29 in the NTT's twiddle products),
through the package's MSM, NTT and prover entry points, byte for byte against the host oracle.

The arithmetic argument (constants, exact row schedule, interval bounds) is pinned on the CPU by
test_field29_qstar.py and test_fr29_qstar.py; here the compiled kernels run it on operands at the edges
of the scalar field and on SRS tables whose points coincide, cancel or are the zero point
(degenerate_cases.py), so the equal, opposite and infinity branches of the 29-bit adds run as well
as the common path, in the bucket accumulation and in the tail's trees.
"""
import json
import os
import random

import pytest

import common
import degenerate_cases as D
from oracle import bn254 as bn
from oracle import poly as OP

pytestmark = pytest.mark.gpu
R = bn.R
POWER = 12
EXTREMES = [0, 1, R - 1, (1 << 253) - 1, common.LOW_ONES]
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


def unmb(b):
    return [bn.fr_from_bytes(b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]


def _scalars(n, seed):
    """the extreme scalars in runs (equal scalars over a pattern's repeated points: equal and opposite
    adds inside a bucket), interleaved, and random ones for the rest"""
    rnd = random.Random(seed)
    v = [rnd.randrange(R) for _ in range(n)]
    for i, s in enumerate(EXTREMES):
        v[16 * i:16 * i + 16] = [s] * 16
    for i in range(128, min(n, 384)):
        v[i] = EXTREMES[i % len(EXTREMES)]
    return v


@pytest.mark.parametrize("name", ["mixed", "w4"])
def test_fixed_base_msm_extreme_scalars(K, name):
    """fixed-base MSM of 2^10 and 2^12 scalars over a degenerate SRS (`mixed`: 1, 1, 2, 4, 0, -1, -8, 8
    times G in a cycle, with zero points; `w4`: four distinct points), on a two-lane and on a one-lane
    context (k_accumulate<2> and <3>), against the closed form (sum s_i k_i) G"""
    with D.ptau_file(name, POWER, "_qstar") as path:
        ctx = K.Context(0)
        try:
            ctx.load_ptau(path, POWER)
            for n in (1 << 10, 1 << 12):
                v = _scalars(n, 8000 + n)
                want = D.expected(name, v)
                mb = common.mont_bytes(v)
                for lanes in (2, 1):
                    ctx.set_msm_lanes(lanes)
                    assert ctx.msm(mb) == want, (n, lanes)
            for s in EXTREMES:  # every point with the same extreme scalar
                v = [s] * 1024
                ctx.set_msm_lanes(1)
                assert ctx.msm(common.mont_bytes(v)) == D.expected(name, v), hex(s)
        finally:
            ctx.close()


@pytest.fixture(scope="module")
def ctx9(K):
    c = K.Context(0)
    c.load_ptau(common.oracle_ptau(9))
    yield c
    c.close()


@pytest.mark.parametrize("logm", [11, 12])
def test_ntt_round_trip_and_forward(ctx9, logm):
    """LDS passes (all of their twiddle products are mul29): forward transform against the oracle and
    forward + inverse round trip, on constant 0, 1 and r - 1 vectors, a mix of them, and random input"""
    m = 1 << logm
    rnd = random.Random(900 + logm)
    mix = [(0, 1, R - 1, (1 << 253) - 1, common.LOW_ONES)[i % 5] for i in range(m)]
    for v in ([0] * m, [1] * m, [R - 1] * m, mix, [rnd.randrange(R) for _ in range(m)]):
        x = common.mont_bytes(v)
        fwd = ctx9.ntt(x, False)
        assert ctx9.ntt(fwd, True) == x
        assert unmb(fwd) == OP.ntt(v, False)


def test_smallest_golden_proof(K):
    case = min(GOLD["cases"], key=lambda c: c["nbits"])
    Fs, Ts, sF, sT = common.make_inputs(case["seed"], case["nbits"], case["npols"], case["selected"])
    assert common.inputs_digest(Fs, Ts, sF, sT) == case["inputs_sha256"]
    eF = [K.Evaluations(x) for x in Fs]
    eT = [K.Evaluations(x) for x in Ts]
    fn = K.grandsum_prover if case["kind"] == "grandsum" else K.grandproduct_prover
    proof = fn(common.oracle_ptau(11), eF if case["npols"] > 1 else eF[0], eT if case["npols"] > 1 else eT[0],
               K.Evaluations(sF) if sF else None, K.Evaluations(sT) if sT else None)
    got = {sec: {k: v.hex() for k, v in proof[sec].items()} for sec in ("commitments", "evaluations")}
    assert got == case["proof"]
