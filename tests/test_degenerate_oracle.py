"""The references of test_gpu_degenerate_srs.py agree with one another on degenerate SRS files
(points that coincide, cancel or are the zero point; tests/degenerate_cases.py), at N <= 64: the
closed form (sum s_i k_i) G equals the Python oracle's Pippenger MSM over the file's points and the C
restatement's MSM, for every pattern and every scalar family, at both windows the GPU test runs."""
import os

import pytest

import common
import degenerate_cases as D
from oracle import bn254 as bn
from oracle import cbackend as C
from oracle import protocol as P
from oracle import ptau as opt
from oracle.ptau import PTau

POWER = 6  # 127 points


@pytest.fixture(scope="module", params=D.PATTERNS)
def srs(request):
    with D.ptau_file(request.param, POWER, "_cpu") as path:
        yield request.param, PTau(path), C.load_srs_bytes(path)[1]


def test_pattern_files(srs):
    """the file holds the pattern: on-curve points (or the zero point) equal to k_i G"""
    name, ptau, raw = srs
    ks = D.multipliers(name, 127)
    assert ptau.power == POWER and len(raw) == 64 * 127
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 126):
        p = ptau.g1_point(i)
        assert bn.g1_is_on_curve(p) and p == bn.g1_mul(bn.G1_GEN, ks[i]), i
    assert D.points(name, 9) == [ptau.g1_point(i) for i in range(9)]
    if name in D.TAUS:  # the oracle's own writer produces the same file from the trapdoor
        with D.ptau_file(name, 3, "_cpu3") as mine:
            theirs = mine + ".oracle"
            try:
                opt.write_synthetic_ptau(theirs, 3, D.TAUS[name])
                assert open(mine, "rb").read() == open(theirs, "rb").read()
            finally:
                if os.path.exists(theirs):
                    os.remove(theirs)


@pytest.mark.parametrize("c", [9, 17])
def test_closed_form_matches_both_msms(srs, c):
    name, ptau, raw = srs
    for fid, v in D.small_families(c):
        assert len(v) <= 64
        want = D.expected(name, v)
        bases = [ptau.g1_point(i) for i in range(len(v))]
        assert bn.g1_to_lem(bn.g1_msm_pippenger(bases, v)) == want, fid
        assert C.msm(raw, common.mont_bytes(v), 2) == want, fid
        if name in D.TAUS:  # and the oracle's trapdoor closed form, which the proofs' reference uses
            assert bn.g1_to_lem(P.SRS(ptau, D.TAUS[name]).msm(v)) == want, fid


def test_identity_results():
    """the cases whose whole result is the zero point expect 64 zero bytes"""
    assert D.expected("alt", [12345] * 64) == bytes(64)
    assert D.expected("all_G", D.cancel(9, 3)) == bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, 3 << 9))
    assert D.expected("zero_tail", [0] + [7] * 63) == bytes(64)
