"""The identity behind the fixed-base MSM's scaled table (csrc/msm.hip msm_build_table, scalar_digits),
on Python integers over BN254.

The device vectors hold Montgomery words s_i = k_i R mod r (R = 2^256). The window table holds
rho P_i with rho = R^-1 mod r, so the MSM reads its digits off the s_i as they are:
sum_i s_i (rho P_i) = sum_i k_i P_i, for any representative of s_i mod r, because every G1 point has
order r.
"""
import random

from oracle import bn254 as bn

R = bn.R
MONT = 1 << 256
RHO = pow(MONT, -1, R)
N = 6


def _points_and_scalars(seed):
    rnd = random.Random(seed)
    pts = [bn.g1_mul(bn.G1_GEN, rnd.randrange(1, R)) for _ in range(N)]
    ks = [rnd.randrange(R) for _ in range(N - 3)] + [0, 1, R - 1]
    return pts, ks


def _mul(p, k):
    """k P by double-and-add over the bits of the integer k as it is (bn.g1_mul reduces k mod r first)"""
    acc, base = None, p
    while k:
        if k & 1:
            acc = bn.g1_add(acc, base)
        base = bn.g1_add(base, base)
        k >>= 1
    return acc


def _msm(points, scalars):
    return bn.g1_sum([_mul(p, s) for p, s in zip(points, scalars)])


def test_rho_is_the_inverse_of_the_montgomery_radix():
    assert 0 < RHO < R
    assert RHO * MONT % R == 1
    # the standard form of the Montgomery word 1, which is where the host code takes it from
    assert RHO == bn.fr_from_bytes((1).to_bytes(32, "little"))


def test_scaled_table_with_montgomery_words():
    pts, ks = _points_and_scalars(1)
    want = _msm(pts, ks)
    scaled = [bn.g1_mul(p, RHO) for p in pts]
    words = [k * MONT % R for k in ks]
    assert words == [int.from_bytes(bn.fr_to_bytes(k), "little") for k in ks]
    assert _msm(scaled, words) == want


def test_other_representative_below_2p255():
    pts, ks = _points_and_scalars(2)
    want = _msm(pts, ks)
    scaled = [bn.g1_mul(p, RHO) for p in pts]
    words = [k * MONT % R for k in ks]
    lifted = [s + R if s + R < 1 << 255 else s for s in words]
    assert any(a != b for a, b in zip(words, lifted))
    assert _msm(scaled, lifted) == want
