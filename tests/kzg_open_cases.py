"""Shared references of test_kzg_open_refs.py (CPU) and test_gpu_kzg_open.py (GPU): the opening proofs of a
polynomial p = sum_i c_i X^i at every point w^i of the domain of n = 2^nbits points (kgs_kzg_open_all), in
the exponent, three ways. Over an SRS s_m = tau^m G with a known tau every proof is pi_i = q_i(tau) G with
q_i = (p(X) - p(w^i)) / (X - w^i), so an expected point is one oracle scalar multiplication
(g1_ntt_cases.point, cached).

  closed form    q_i(tau) = (p(tau) - p(w^i)) / (tau - w^i), for tau outside the domain
  quotient form  q_z(tau) = sum_k tau^k sum_{j > k} c_j z^(j - k - 1): the synthetic division, which divides
                 by nothing and so holds for tau inside the domain (and tau = 0) too
  Toeplitz form  the steps the library runs (Feist-Khovratovich): h_k = sum_{j >= k + 1} c_j s_{j - 1 - k} by one
                 cyclic convolution of size 2n, then pi = the forward transform of size n of (h_0 .. h_{n-2}, 0)
"""
import random

import common
import degenerate_cases as D
import g1_ntt_cases as N
from oracle import bn254 as bn

R = N.R


def poly_eval(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % R
    return acc


def quotient_coeffs(c, z):
    """the coefficients of (p(X) - p(z)) / (X - z): q_k = sum_{j > k} c_j z^(j - k - 1), k < len(c) - 1"""
    q, acc = [0] * max(len(c) - 1, 0), 0
    for k in range(len(c) - 2, -1, -1):
        acc = (acc * z + c[k + 1]) % R
        q[k] = acc
    return q


def quotient_form(c, z, tau):
    return poly_eval(quotient_coeffs(c, z), tau)


def closed_form(c, nbits, tau=None):
    """q_i(tau), i < 2^nbits, for tau outside the domain: one Fr transform for the p(w^i) and one batched
    inversion, so 2^14 points cost no more than a few Horner passes"""
    tau = common.tau() if tau is None else tau
    den = [(tau - w) % R for w in N.omegas(nbits)]
    assert all(den), "tau lies in the domain: use quotient_scalars"
    pt = poly_eval(c, tau)
    return [(pt - y) * d % R for y, d in zip(evals(c, nbits), N.batch_inv(den))]


def quotient_scalars(c, nbits, tau):
    return [quotient_form(c, w, tau) for w in N.omegas(nbits)]


def toeplitz_steps(c, nbits, tau=None):
    """the library's route on integers in the exponent; returns (h, pi)"""
    tau = common.tau() if tau is None else tau
    n = 1 << nbits
    assert len(c) <= n
    s = N.tau_powers(max(n - 1, 1), tau)
    x = [s[n - 2 - j] if j <= n - 2 else 0 for j in range(2 * n)]              # 1
    xh = N.transform_scalars(x)                                                # 2
    ch = N.transform_scalars(list(c) + [0] * (2 * n - len(c)))                 # 3
    uh = [a * b % R for a, b in zip(ch, xh)]                                   # 4 (the 1 / 2n is in step 5 here)
    u = N.transform_scalars(uh, inverse=True)                                  # 5
    h = [u[n - 1 + k] for k in range(n - 1)]
    return h, N.transform_scalars(h + [0])


def open_all_scalars(c, nbits, tau=None):
    tau = common.tau() if tau is None else tau
    in_domain = pow(tau, 1 << nbits, R) == 1
    return quotient_scalars(c, nbits, tau) if in_domain else closed_form(c, nbits, tau)


def expected_proofs(c, nbits, tau=None):
    return N.points(open_all_scalars(c, nbits, tau))


def evals(c, nbits):
    """p(w^i), i < 2^nbits"""
    return N.transform_scalars(list(c) + [0] * ((1 << nbits) - len(c)))


def mont(vals):
    return common.mont_bytes([v % R for v in vals])


def from_mont(b):
    rinv = pow(1 << 256, R - 2, R)
    return [int.from_bytes(b[i:i + 32], "little") * rinv % R for i in range(0, len(b), 32)]


def commitment(c, tau=None):
    tau = common.tau() if tau is None else tau
    return N.point(poly_eval(c, tau))


def tau_g2(tau=None):
    tau = common.tau() if tau is None else tau
    return bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, tau))


# ------------------------------------------------------------------ kgs_g1_mul_each
# edge scalars of the signed-digit recoding: 0, 1, 2, around r, the top bits, alternating bits (the densest
# NAF), and 3 * 2^252 < r whose NAF 2^254 - 2^252 carries out of bit 253
EDGE_SCALARS = [0, 1, 2, R - 1, R, R + 1, 1 << 253, (1 << 254) - 1, (1 << 256) - 1, ((1 << 254) - 1) // 3,
                3 << 252]
assert (3 << 252) < R


def mul_each_case(n, seed):
    """(multipliers k_i of the points k_i G, scalars s_i): tau^i G with identities at the first, a middle
    and the last index (n > 3); the edge scalars laid over random ones, some of them above r"""
    k = N.tau_powers(n)
    for i in {0, n // 2, n - 1} if n > 3 else ():
        k[i] = 0
    s = D.random_scalars(n, seed)
    rnd = random.Random(seed)
    big = [v + R * rnd.randrange(5) for v in s]
    s = [b if b < 1 << 256 else v for b, v in zip(big, s)]
    for j, e in enumerate(EDGE_SCALARS):
        s[(1 + 7 * j) % n] = e  # n = 1: the last one stays
    return k, s


def mul_each_expected(k, s):
    return N.points([a * b % R for a, b in zip(k, s)])
