"""Shared references of test_g1_ntt.py (CPU, host path) and test_gpu_g1_ntt.py (GPU): inputs of the G1
transform (kgs_g1_ntt) whose output is known in the exponent.

Over the bases P_i = tau^i G of a synthetic ptau with common.tau() both transforms have a closed form,
so every expected point is one oracle scalar multiplication:
  forward  out_j = sum_i w^(ij) tau^i G = ((tau^n - 1) / (w^j tau - 1)) G, or n G when w^j tau = 1
  inverse  out_j = L_j(tau) G,  L_j(tau) = w^j (tau^n - 1) / (n (tau - w^j)); tau in the domain: 1 or 0
For general inputs P_i = a_i G the expected scalars are the Fr transform of a on Python integers
(oracle/poly.py). Scalar -> point conversions are cached, so a size is paid for once.
"""
import functools

import common
from oracle import bn254 as bn
from oracle import poly

R = bn.R


def inv(x):
    return pow(x, R - 2, R)


def batch_inv(vals):
    """1 / v for every v (all nonzero), one modular inversion"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % R
    acc = inv(acc)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = acc * pre[i] % R
        acc = acc * vals[i] % R
    return out


@functools.lru_cache(None)
def point(k):
    """k G as 64 B affine LEM (k = 0 mod r: 64 zero bytes)"""
    return bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, k % R))


def points(scalars):
    return b"".join(point(s % R) for s in scalars)


def omegas(logm):
    n, w = 1 << logm, bn.FR_W[logm]
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * w % R
    return out


def tau_powers(n, tau=None):
    tau = common.tau() if tau is None else tau
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * tau % R
    return out


def forward_scalars(logm, tau=None):
    """s_j with out_j = s_j G for the forward transform of tau^i G, i < 2^logm"""
    tau = common.tau() if tau is None else tau
    n = 1 << logm
    num = (pow(tau, n, R) - 1) % R
    den = [(w * tau - 1) % R for w in omegas(logm)]
    di = batch_inv([d if d else 1 for d in den])
    return [num * i % R if d else n % R for d, i in zip(den, di)]


def lagrange_scalars(logm, tau=None):
    """L_j(tau), j < 2^logm: the inverse transform of tau^i G in the exponent"""
    tau = common.tau() if tau is None else tau
    n = 1 << logm
    num = (pow(tau, n, R) - 1) * inv(n) % R
    ws = omegas(logm)
    den = [(tau - w) % R for w in ws]
    di = batch_inv([d if d else 1 for d in den])
    return [w * num % R * i % R if d else 1 for w, d, i in zip(ws, den, di)]


def naive_scalars(a, inverse=False):
    """the O(n^2) sum: out_j = sum_i w^(+-ij) a_i (inverse: / n)"""
    n = len(a)
    logm = n.bit_length() - 1
    w = bn.FR_W[logm]
    if inverse:
        w = inv(w)
    out = [sum(ai * pow(w, i * j, R) for i, ai in enumerate(a)) % R for j in range(n)]
    return [x * inv(n) % R for x in out] if inverse else out


def transform_scalars(a, inverse=False):
    """the Fr transform of a (oracle/poly.py), a tuple or list of integers"""
    return poly.ntt(list(a), inverse=inverse)


@functools.lru_cache(None)
def expected_forward(logm):
    return points(forward_scalars(logm))


@functools.lru_cache(None)
def expected_inverse(logm):
    return points(lagrange_scalars(logm))


def scalar_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)
