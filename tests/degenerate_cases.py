"""Shared inputs of test_degenerate_oracle.py (CPU: pins the references) and test_gpu_degenerate_srs.py
(GPU): SRS files whose points coincide, cancel or are the zero point, and scalar vectors that force
the MSM's equal-point, opposite-point and infinity branches whatever order the sort leaves inside a
bucket.

Every point of a pattern is a known multiple k_i of the generator G, so the expected MSM is one scalar
multiplication: sum_i s_i (k_i G) = (sum_i s_i k_i mod r) G, the zero point (64 zero bytes) when the
sum is 0. Each test writes a ptau of its own (pid-suffixed, removed afterwards), so no window table is
shared with another context.
"""
import contextlib
import functools
import os
import random
import struct

from oracle import bn254 as bn
from oracle import ptau as opt

R = bn.R
W4 = bn.FR_W[2]  # a primitive 4th root of unity mod r
assert pow(W4, 2, R) == R - 1

MIXED_CYCLE = (1, 1, 2, 4, 0, -1, -8, 8)
PATTERNS = ("all_G", "alt", "w4", "zero_tail", "mixed")
# the patterns that are an SRS of a trapdoor: tau^i G
TAUS = {"all_G": 1, "alt": R - 1, "w4": W4, "zero_tail": 0}


def multipliers(name, n):
    """k_i (mod r) of the first n points of a pattern"""
    if name == "all_G":
        return [1] * n
    if name == "alt":
        return [1 if i % 2 == 0 else R - 1 for i in range(n)]
    if name == "w4":
        return [pow(W4, i % 4, R) for i in range(n)]
    if name == "zero_tail":
        return [1] + [0] * (n - 1)
    if name == "mixed":
        return [MIXED_CYCLE[i % 8] % R for i in range(n)]
    raise KeyError(name)


@functools.lru_cache(None)
def _multiple_lem(k):
    return bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, k))  # k == 0: the zero point, 64 zero bytes


@functools.lru_cache(None)
def srs_bytes(name, power):
    """section 2 of the pattern's ptau: 2^(power+1) - 1 points, 64 B each"""
    return b"".join(_multiple_lem(k) for k in multipliers(name, (1 << (power + 1)) - 1))


def points(name, n):
    """the first n points, affine (None: the zero point)"""
    b = srs_bytes(name, max(1, (n - 1).bit_length()))
    return [bn.g1_from_lem(b[64 * i:64 * i + 64]) for i in range(n)]


def write_ptau(path, name, power):
    """the pattern as a ptau file (layout of oracle.ptau.write_synthetic_ptau; the G2 section holds
    [tau]_2 of the pattern's trapdoor, [1]_2 for `mixed`, which has none)"""
    sec1 = struct.pack("<I", 32) + bn.Q.to_bytes(32, "little") + struct.pack("<II", power, power)
    sec3 = bn.g2_to_lem(bn.G2_GEN) + bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, TAUS.get(name, 1)))
    with open(path, "wb") as fh:
        fh.write(b"ptau" + struct.pack("<II", 1, 3))
        for sid, payload in ((1, sec1), (2, srs_bytes(name, power)), (3, sec3)):
            fh.write(struct.pack("<IQ", sid, len(payload)))
            fh.write(payload)


@contextlib.contextmanager
def ptau_file(name, power, tag=""):
    """a ptau of the caller's own under /tmp, removed on exit"""
    path = f"/tmp/kgs_test_degen_{name}_p{power}{tag}.{os.getpid()}.ptau"
    try:
        write_ptau(path, name, power)
        yield path
    finally:
        if os.path.exists(path):
            os.remove(path)


def expected(name, scalars):
    """closed form of MSM(pattern's points, scalars), 64 B LEM"""
    acc = 0
    for s, k in zip(scalars, multipliers(name, len(scalars))):
        acc += s * k
    return _multiple_lem(acc % R)


# ------------------------------------------------------------------ scalar families
# c: the window of the resident tables (signed digits in [-2^(c-1) + 1, 2^(c-1)]; a digit above
# 2^(c-1) becomes digit - 2^c with a carry into the next window, so 2^c - d has digits (-d, +1)).
D = 5  # a small digit: bucket 5 of window 0, below 2^(c-1) for every c >= 7


def windows(c):
    return (255 + c - 1) // c


def equal_small(c, n, neg=False):
    """n copies of d (neg: of 2^c - d, i.e. digit -d in window 0 and +1 in window 1)"""
    return [(1 << c) - D if neg else D] * n


def cancel(c, k):
    """k copies of d, then k of 2^c - d: bucket d holds k points and their k opposites"""
    return [D] * k + [(1 << c) - D] * k


def cancel_restart(c):
    return [D, (1 << c) - D, D]


def ramp(n):
    """1 .. n: one point per bucket while n <= 2^(c-1)"""
    return list(range(1, n + 1))


def identity_buckets(c, m):
    """i and 2^c - i for i in 1..m: every bucket 1..m sums to the zero point; window 1 holds m points"""
    out = []
    for i in range(1, m + 1):
        out += [i, (1 << c) - i]
    return out


def digit_edges(c):
    """scalars at the edges of the signed-digit recoding; the last two have the maximal top digit,
    without and with a carry that ripples through every window"""
    sh = (windows(c) - 1) * c
    top = (R >> sh) << sh
    return [1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1, 1 << c, R - 1, R - (1 << (c - 1)), top, top - 1]


def random_scalars(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def small_families(c):
    """every family at N <= 64, for the CPU test that pins the references: (id, scalars)"""
    out = []
    for n in (2, 3, 4, 5, 64):
        out.append((f"equal-{n}", equal_small(c, n)))
        out.append((f"equal-neg-{n}", equal_small(c, n, True)))
    for k in (1, 2, 3, 32):
        out.append((f"cancel-{k}", cancel(c, k)))
    out.append(("cancel-restart", cancel_restart(c)))
    out.append(("all-equal-even", [random_scalars(1, 7)[0]] * 64))
    for n in (7, 63, 64):
        out.append((f"ramp-{n}", ramp(n)))
    out.append(("identity-buckets", identity_buckets(c, 31)))
    out.append(("digit-edges", digit_edges(c)))
    for i, s in enumerate(digit_edges(c)):
        out.append((f"digit-edge-{i}", [s]))
    for n in (1, 2, 64):
        out.append((f"random-{n}", random_scalars(n, 100 + n)))
    return out
