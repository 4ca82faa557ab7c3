"""Shared references of test_kzg_recover_refs.py (CPU) and test_gpu_kzg_recover.py (GPU): the recovery of a
polynomial of known length from a subset of its cosets (kgs_kzg_recover_cosets), on Python integers.
n = 2^nbits, l = 2^lbits, m = n / l, w = Fr.w[nbits]; coset i < m is { w^(i + m j) : j < l }, the zeros of
X^l - a_i with a_i = w^(i l). Row k of the input holds y_{k,j} = p(w^(index[k] + m j)).

  (a) lagrange   the interpolant through the count * l points, by the master polynomial and one synthetic
                 division per point; consistent iff its coefficients from `length` on vanish
  (b) steps      DESIGN.md §22: Z = z(X^l) with z = prod over the missing cosets of (Y - a_i) multiplied out term by
                 term, R = INTT(E Z), R on the coset g <w>, divided there by z(g^l a_i), back to coefficients
                 q; consistent iff q_j = 0 for j >= length. Transforms: oracle/poly.py ntt

A case is made from a seeded polynomial and a named pattern of missing cosets, so the expected coefficients are
the ones it was built from.
"""
import random

import ntt_cases as T
from oracle import bn254 as bn
from oracle import poly as OP

R = bn.R
PATTERNS = ("none", "minimum", "run", "alternate", "random", "shuffled")
LEN_KINDS = ("odd", "max", "one")


def sizes(nbits, lbits):
    assert 0 <= lbits <= nbits
    return 1 << nbits, 1 << lbits, 1 << (nbits - lbits)


def evals(coefs, nbits):
    n = 1 << nbits
    return OP.ntt(list(coefs) + [0] * (n - len(coefs)), False)


def rows_of(ev, nbits, lbits, index):
    n, l, m = sizes(nbits, lbits)
    return [[ev[i + m * j] for j in range(l)] for i in index]


def length_for(cap, l, kind):
    """a length <= cap = count * l: the whole capacity, one, or an odd one that is no multiple of l (l > 1)"""
    if kind == "max":
        return cap
    if kind == "one":
        return 1
    if l > 1:
        return cap - 1
    return cap if cap % 2 else max(cap - 1, 1)


def present_cosets(pattern, m, rng, len_kind="odd"):
    """the given cosets of a named pattern, in the order they are handed over"""
    if pattern == "none":
        return list(range(m))
    if pattern == "minimum":  # the length is then chosen so that ceil(len / l) == count
        return sorted(rng.sample(range(m), 1 if len_kind == "one" else rng.randint(1, m)))
    if pattern == "run":  # a contiguous run missing
        k = rng.randint(1, m - 1) if m > 1 else 0
        s = rng.randint(0, m - k)
        return [i for i in range(m) if not s <= i < s + k]
    if pattern == "alternate":
        return list(range(0, m, 2))
    got = [i for i in range(m) if rng.random() < 0.5] or [rng.randrange(m)]
    if pattern == "shuffled":
        rng.shuffle(got)
    return got


def case_from(index, nbits, lbits, length, rng):
    coefs = [rng.randrange(R) for _ in range(length)]
    return list(index), rows_of(evals(coefs, nbits), nbits, lbits, index), length, coefs


def make_case(seed, nbits, lbits, pattern, len_kind="odd"):
    """(index, rows, length, coefs): rows[k][j] = p(w^(index[k] + m j)) for the seeded p of `length` coefficients"""
    n, l, m = sizes(nbits, lbits)
    rng = random.Random(seed)
    index = present_cosets(pattern, m, rng, len_kind)
    cap = len(index) * l
    if pattern == "minimum":
        length = cap - 1 if len_kind == "odd" and l > 1 else cap
    else:
        length = length_for(cap, l, len_kind)
    return case_from(index, nbits, lbits, length, rng)


def flat(rows):
    return [y for row in rows for y in row]


# ------------------------------------------------------------------ (a) Lagrange
def lagrange(index, rows, nbits, lbits, length):
    """(verdict, coefficients): the interpolant through all the points, cut to `length`"""
    n, l, m = sizes(nbits, lbits)
    w = bn.FR_W[nbits]
    xs = [pow(w, i + m * j, R) for i in index for j in range(l)]
    ys = flat(rows)
    N = len(xs)
    master = [1]
    for x in xs:  # times (X - x)
        master = [((master[k - 1] if k else 0) - x * (master[k] if k < len(master) else 0)) % R
                  for k in range(len(master) + 1)]
    out = [0] * N
    for x, y in zip(xs, ys):
        q = [0] * N  # master / (X - x), top down
        acc = 0
        for k in range(N, 0, -1):
            acc = (master[k] + x * acc) % R
            q[k - 1] = acc
        den = 0
        for c in reversed(q):
            den = (den * x + c) % R
        f = y * pow(den, R - 2, R) % R
        for k in range(N):
            out[k] = (out[k] + f * q[k]) % R
    return (1 if not any(out[length:]) else 0), out[:length]


# ------------------------------------------------------------------ (b) the steps of DESIGN.md §22
def vanishing(missing, nbits, lbits):
    """z(Y) = prod (Y - a_i), low coefficient first (leading 1 included)"""
    wl = bn.FR_W[nbits - lbits]
    z = [1]
    for i in missing:
        a = pow(wl, i, R)
        z = [((z[k - 1] if k else 0) - a * (z[k] if k < len(z) else 0)) % R for k in range(len(z) + 1)]
    return z


def steps(index, rows, nbits, lbits, length):
    n, l, m = sizes(nbits, lbits)
    g = T.COSET_GEN
    have = set(index)
    z = vanishing([i for i in range(m) if i not in have], nbits, lbits)
    zc = z + [0] * (m - len(z))
    z_on = OP.ntt(zc, False)                                                   # z(a_i)
    gl = pow(g, l, R)
    z_sh = OP.ntt([c * pow(gl, t, R) % R for t, c in enumerate(zc)], False)    # z(g^l a_i)
    ez = [0] * n
    for k, i in enumerate(index):
        for j in range(l):
            ez[i + m * j] = rows[k][j] * z_on[i] % R
    r = OP.ntt(ez, True)
    on_coset = OP.ntt([c * pow(g, j, R) % R for j, c in enumerate(r)], False)  # R(g w^k)
    inv = OP.batch_inverse(z_sh)
    assert all(inv)
    q = OP.ntt([v * inv[k % m] % R for k, v in enumerate(on_coset)], True)
    gi = pow(g, R - 2, R)
    q = [c * pow(gi, j, R) % R for j, c in enumerate(q)]
    return (1 if not any(q[length:]) else 0), q[:length]
