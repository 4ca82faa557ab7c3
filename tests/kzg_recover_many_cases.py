"""Shared cases of test_kzg_recover_many_refs.py (CPU) and test_gpu_kzg_recover_many.py (GPU): the recovery of many
polynomials of one length from their cells in one call (kgs_kzg_recover_cosets_many), over the references of
kzg_recover_cases.py. A case is a flat list of cells (which polynomial, which coset, l values), shuffled across
the polynomials, with what each polynomial must come back as.

Status of a polynomial: 1 recovered, 0 its cells lie on no polynomial of degree < length, 2 fewer than
ceil(length / l) cells.

blocked_nside restates the size-n side of DESIGN.md §24 on Python integers with butterflies of its own: E Z
scattered to the bit-reversed positions, the inverse transform from bit-reversed order, the twist by g^j, the forward
transform to bit-reversed order, the division at x >> lbits, the inverse and the untwist.
"""
import random

import kzg_recover_cases as C
import ntt_cases as T
from oracle import bn254 as bn
from oracle import poly as OP

R = C.R
OK, NO_POLY, TOO_FEW = 1, 0, 2
LEN_KINDS = C.LEN_KINDS


class Many:
    """poly_of / index / rows: the cells; cells_of[b] = (index, rows) of polynomial b in the order the flat list holds
    them; expect[b] = (status, coefficients or None)"""

    def __init__(self, nbits, lbits, length, per_poly, expect, rng):
        self.nbits, self.lbits, self.length, self.polys = nbits, lbits, length, len(per_poly)
        cells = [(b, i, row) for b, (index, rows) in enumerate(per_poly) for i, row in zip(index, rows)]
        rng.shuffle(cells)
        self.poly_of = [c[0] for c in cells]
        self.index = [c[1] for c in cells]
        self.rows = [c[2] for c in cells]
        self.cells_of = [([i for b, i, _ in cells if b == p], [r for b, _, r in cells if b == p])
                         for p in range(self.polys)]
        self.expect = expect

    def status(self):
        return [s for s, _ in self.expect]


def need(length, lbits):
    return (length + (1 << lbits) - 1) >> lbits


def make_many(seed, nbits, lbits, polys, shared=False, len_kind="odd", first_pattern=0):
    """polys recoverable polynomials of one length: per-polynomial patterns cycling through C.PATTERNS (all "none"
    for the length n), or one set shared by all"""
    n, l, m = C.sizes(nbits, lbits)
    rng = random.Random(seed)
    if len_kind == "max":
        sets = [list(range(m)) for _ in range(polys)]
    elif shared:
        pattern = C.PATTERNS[(first_pattern + seed) % len(C.PATTERNS)]
        sets = [C.present_cosets(pattern, m, rng, len_kind)] * polys
    else:
        sets = [C.present_cosets(C.PATTERNS[(first_pattern + b) % len(C.PATTERNS)], m, rng, len_kind) for b in range(polys)]
    length = C.length_for(min(len(s) for s in sets) * l, l, len_kind) if polys else 1
    per_poly, expect = [], []
    for s in sets:
        index, rows, _, coefs = C.case_from(s, nbits, lbits, length, rng)
        per_poly.append((index, rows))
        expect.append((OK, coefs))
    return Many(nbits, lbits, length, per_poly, expect, rng)


def from_sets(seed, nbits, lbits, sets, length):
    """recoverable polynomials over the given sets of present cosets"""
    rng = random.Random(seed)
    per_poly, expect = [], []
    for s in sets:
        index, rows, _, coefs = C.case_from(s, nbits, lbits, length, rng)
        per_poly.append((index, rows))
        expect.append((OK, coefs))
    return Many(nbits, lbits, length, per_poly, expect, rng)


STATUS_KINDS = ("recovered", "tampered", "lagrange", "too few", "none", "recovered")


def make_statuses(seed, nbits, lbits, sets=None):
    """One call with every status (m >= 4): length = l m / 2, so ceil(length / l) = m / 2 cells are the minimum.
    recovered: more than the minimum; tampered: cells to spare and one wrong value (0); lagrange: exactly the minimum
    and one wrong value, which is then the interpolant's (1); too few: m / 2 - 1 cells (2); none (2).
    sets: the present cosets of the two recovered and the tampered polynomial (each more than m / 2), else random."""
    n, l, m = C.sizes(nbits, lbits)
    assert m >= 4
    rng = random.Random(seed)
    length = l * (m // 2)
    per_poly, expect = [], []
    spare = iter(sets or [])
    for kind in STATUS_KINDS:
        if kind in ("recovered", "tampered"):
            s = next(spare, None) or rng.sample(range(m), rng.randint(m // 2 + 1, m))
            assert len(s) > m // 2
        elif kind == "lagrange":
            s = rng.sample(range(m), m // 2)
        elif kind == "too few":
            s = rng.sample(range(m), m // 2 - 1)
        else:
            s = []
        index, rows, _, coefs = C.case_from(s, nbits, lbits, length, rng)
        if kind in ("tampered", "lagrange"):
            k, j = rng.randrange(len(rows)), rng.randrange(l)
            rows[k][j] = (rows[k][j] + 1 + rng.randrange(R - 1)) % R
        per_poly.append((index, rows))
        if kind == "recovered":
            expect.append((OK, coefs))
        elif kind == "tampered":
            expect.append((NO_POLY, None))
        elif kind == "lagrange":
            expect.append((OK, C.steps(index, rows, nbits, lbits, length)[1]))
        else:
            expect.append((TOO_FEW, None))
    return Many(nbits, lbits, length, per_poly, expect, rng)


def reference(case, b, with_lagrange=None):
    """(status, coefficients or None) of polynomial b from its own cells by kzg_recover_cases' references"""
    index, rows = case.cells_of[b]
    if len(index) < need(case.length, case.lbits):
        return TOO_FEW, None
    verdict, coefs = C.steps(index, rows, case.nbits, case.lbits, case.length)
    if case.nbits <= 5 if with_lagrange is None else with_lagrange:
        assert C.lagrange(index, rows, case.nbits, case.lbits, case.length)[0] == verdict
        if verdict:
            assert C.lagrange(index, rows, case.nbits, case.lbits, case.length)[1] == coefs
    return (OK, coefs) if verdict else (NO_POLY, None)


# ------------------------------------------------------------------ the blocked size-n side on integers
def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def dif(a, logn, inverse=False):
    """natural order in, bit-reversed order out (no scaling)"""
    a, n = list(a), 1 << logn
    for lg in range(logn, 0, -1):
        h = 1 << (lg - 1)
        w = bn.FR_W[lg] if not inverse else pow(bn.FR_W[lg], R - 2, R)
        for s in range(0, n, 2 * h):
            wt = 1
            for t in range(h):
                u, v = a[s + t], a[s + t + h]
                a[s + t], a[s + t + h] = (u + v) % R, (u - v) * wt % R
                wt = wt * w % R
    return a


def dit(a, logn, inverse=False):
    """bit-reversed order in, natural order out; the inverse includes 1 / n"""
    a, n = list(a), 1 << logn
    for lg in range(1, logn + 1):
        h = 1 << (lg - 1)
        w = bn.FR_W[lg] if not inverse else pow(bn.FR_W[lg], R - 2, R)
        for s in range(0, n, 2 * h):
            wt = 1
            for t in range(h):
                u, v = a[s + t], a[s + t + h] * wt % R
                a[s + t], a[s + t + h] = (u + v) % R, (u - v) % R
                wt = wt * w % R
    if inverse:
        ninv = pow(n, R - 2, R)
        a = [x * ninv % R for x in a]
    return a


def blocked_nside(index, rows, nbits, lbits, length):
    """(verdict, coefficients) as C.steps gives them, by the positions and orders the batched call uses per block"""
    n, l, m = C.sizes(nbits, lbits)
    logm = nbits - lbits
    g = T.COSET_GEN
    have = set(index)
    z = C.vanishing([i for i in range(m) if i not in have], nbits, lbits)
    zc = z + [0] * (m - len(z))
    gl = pow(g, l, R)
    zev = dif(zc, logm)                                                     # z(a_i) at bitrev_m(i)
    zsh = dif([c * pow(gl, t, R) % R for t, c in enumerate(zc)], logm)      # z(g^l a_i) at bitrev_m(i)
    inv = OP.batch_inverse(zsh)
    assert all(inv)
    row_of = {i: k for k, i in enumerate(index)}
    a = [0] * n
    for o in range(n):  # the scatter, by output position
        u = o >> lbits
        i, j = bitrev(u, logm), bitrev(o & (l - 1), lbits)
        assert bitrev(o, nbits) == i + m * j
        if i in row_of:
            a[o] = rows[row_of[i]][j] * zev[u] % R
    a = dit(a, nbits, inverse=True)
    a = dif([c * pow(g, j, R) % R for j, c in enumerate(a)], nbits)
    a = dit([v * inv[x >> lbits] % R for x, v in enumerate(a)], nbits, inverse=True)
    gi = pow(g, R - 2, R)
    high = any(a[length:])
    return (0 if high else 1), [c * pow(gi, j, R) % R for j, c in enumerate(a[:length])]
