"""Shared references of test_kzg_coset_refs.py (CPU) and test_gpu_kzg_cosets.py (GPU): the coset openings of a
polynomial p = sum_j c_j X^j (kgs_kzg_open_cosets), in the exponent over an SRS s_k = tau^k G with a known
tau. n = 2^nbits, l = 2^lbits, m = n / l, w = Fr.w[nbits]; coset i < m is H_i = { w^(i + m j) : j < l }, the zeros
of X^l - a_i with a_i = w^(i l); p = q_i (X^l - a_i) + I_i with deg I_i < l and the proof is pi_i = q_i(tau) G.

  (a) long division   q_i by the recurrence q_j = c_(j+l) + a_i q_(j+l) on integers, evaluated at tau. It divides
                      by nothing, so it holds for every tau
  (b) closed form     (p(tau) - I_i(tau)) / (tau^l - a_i), for tau^l != a_i; I_i by interpolation
  (c) library steps   the coefficients and the SRS de-interleaved into l rows, l cyclic convolutions of size 2m
                      summed before ONE inverse transform, h_k = u_(m-1+k), then the transform of size m

An expected point is one oracle scalar multiplication (g1_ntt_cases.point, cached).
"""
import common
import g1_ntt_cases as N
import kzg_open_cases as Z
from oracle import bn254 as bn

R = N.R


def sizes(nbits, lbits):
    assert 0 <= lbits <= nbits
    return 1 << nbits, 1 << lbits, 1 << (nbits - lbits)


def a_of(nbits, lbits, i):
    """a_i = w^(i l): the power of Fr.w[nbits - lbits]"""
    return pow(bn.FR_W[nbits - lbits], i, R)


def coset_points(nbits, lbits, i):
    n, l, m = sizes(nbits, lbits)
    w = bn.FR_W[nbits]
    return [pow(w, i + m * j, R) for j in range(l)]


def coset_values(evals, nbits, lbits, i):
    """y_j = e_(i + m j) of the evaluations in natural order"""
    n, l, m = sizes(nbits, lbits)
    return [evals[i + m * j] for j in range(l)]


# ------------------------------------------------------------------ (a) long division
def divide(c, l, a):
    """(q, rem) with p = q (X^l - a) + rem, deg rem < l: q_j = c_(j+l) + a q_(j+l), top down"""
    c = list(c)
    q = [0] * max(len(c) - l, 0)
    for j in range(len(q) - 1, -1, -1):
        q[j] = (c[j + l] + a * (q[j + l] if j + l < len(q) else 0)) % R
    rem = [(c[k] + a * (q[k] if k < len(q) else 0)) % R if k < len(c) else 0 for k in range(l)]
    return q, rem


def division_scalars(c, nbits, lbits, tau=None):
    tau = common.tau() if tau is None else tau
    n, l, m = sizes(nbits, lbits)
    return [Z.poly_eval(divide(c, l, a_of(nbits, lbits, i))[0], tau) for i in range(m)]


# ------------------------------------------------------------------ the interpolant
def interpolant(ys, nbits, lbits, i):
    """the coefficients d_k of I_i: d_k = w^(-i k) J_k, J the inverse transform of size l of the values"""
    J = N.transform_scalars(list(ys), inverse=True)
    wi = N.inv(pow(bn.FR_W[nbits], i, R))
    return [J[k] * pow(wi, k, R) % R for k in range(len(J))]


# ------------------------------------------------------------------ (b) closed form
def closed_scalars(c, nbits, lbits, tau=None):
    tau = common.tau() if tau is None else tau
    n, l, m = sizes(nbits, lbits)
    ev = Z.evals(c, nbits)
    pt, tl = Z.poly_eval(c, tau), pow(tau, l, R)
    den = [(tl - a_of(nbits, lbits, i)) % R for i in range(m)]
    assert all(den), "tau^l is one of the a_i: use division_scalars"
    di = N.batch_inv(den)
    return [(pt - Z.poly_eval(interpolant(coset_values(ev, nbits, lbits, i), nbits, lbits, i), tau)) * di[i] % R
            for i in range(m)]


# ------------------------------------------------------------------ (c) the library's steps
def library_steps(c, nbits, lbits, tau=None):
    """returns (h, pi): h_0 .. h_(m-2) and the m proofs' scalars"""
    tau = common.tau() if tau is None else tau
    n, l, m = sizes(nbits, lbits)
    assert len(c) <= n
    if m == 1:
        return [], [0]
    c = list(c) + [0] * (n - len(c))
    s = N.tau_powers(n, tau)
    uh = [0] * (2 * m)
    for r in range(l):
        crow = [c[u * l + r] for u in range(m)]
        srow = [s[v * l + r] for v in range(m)]
        x = [srow[m - 2 - j] if j <= m - 2 else 0 for j in range(2 * m)]
        xh = N.transform_scalars(x)
        ch = N.transform_scalars(crow + [0] * m)
        uh = [(acc + a * b) % R for acc, a, b in zip(uh, ch, xh)]  # the rows summed BEFORE the inverse transform
    u = N.transform_scalars(uh, inverse=True)
    h = [u[m - 1 + k] for k in range(m - 1)]
    return h, N.transform_scalars(h + [0])


def h_direct(c, nbits, lbits, tau=None):
    """h_k = sum_{j >= (k+1) l} c_j s_(j - (k+1) l)"""
    tau = common.tau() if tau is None else tau
    n, l, m = sizes(nbits, lbits)
    s = N.tau_powers(n, tau)
    return [sum(c[j] * s[j - (k + 1) * l] for j in range((k + 1) * l, len(c))) % R for k in range(m - 1)]


def open_cosets_scalars(c, nbits, lbits, tau=None):
    """(b) where it is defined, (a) where tau^l is one of the a_i (tau in the domain)"""
    tau = common.tau() if tau is None else tau
    n, l, m = sizes(nbits, lbits)
    tl = pow(tau, l, R)
    if any(tl == a_of(nbits, lbits, i) for i in range(m)):
        return division_scalars(c, nbits, lbits, tau)
    return closed_scalars(c, nbits, lbits, tau)


def expected_proofs(c, nbits, lbits, tau=None):
    return N.points(open_cosets_scalars(c, nbits, lbits, tau))


# ------------------------------------------------------------------ the check, as an integer equation
def check_identity(c, nbits, lbits, i, ys, pi, tau=None):
    """C - I(tau) + a_i pi == tau^l pi in the exponent: what the pairing equation of kgs_kzg_verify_coset says"""
    tau = common.tau() if tau is None else tau
    n, l, m = sizes(nbits, lbits)
    lhs = (Z.poly_eval(c, tau) - Z.poly_eval(interpolant(ys, nbits, lbits, i), tau) + a_of(nbits, lbits, i) * pi) % R
    return lhs == pow(tau, l, R) * pi % R


def tau_l_g2(lbits, tau=None):
    tau = common.tau() if tau is None else tau
    return bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, pow(tau, 1 << lbits, R)))


def srs_g1(lbits, tau=None):
    """the first l points tau^k G"""
    return N.points(N.tau_powers(1 << lbits, tau))


# ------------------------------------------------------------------ kgs_g1_mul_sum
def mul_sum_case(rows, cols, seed):
    """rows * cols terms from kzg_open_cases.mul_each_case: identities at the first, a middle and the last
    index, the edge scalars of the recoding, scalars above r"""
    return Z.mul_each_case(rows * cols, seed)


def mul_sum_expected(k, s, rows):
    cols = len(k) // rows
    return N.points([sum(k[r * cols + i] * s[r * cols + i] for r in range(rows)) % R for i in range(cols)])
