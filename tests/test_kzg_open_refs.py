"""The references of kzg_open_cases.py pinned to each other and to oracle/poly.py's division (nbits 0 .. 6,
0 / 1 / n/2 + 1 / n coefficients, the degenerate taus), and what of the opening API runs without a GPU:
kgs_kzg_verify against oracle points, valid and tampered, the host path of kgs_g1_mul_each, and the argument
errors that need no device. No GPU is touched."""
import ctypes
import random

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
import kzg_open_cases as Z
from oracle import poly

R = N.R
KGS_E_ARG = -1


def K():
    return common.load_pkg()


def coefs(nbits, count, seed=0):
    rnd = random.Random(1000 * nbits + count + seed)
    return [rnd.randrange(R) for _ in range(count)]


def counts(nbits):
    n = 1 << nbits
    return sorted({0, 1, min(n // 2 + 1, n), n})


# ------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("nbits", range(7))
def test_three_forms_agree(nbits):
    for count in counts(nbits):
        c = coefs(nbits, count)
        want = Z.closed_form(c, nbits)
        assert Z.quotient_scalars(c, nbits, common.tau()) == want, count
        h, pi = Z.toeplitz_steps(c, nbits)
        assert pi == want, count
        # h_k is the coefficient of w^(ik) in pi_i: the commitment to the k-th "shifted" polynomial
        tp = N.tau_powers(1 << nbits)
        assert h == [sum(c[j] * tp[j - 1 - k] for j in range(k + 1, len(c))) % R for k in range((1 << nbits) - 1)]
        assert Z.open_all_scalars(c, nbits) == want


@pytest.mark.parametrize("nbits", [1, 3, 6])
def test_quotient_is_the_oracles_division(nbits):
    n = 1 << nbits
    c = coefs(nbits, n, 5)
    for z in (N.omegas(nbits)[n // 2 + (n > 2)], 12345, 0):
        y = Z.poly_eval(c, z)
        assert y == poly.Polynomial(c).evaluate(z)
        p = poly.Polynomial(c).sub_scalar(y)
        assert p.div_by_x_sub_value(z).coef == Z.quotient_coeffs(c, z) + [0]


@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_taus_quotient_form(name):
    """tau in {1, r - 1, a 4th root of unity, 0}: inside the domain (or zero) the closed form divides by
    zero; the quotient form and the Toeplitz route do not, and agree"""
    tau = D.TAUS[name]
    for nbits in (0, 1, 2, 3, 6):
        for count in counts(nbits):
            c = coefs(nbits, count, 9)
            want = Z.quotient_scalars(c, nbits, tau)
            assert Z.toeplitz_steps(c, nbits, tau)[1] == want, (nbits, count)
            assert Z.open_all_scalars(c, nbits, tau) == want
            if pow(tau, 1 << nbits, R) != 1:
                assert Z.closed_form(c, nbits, tau) == want


def test_evals_and_mont_round_trip():
    c = coefs(4, 9)
    assert Z.evals(c, 4) == [Z.poly_eval(c, w) for w in N.omegas(4)]
    assert Z.from_mont(Z.mont(c)) == c


# ------------------------------------------------------------------ kgs_kzg_verify (host only)
def test_kzg_verify_valid_and_tampered():
    k = K()
    nbits = 3
    c = coefs(nbits, 8, 2)
    C, t2 = Z.commitment(c), Z.tau_g2()
    pi = Z.closed_form(c, nbits)
    ws = N.omegas(nbits)
    for i in (0, 3, 7):
        z, y, proof = Z.mont([ws[i]]), Z.mont([Z.poly_eval(c, ws[i])]), N.point(pi[i])
        assert k.kzg_verify(t2, C, z, y, proof) is True
        assert k.kzg_verify(common.oracle_ptau(6), C, z, y, proof) is True  # [tau]_2 read from the file
        assert k.kzg_verify(t2, C, z, Z.mont([Z.poly_eval(c, ws[i]) + 1]), proof) is False
        assert k.kzg_verify(t2, C, Z.mont([ws[i] + 1]), y, proof) is False
        assert k.kzg_verify(t2, C, z, y, N.point(pi[i] + 1)) is False  # another point of the curve
        assert k.kzg_verify(t2, N.point(5), z, y, proof) is False
        bad = bytearray(proof)
        bad[5] ^= 1  # off the curve
        assert k.kzg_verify(t2, C, z, y, bytes(bad)) is False
    z = 987654321  # off the domain
    y, proof = Z.poly_eval(c, z), N.point(Z.quotient_form(c, z, common.tau()))
    assert k.kzg_verify(t2, C, Z.mont([z]), Z.mont([y]), proof) is True
    # a constant polynomial opens with the identity; the zero polynomial commits to it too
    assert k.kzg_verify(t2, N.point(7), Z.mont([z]), Z.mont([7]), bytes(64)) is True
    assert k.kzg_verify(t2, bytes(64), Z.mont([z]), Z.mont([0]), bytes(64)) is True
    assert k.kzg_verify(t2, bytes(64), Z.mont([z]), Z.mont([1]), bytes(64)) is False
    # non-canonical scalars are invalid, not an error
    assert k.kzg_verify(t2, C, R.to_bytes(32, "little"), Z.mont([y]), proof) is False


def test_kzg_verify_argument_errors():
    k = K()
    L = k.lib()
    b64, b32, t2 = bytes(64), bytes(32), Z.tau_g2()
    assert L.kgs_kzg_verify(None, b32, b32, b64, t2) == KGS_E_ARG
    assert L.kgs_kzg_verify(b64, b32, b32, b64, None) == KGS_E_ARG
    bad = bytearray(t2)
    bad[3] ^= 1
    assert L.kgs_kzg_verify(b64, b32, b32, b64, bytes(bad)) == KGS_E_ARG  # [tau]_2 off its curve
    with pytest.raises(ValueError):
        k.kzg_verify(t2, b64, b32, b32, bytes(63))


# ------------------------------------------------------------------ kgs_g1_mul_each, host path
@pytest.mark.parametrize("n", [1, 5, 40])
def test_g1_mul_each_host(n):
    k = K()
    mult, s = Z.mul_each_case(n, 30 + n)
    got = k.g1_mul_each(N.points(mult), N.scalar_bytes(s), device=None)
    assert got == Z.mul_each_expected(mult, s)
    if n == 40:
        assert bytes(64) in (got[0:64], got[64 * 20:64 * 21])  # identities in, identities out
        assert all(e in s for e in Z.EDGE_SCALARS)


def test_g1_mul_each_host_arguments():
    k = K()
    L = k.lib()
    assert k.g1_mul_each(b"", b"", device=None) == b""
    with pytest.raises(ValueError):
        k.g1_mul_each(N.point(1), bytes(64), device=None)
    p, s, o = ctypes.create_string_buffer(N.point(1) * 2, 128), ctypes.create_string_buffer(64), \
        ctypes.create_string_buffer(128)
    for args in ((None, s, 2, o), (p, None, 2, o), (p, s, 2, None), (p, s, (1 << 26) + 1, o)):
        assert L.kgs_g1_mul_each(None, *args) == KGS_E_ARG
    assert L.kgs_g1_mul_each_device(None, p, s, 2, o) == KGS_E_ARG and "ctx" in L.kgs_last_error().decode()
    # in place
    buf = ctypes.create_string_buffer(N.point(3) + N.point(4), 128)
    assert L.kgs_g1_mul_each(None, buf, N.scalar_bytes([5, R + 2]), 2, buf) == 0
    assert buf.raw == N.point(15) + N.point(8)


def test_context_entry_points_need_a_context():
    L = K().lib()
    b = ctypes.create_string_buffer(64)
    rc = L.kgs_kzg_open(None, b, 1, b, b, b)
    assert rc == KGS_E_ARG and "ctx" in L.kgs_last_error().decode()
    for fn in (L.kgs_kzg_open_all, L.kgs_kzg_open_all_device):
        rc = fn(None, b, 1, 0, b, None)
        assert rc == KGS_E_ARG and "ctx" in L.kgs_last_error().decode()
