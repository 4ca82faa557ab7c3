"""The references of kzg_coset_cases.py pinned to each other (nbits 0 .. 6, every lbits, 0 / 1 / n/2 + 1 / n
coefficients, the degenerate taus) and to kzg_open_cases at lbits = 0, and what of the coset API runs without
a GPU: the host path of kgs_g1_mul_sum, kgs_kzg_verify_coset against oracle points, valid and tampered, and
kgs_ptau_read_tau_g2_pow on small files the test writes. No GPU is touched."""
import ctypes
import random
import struct

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
import kzg_coset_cases as C
import kzg_open_cases as Z
from oracle import bn254 as bn

R = N.R
KGS_E_ARG, KGS_E_IO = -1, -6


def K():
    return common.load_pkg()


def coefs(nbits, count, seed=0):
    rnd = random.Random(3000 * nbits + count + seed)
    return [rnd.randrange(R) for _ in range(count)]


def counts(nbits):
    n = 1 << nbits
    return sorted({0, 1, min(n // 2 + 1, n), n})


# ------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("nbits", range(7))
def test_three_forms_agree(nbits):
    for lbits in range(nbits + 1):
        n, l, m = C.sizes(nbits, lbits)
        for count in counts(nbits):
            c = coefs(nbits, count, lbits)
            a = C.division_scalars(c, nbits, lbits)
            assert C.closed_scalars(c, nbits, lbits) == a, (lbits, count)
            h, pi = C.library_steps(c, nbits, lbits)
            assert pi == a, (lbits, count)
            assert h == C.h_direct(c, nbits, lbits), (lbits, count)
            assert C.open_cosets_scalars(c, nbits, lbits) == a
            if m == 1:
                assert a == [0]


@pytest.mark.parametrize("nbits", range(7))
def test_lbits_zero_is_open_all(nbits):
    for count in counts(nbits):
        c = coefs(nbits, count, 77)
        assert C.division_scalars(c, nbits, 0) == Z.open_all_scalars(c, nbits), count
        assert C.library_steps(c, nbits, 0)[1] == Z.toeplitz_steps(c, nbits)[1]


@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_taus(name):
    """tau in {1, r - 1, a 4th root of unity, 0}: tau^l can be one of the a_i, where the closed form divides by
    zero; the long division and the library's route do not, and agree"""
    tau = D.TAUS[name]
    for nbits in (0, 1, 2, 3, 5):
        for lbits in range(nbits + 1):
            for count in counts(nbits):
                c = coefs(nbits, count, 9)
                want = C.division_scalars(c, nbits, lbits, tau)
                assert C.library_steps(c, nbits, lbits, tau)[1] == want, (nbits, lbits, count)
                assert C.open_cosets_scalars(c, nbits, lbits, tau) == want


def test_coset_geometry():
    """psi = w^m = Fr.w[lbits] generates the coset's subgroup; a_i = w^(i l) is what X^l takes on H_i; the
    remainder of the long division is the interpolant of the values"""
    for nbits, lbits in ((3, 0), (3, 1), (4, 2), (5, 5), (6, 3)):
        n, l, m = C.sizes(nbits, lbits)
        assert pow(bn.FR_W[nbits], m, R) == bn.FR_W[lbits]
        c = coefs(nbits, n, 4)
        ev = Z.evals(c, nbits)
        for i in {0, 1 % m, m - 1}:
            pts = C.coset_points(nbits, lbits, i)
            assert pts == [pow(bn.FR_W[nbits], i, R) * pow(bn.FR_W[lbits], j, R) % R for j in range(l)]
            assert all(pow(z, l, R) == C.a_of(nbits, lbits, i) for z in pts)
            ys = C.coset_values(ev, nbits, lbits, i)
            assert ys == [Z.poly_eval(c, z) for z in pts]
            d = C.interpolant(ys, nbits, lbits, i)
            assert [Z.poly_eval(d, z) for z in pts] == ys
            q, rem = C.divide(c, l, C.a_of(nbits, lbits, i))
            assert rem == d
            pi = Z.poly_eval(q, common.tau())
            assert C.check_identity(c, nbits, lbits, i, ys, pi)
            assert not C.check_identity(c, nbits, lbits, i, ys, pi + 1)


# ------------------------------------------------------------------ kgs_g1_mul_sum, host path
@pytest.mark.parametrize("rows,cols", [(1, 5), (2, 7), (3, 4), (5, 8), (8, 1)])
def test_g1_mul_sum_host(rows, cols):
    k = K()
    mult, s = C.mul_sum_case(rows, cols, 50 + rows)
    got = k.g1_mul_sum(N.points(mult), N.scalar_bytes(s), rows, device=None)
    assert got == C.mul_sum_expected(mult, s, rows)
    if rows == 1:
        assert got == k.g1_mul_each(N.points(mult), N.scalar_bytes(s), device=None)


def test_g1_mul_sum_host_sum_paths():
    k = K()
    # a column of equal terms, a column of pairs k P, (r - k) P, a column of identities
    mult = [3, 5, 0] * 4
    s = [7, 9, 11] * 2 + [7, R - 9, 4] * 2
    assert k.g1_mul_sum(N.points(mult), N.scalar_bytes(s), 4, device=None) == N.point(84) + bytes(128)


def test_g1_mul_sum_host_arguments():
    k = K()
    L = k.lib()
    assert k.g1_mul_sum(b"", b"", 3, device=None) == b""
    with pytest.raises(ValueError):
        k.g1_mul_sum(N.point(1) * 3, bytes(96), 2, device=None)
    p, s, o = ctypes.create_string_buffer(N.point(1) * 2, 128), ctypes.create_string_buffer(64), \
        ctypes.create_string_buffer(128)
    for args in ((None, s, 2, 1, o), (p, None, 2, 1, o), (p, s, 2, 1, None), (p, s, 0, 2, o),
                 (p, s, (1 << 13) + 1, 1 << 13, o), (p, s, 1 << 40, 1 << 40, o)):
        assert L.kgs_g1_mul_sum(None, *args) == KGS_E_ARG
    assert L.kgs_g1_mul_sum_device(None, p, s, 2, 1, o) == KGS_E_ARG and "ctx" in L.kgs_last_error().decode()


# ------------------------------------------------------------------ kgs_kzg_verify_coset (host only)
@pytest.mark.parametrize("nbits,lbits", [(3, 0), (3, 1), (3, 3), (5, 2)])
def test_kzg_verify_coset_valid_and_tampered(nbits, lbits):
    k = K()
    n, l, m = C.sizes(nbits, lbits)
    c = coefs(nbits, n, 2)
    cm, t2, srs = Z.commitment(c), C.tau_l_g2(lbits), C.srs_g1(lbits)
    pi = C.closed_scalars(c, nbits, lbits)
    ev = Z.evals(c, nbits)
    for i in sorted({0, m // 2, m - 1}):
        ys = C.coset_values(ev, nbits, lbits, i)
        ym, proof = Z.mont(ys), N.point(pi[i])
        assert k.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, ym, proof) is True
        if m > 1:
            assert k.kzg_verify_coset(t2, srs, cm, nbits, lbits, (i + 1) % m, ym, proof) is False  # a wrong index
        bad = list(ys)
        bad[l // 2] = (bad[l // 2] + 1) % R
        assert k.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, Z.mont(bad), proof) is False  # one changed y
        assert k.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, ym, N.point(pi[i] + 1)) is False  # a changed proof
        off = bytearray(proof if any(proof) else N.point(1))
        off[5] ^= 1
        assert k.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, ym, bytes(off)) is False  # off the curve
        big = bytearray(ym)
        big[32 * (l - 1):32 * l] = R.to_bytes(32, "little")
        assert k.kzg_verify_coset(t2, srs, cm, nbits, lbits, i, bytes(big), proof) is False  # a y >= r
        assert k.kzg_verify_coset(t2, srs, N.point(5), nbits, lbits, i, ym, proof) is False
    if lbits == 0:  # the one-point check accepts the same proof
        z, y = Z.mont([N.omegas(nbits)[1 % n]]), Z.mont([ev[1 % n]])
        assert k.kzg_verify(Z.tau_g2(), cm, z, y, N.point(pi[1 % n])) is True


def test_kzg_verify_coset_argument_errors():
    k = K()
    L = k.lib()
    b64, b32, t2 = bytes(64), bytes(64), C.tau_l_g2(1)
    good = (b64, 3, 1, 0, b32, b64, b64 * 2, t2)
    assert L.kgs_kzg_verify_coset(*good) in (0, 1)
    for pos in (0, 4, 5, 6, 7):
        args = list(good)
        args[pos] = None
        assert L.kgs_kzg_verify_coset(*args) == KGS_E_ARG, pos
    bad = bytearray(t2)
    bad[3] ^= 1
    assert L.kgs_kzg_verify_coset(*good[:7], bytes(bad)) == KGS_E_ARG  # [tau^l]_2 off its curve
    for nbits, lbits, index in ((-1, 0, 0), (29, 1, 0), (3, 4, 0), (3, -1, 0), (3, 1, 4)):
        assert L.kgs_kzg_verify_coset(b64, nbits, lbits, index, b32, b64, b64 * 2, t2) == KGS_E_ARG
    with pytest.raises(ValueError):
        k.kzg_verify_coset(t2, b64 * 2, b64, 3, 1, 0, bytes(32), b64)


# ------------------------------------------------------------------ kgs_ptau_read_tau_g2_pow
def _small_ptau(path, g2_count):
    """a ptau with one G1 point and g2_count points [tau^k]_2"""
    tau = common.tau()
    sec1 = struct.pack("<I", 32) + bn.Q.to_bytes(32, "little") + struct.pack("<II", 1, 1)
    sec3 = b"".join(bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, pow(tau, k, R))) for k in range(g2_count))
    with open(path, "wb") as fh:
        fh.write(b"ptau" + struct.pack("<II", 1, 3))
        for sid, payload in ((1, sec1), (2, N.point(1)), (3, sec3)):
            fh.write(struct.pack("<IQ", sid, len(payload)))
            fh.write(payload)


def test_ptau_read_tau_g2_pow(tmp_path):
    k = K()
    L = k.lib()
    lbits = 2
    path = str(tmp_path / "g2.ptau")
    _small_ptau(path, (1 << lbits) + 1)
    assert k.ptau_read_tau_g2_pow(path, 0) == bn.g2_to_lem(bn.G2_GEN)
    assert k.ptau_read_tau_g2_pow(path, 1) == Z.tau_g2()
    assert k.ptau_read_tau_g2_pow(path, 1 << lbits) == C.tau_l_g2(lbits)
    t2 = ctypes.create_string_buffer(128)
    assert L.kgs_ptau_read_tau_g2(path.encode(), t2) == 0 and t2.raw == Z.tau_g2()
    with pytest.raises(k.KgsError) as e:
        k.ptau_read_tau_g2_pow(path, (1 << lbits) + 1)
    assert e.value.code == KGS_E_IO
    # kzg_verify_coset reads [tau^l]_2 from the file by itself
    nbits = 4
    c = coefs(nbits, 16, 8)
    pi = C.closed_scalars(c, nbits, lbits)
    ys = C.coset_values(Z.evals(c, nbits), nbits, lbits, 3)
    assert k.kzg_verify_coset(path, C.srs_g1(lbits), Z.commitment(c), nbits, lbits, 3, Z.mont(ys), N.point(pi[3])) is True
    two = str(tmp_path / "two.ptau")
    _small_ptau(two, 2)
    assert k.ptau_read_tau_g2_pow(two, 1) == Z.tau_g2()
    assert L.kgs_ptau_read_tau_g2_pow(two.encode(), 2, t2) == KGS_E_IO
    assert L.kgs_ptau_read_tau_g2_pow(None, 1, t2) == KGS_E_ARG
    assert L.kgs_ptau_read_tau_g2_pow(two.encode(), 1, None) == KGS_E_ARG


def test_context_entry_points_need_a_context():
    L = K().lib()
    b = ctypes.create_string_buffer(64)
    for fn in (L.kgs_kzg_open_cosets, L.kgs_kzg_open_cosets_device):
        rc = fn(None, b, 1, 0, 0, b, None)
        assert rc == KGS_E_ARG and "ctx" in L.kgs_last_error().decode()
