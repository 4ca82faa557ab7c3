"""The G1 transform on the host path (kgs_g1_ntt with ctx == NULL, g1_ntt(device=None)) and the references
of g1_ntt_cases.py: the two closed forms against the naive sum in the exponent, forward and inverse over
tau^i G, round trips, identities among the inputs, the degenerate point families, and every argument
error that needs no GPU. No GPU is touched."""
import ctypes

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
from oracle import ptau as opt

R = N.R
KGS_E_ARG = -1
LOGS = list(range(7))  # 1 .. 64 points


def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def bases():
    return opt.PTau(common.oracle_ptau(6)).g1_bytes  # 127 points tau^i G


def host(points, inverse=False):
    return K().g1_ntt(points, inverse=inverse, device=None)


# ------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("logm", LOGS)
def test_closed_forms_match_the_naive_sum(logm):
    n = 1 << logm
    a = N.tau_powers(n)
    assert N.forward_scalars(logm) == N.naive_scalars(a)
    L = N.lagrange_scalars(logm)
    assert L == N.naive_scalars(a, inverse=True)
    assert sum(L) % R == 1
    assert N.transform_scalars(a) == N.naive_scalars(a)
    assert N.transform_scalars(a, inverse=True) == L


@pytest.mark.parametrize("name", list(D.TAUS))
def test_closed_forms_at_degenerate_tau(name):
    """tau in the domain (1, -1, a 4th root of unity): L_j(tau) is 1 or 0, and one forward output is n;
    tau = 0: every L_j is 1 / n"""
    tau = D.TAUS[name]
    for logm in (0, 1, 2, 3, 5):
        a = N.tau_powers(1 << logm, tau)
        assert N.forward_scalars(logm, tau) == N.naive_scalars(a)
        L = N.lagrange_scalars(logm, tau)
        assert L == N.naive_scalars(a, inverse=True) and sum(L) % R == 1
        if pow(tau, 1 << logm, R) == 1:
            assert sorted(L) == [0] * ((1 << logm) - 1) + [1]


# ------------------------------------------------------------------ the host path
@pytest.mark.parametrize("logm", LOGS)
def test_forward_and_inverse_over_tau_powers(bases, logm):
    x = bases[:64 << logm]
    assert host(x) == N.expected_forward(logm)
    assert host(x, inverse=True) == N.expected_inverse(logm)


@pytest.mark.parametrize("logm", LOGS)
def test_round_trip(bases, logm):
    x = bases[:64 << logm]
    assert host(host(x), inverse=True) == x
    assert host(host(x, inverse=True)) == x


@pytest.mark.parametrize("logm", [1, 3, 6])
def test_general_scalars_and_identities(logm):
    n = 1 << logm
    a = D.random_scalars(n, 40 + logm)
    for i in range(0, n, 3):
        a[i] = 0  # the identity among the inputs
    x = N.points(a)
    assert x[:64] == bytes(64)
    assert host(x) == N.points(N.transform_scalars(a))
    assert host(x, inverse=True) == N.points(N.transform_scalars(a, inverse=True))
    assert host(bytes(64 * n)) == bytes(64 * n) == host(bytes(64 * n), inverse=True)


@pytest.mark.parametrize("name", list(D.TAUS))
@pytest.mark.parametrize("logm", [1, 2, 4, 6])
def test_degenerate_points(name, logm):
    """all points equal (every a + b is a doubling, every a - b the identity), P / -P alternating, a
    4-cycle, G followed by zero points"""
    n = 1 << logm
    x = D.srs_bytes(name, 6)[:64 * n]
    k = D.multipliers(name, n)
    assert host(x) == N.points(N.transform_scalars(k))
    assert host(x, inverse=True) == N.points(N.transform_scalars(k, inverse=True))
    assert host(x, inverse=True) == N.points(N.lagrange_scalars(logm, D.TAUS[name]))


def test_in_place():
    L = K().lib()
    x = N.points(D.random_scalars(8, 3))
    buf = ctypes.create_string_buffer(x, len(x))
    assert L.kgs_g1_ntt(None, buf, buf, 3, 0) == 0
    assert buf.raw == host(x)


# ------------------------------------------------------------------ argument errors
def test_argument_errors(bases):
    k = K()
    L = k.lib()
    pts = ctypes.create_string_buffer(bases[:128], 128)
    out = ctypes.create_string_buffer(128)

    def err(rc):
        return rc, L.kgs_last_error().decode()

    for logm in (-1, 25, 64):
        rc, msg = err(L.kgs_g1_ntt(None, pts, out, logm, 0))
        assert rc == KGS_E_ARG and "logm" in msg, logm
    for p, o in ((None, out), (pts, None)):
        rc, msg = err(L.kgs_g1_ntt(None, p, o, 1, 0))
        assert rc == KGS_E_ARG and "NULL" in msg
    rc, msg = err(L.kgs_g1_ntt_device(None, pts, out, 1, 0))  # the device entry needs a context
    assert rc == KGS_E_ARG and "ctx" in msg
    # the calls over a resident SRS need a context
    rc, msg = err(L.kgs_srs_lagrange(None, 1, out))
    assert rc == KGS_E_ARG and "ctx" in msg
    for fn in (L.kgs_commit_evals, L.kgs_commit_evals_device):
        rc, msg = err(fn(None, pts, 1, out))
        assert rc == KGS_E_ARG and "ctx" in msg
    for bad in (b"", bases[:100], bases[:192]):  # not a power of two of points
        with pytest.raises(ValueError):
            k.g1_ntt(bad, device=None)
