"""Variable-base MSM on the host path (kgs_msm_points with ctx == NULL, msm_points(device=None)): the
closed form over the bases tau^i G, the degenerate base families, scalars at and above r, the identity,
the argument errors of the C-ABI and of the Python wrapper. No GPU is touched."""
import ctypes

import pytest

import common
import degenerate_cases as D
import msm_points_cases as M
from oracle import ptau as opt

R = M.R
KGS_E_ARG = -1
POWER = 6  # 127 points


def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def bases():
    return opt.PTau(common.oracle_ptau(POWER)).g1_bytes


def host(points, scalars, window_c=0):
    return K().msm_points(points, M.scalar_bytes(scalars), device=None, window_c=window_c)


@pytest.mark.parametrize("n", [0, 1, 2, 17, 64])
def test_closed_form(bases, n):
    s = D.random_scalars(n, 900 + n)
    assert host(bases[:64 * n], s) == M.closed_form(s)


@pytest.mark.parametrize("name", list(D.TAUS))
def test_degenerate_bases(name):
    """tau in {1, r-1, a 4th root of unity, 0}: all points equal, P / -P alternating, a 4-cycle, G then
    zero points; random scalars and all scalars equal (tau = r-1: the sum cancels to the identity)"""
    n = 16
    pts = D.srs_bytes(name, 4)[:64 * n]
    s = D.random_scalars(n, 77)
    assert host(pts, s) == D.expected(name, s)
    eq = [s[0]] * n
    assert host(pts, eq) == D.expected(name, eq)
    if name == "alt":
        assert D.expected(name, eq) == bytes(64)


def test_scalars_at_and_above_r(bases):
    """any 256-bit integer is taken mod r"""
    s = [0, 1, R - 1, R, R + 1, (1 << 256) - 1]
    assert host(bases[:64 * len(s)], s) == M.closed_form([v % R for v in s])
    for v in s:
        assert host(bases[64:128], [v]) == M.closed_form([0, v % R]), hex(v)


def test_identity_in_identity_out(bases):
    s = D.random_scalars(5, 3)
    assert host(bytes(64 * 5), s) == bytes(64)
    assert host(bases[:64 * 5], [0] * 5) == bytes(64)
    assert host(bases[:64 * 5], [R] * 5) == bytes(64)
    # zero points among real bases contribute nothing
    mixed = bases[:64] + bytes(64) + bases[128:192] + bytes(128)
    assert host(mixed, s) == M.closed_form([s[0], 0, s[2]])


def test_window_is_range_checked_only(bases):
    s = D.random_scalars(17, 5)
    want = M.closed_form(s)
    for c in (7, 16):
        assert host(bases[:64 * 17], s, window_c=c) == want


def raw(ctx, points, scalars, n, window_c, device=False):
    L = K().lib()
    out = ctypes.create_string_buffer(64)
    fn = L.kgs_msm_points_device if device else L.kgs_msm_points
    rc = fn(ctx, points, scalars, n, window_c, out)
    return rc, L.kgs_last_error().decode()


def test_argument_errors(bases):
    pts = ctypes.create_string_buffer(bases[:128], 128)
    sc = ctypes.create_string_buffer(M.scalar_bytes([1, 2]), 64)
    for c in (-1, 1, 6, 17, 20):
        rc, msg = raw(None, pts, sc, 2, c)
        assert rc == KGS_E_ARG and "window_c" in msg, c
    for p, s in ((None, sc), (pts, None)):
        rc, msg = raw(None, p, s, 2, 0)
        assert rc == KGS_E_ARG and "NULL" in msg
    rc, msg = raw(None, pts, sc, (1 << 26) + 1, 0)  # refused before a byte is read
    assert rc == KGS_E_ARG and "2^26" in msg
    rc, msg = raw(None, pts, sc, 2, 0, device=True)  # the device entry needs a context
    assert rc == KGS_E_ARG and "ctx" in msg
    assert raw(None, None, None, 0, 0)[0] == 0  # n == 0 needs no buffers
    with pytest.raises(K().KgsError) as e:
        K().msm_points(bases[:128], M.scalar_bytes([1, 2]), device=None, window_c=6)
    assert e.value.code == KGS_E_ARG


def test_python_length_mismatches(bases):
    k = K()
    for pts, sc in ((bases[:128], bytes(32)), (bases[:64], bytes(64)), (bases[:100], bytes(32)),
                    (bases[:64], bytes(31)), (b"", bytes(32))):
        with pytest.raises(ValueError):
            k.msm_points(pts, sc, device=None)
