"""The reference of kgs_ntt_blocks (ntt_cases.ref_blocks) against the references it is made of, against itself
(inverse of forward), and against an integer model of what the block routes of ntt.hip rest on: the transforms of
size 2^s over the consecutive blocks of an array of 2^logtotal elements are the last s decimation-in-frequency
stages of that array (the first s decimation-in-time ones), read from stage tables of 2^s entries. And what of
the call can be checked without a GPU: the export and the refusal of a NULL context."""
import ctypes

import pytest

import common
import ntt_cases as N
from oracle import bn254 as bn

R = N.R
KGS_E_ARG = -1
VARIANTS = [0, N.INVERSE, N.INVERSE | N.NO_SCALE]


def blocks(data, s):
    size = 32 << s
    return [data[at:at + size] for at in range(0, len(data), size)]


@pytest.mark.parametrize("logm", [0, 1, 3, 7])
def test_one_block_is_the_whole_transform(logm):
    x = N.random_elements(10 + logm, 1 << logm)
    assert N.ref_blocks(x, logm, logm, 0) == N.ref(x, logm, N.BITREV)
    assert N.ref_blocks(x, logm, logm, N.INVERSE) == N.ref(x, logm, N.INVERSE | N.BITREV)
    assert N.ref_blocks(x, logm, logm, N.INVERSE | N.NO_SCALE) == N.ref(x, logm, N.INVERSE | N.BITREV | N.NO_SCALE)
    for build in (0, N.INFLIGHT):  # the pass build and a forward NO_SCALE change nothing
        assert N.ref_blocks(x, logm, logm, build | N.NO_SCALE) == N.ref(x, logm, N.BITREV)


def test_blocks_are_transformed_one_by_one():
    logtotal, s = 6, 2
    x = N.random_elements(20, 1 << logtotal)
    for flags in VARIANTS:
        got = blocks(N.ref_blocks(x, logtotal, s, flags), s)
        assert len(got) == 16
        for b, block in enumerate(blocks(x, s)):
            assert got[b] == N.ref(block, s, N.BITREV | flags), (flags, b)
    assert N.ref_blocks(x, logtotal, 0, 0) == N.ref_blocks(x, logtotal, 0, N.INVERSE) == x


def test_python_and_c_references_agree_block_by_block():
    """s = 10 lies below PY_MAX_LOGM, so ref_blocks takes the integer reference there; above it, oracle/c"""
    logtotal, s = 11, 10
    assert s <= N.PY_MAX_LOGM
    x = N.random_elements(21, 1 << logtotal)
    for flags in VARIANTS:
        f = N.BITREV | flags
        assert N.ref_blocks(x, logtotal, s, flags) == b"".join(N.ref_c(block, s, f) for block in blocks(x, s)), flags


@pytest.mark.parametrize("logtotal,s", [(5, 2), (9, 4), (11, 10), (14, 13)])
def test_inverse_of_forward(logtotal, s):
    x = N.random_elements(30 + logtotal, 1 << logtotal)
    y = N.ref_blocks(x, logtotal, s, 0)
    assert y != x
    assert N.ref_blocks(y, logtotal, s, N.INVERSE) == x
    scaled = N.ref_blocks(y, logtotal, s, N.INVERSE | N.NO_SCALE)
    assert scaled == common.mont_bytes([(v << s) % R for v in N.unmont(x)])


# ------------------------------------------------------------------ the identity the routes rest on
def stage_table(logM, inverse):
    """tw[h + t] = w_{2h}^t for t < h, h = 1, 2, .. 2^(logM - 1): 2^logM entries, entry 0 unused"""
    tw = [None] * (1 << logM)
    for lg in range(logM):
        h, w = 1 << lg, bn.FR_W[lg + 1]
        if inverse:
            w = pow(w, R - 2, R)
        for t in range(h):
            tw[h + t] = pow(w, t, R)
    return tw


def dif_stages(a, logm, first, last, tw):
    """stages first .. last - 1 of the decimation-in-frequency transform of 2^logm elements: stage k pairs
    i and i + h, h = 2^(logm - 1 - k), (x, y) -> (x + y, (x - y) tw[h + (i mod h)])"""
    a = list(a)
    for k in range(first, last):
        h = (1 << logm) >> (k + 1)
        for i in range(1 << logm):
            if not i & h:
                x, y = a[i], a[i + h]
                a[i], a[i + h] = (x + y) % R, (x - y) * tw[h + (i & (h - 1))] % R
    return a


def dit_stages(a, logm, first, last, tw):
    """stages first .. last - 1 of the decimation-in-time transform: stage k pairs i and i + h, h = 2^k,
    (x, y) -> (x + y w, x - y w), w = tw[h + (i mod h)]"""
    a = list(a)
    for k in range(first, last):
        h = 1 << k
        for i in range(1 << logm):
            if not i & h:
                x, y = a[i], a[i + h] * tw[h + (i & (h - 1))] % R
                a[i], a[i + h] = (x + y) % R, (x - y) % R
    return a


@pytest.mark.parametrize("logtotal,s", [(6, 3), (7, 1), (5, 5), (4, 0)])
def test_the_last_stages_of_the_whole_array_are_the_block_transforms(logtotal, s):
    """with tables of 2^s entries only: a stage's twiddles sit at tw[h .. 2h), whatever the array's size"""
    x = N.random_elements(40 + logtotal, 1 << logtotal)
    v = N.unmont(x)
    fwd = dif_stages(v, logtotal, logtotal - s, logtotal, stage_table(s, False))
    assert common.mont_bytes(fwd) == N.ref_blocks(x, logtotal, s, 0)
    inv = dit_stages(v, logtotal, 0, s, stage_table(s, True))
    assert common.mont_bytes(inv) == N.ref_blocks(x, logtotal, s, N.INVERSE | N.NO_SCALE)
    half = pow(2, R - 1 - s, R)  # 1 / 2^s
    assert common.mont_bytes([e * half % R for e in inv]) == N.ref_blocks(x, logtotal, s, N.INVERSE)
    if 0 < s < logtotal:  # and the stages before them do belong to a larger transform
        assert dif_stages(v, logtotal, logtotal - s - 1, logtotal, stage_table(s + 1, False)) != fwd


# ------------------------------------------------------------------ the library without a GPU
def test_the_library_exports_the_call_and_refuses_a_null_context():
    """no GPU is opened: the refusal comes before anything touches a device"""
    L = common.load_pkg().lib()
    assert hasattr(L, "kgs_ntt_blocks")
    x = N.random_elements(50, 16)
    out = ctypes.create_string_buffer(32 * 16)
    for flags in VARIANTS:
        assert L.kgs_ntt_blocks(None, ctypes.create_string_buffer(x, len(x)), out, 4, 2, flags) == KGS_E_ARG
        assert "NULL ctx" in L.kgs_last_error().decode()
    assert out.raw == bytes(32 * 16)  # nothing written
