"""The two integer references of kzg_recover_cases.py against each other and against the polynomial every case is
built from, and what of kgs_kzg_recover_cosets can be checked without a GPU: the export and the refusal of a NULL
context."""
import ctypes

import pytest

import common
import kzg_recover_cases as C

R = C.R
KGS_E_ARG = -1
SHAPES = [(nbits, lbits) for nbits in range(7) for lbits in range(nbits + 1)]


@pytest.mark.parametrize("nbits,lbits", SHAPES)
def test_references_agree_with_the_construction(nbits, lbits):
    for p, pattern in enumerate(C.PATTERNS):
        for kind in C.LEN_KINDS if nbits <= 4 else C.LEN_KINDS[:1]:
            index, rows, length, coefs = C.make_case(1000 * nbits + 100 * lbits + p, nbits, lbits, pattern, kind)
            assert len(set(index)) == len(index) and len(index) << lbits >= length >= 1
            assert C.lagrange(index, rows, nbits, lbits, length) == (1, coefs), (pattern, kind)
            assert C.steps(index, rows, nbits, lbits, length) == (1, coefs), (pattern, kind)


def tampered(rows, seed):
    k, j = seed % len(rows), (seed // 7) % len(rows[0])
    out = [list(r) for r in rows]
    out[k][j] = (out[k][j] + 1 + seed) % R
    return out


@pytest.mark.parametrize("nbits,lbits", [s for s in SHAPES if s[0] >= 1])
def test_a_tampered_value_with_values_to_spare_is_inconsistent(nbits, lbits):
    for p, pattern in enumerate(("none", "run", "random", "shuffled")):
        index, rows, length, coefs = C.make_case(2000 * nbits + 100 * lbits + p, nbits, lbits, pattern, "odd")
        if len(index) << lbits == length:  # nothing to spare (l = 1 and an odd capacity)
            continue
        bad = tampered(rows, 31 * nbits + p)
        assert C.lagrange(index, bad, nbits, lbits, length)[0] == 0, pattern
        assert C.steps(index, bad, nbits, lbits, length)[0] == 0, pattern


@pytest.mark.parametrize("nbits,lbits", SHAPES)
def test_a_tampered_value_at_full_length_gives_another_polynomial(nbits, lbits):
    for p, pattern in enumerate(("none", "minimum", "random")):
        index, rows, length, coefs = C.make_case(3000 * nbits + 100 * lbits + p, nbits, lbits, pattern, "max")
        assert len(index) << lbits == length
        bad = tampered(rows, 17 * nbits + p)
        verdict, lag = C.lagrange(index, bad, nbits, lbits, length)
        assert verdict == 1 and lag != coefs
        assert C.steps(index, bad, nbits, lbits, length) == (1, lag), pattern
        assert C.rows_of(C.evals(lag, nbits), nbits, lbits, index) == bad


def test_the_library_exports_the_call_and_refuses_a_null_context():
    """no GPU is opened: the refusal comes before anything touches a device"""
    L = common.load_pkg().lib()
    for name in ("kgs_kzg_recover_cosets", "kgs_kzg_recover_cosets_device"):
        assert hasattr(L, name), name
    idx = (ctypes.c_uint64 * 2)(0, 1)
    ys = common.mont_bytes([1, 2, 3, 4])
    coef = ctypes.create_string_buffer(32 * 4)
    p = ctypes.cast(idx, ctypes.c_void_p)
    assert L.kgs_kzg_recover_cosets(None, 2, 1, p, ys, 2, 4, coef, None) == KGS_E_ARG
    assert "ctx" in L.kgs_last_error().decode()
    assert L.kgs_kzg_recover_cosets_device(None, 2, 1, p, ys, 2, 4, coef, None) == KGS_E_ARG
    assert "ctx" in L.kgs_last_error().decode()
