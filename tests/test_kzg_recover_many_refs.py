"""The cases of kzg_recover_many_cases.py against the references of kzg_recover_cases.py, polynomial by polynomial; the
integer restatement of the blocked size-n side against C.steps; and what of kgs_kzg_recover_cosets_many can be
checked without a GPU: the exports and the refusal of a NULL context."""
import ctypes

import pytest

import common
import kzg_recover_cases as C
import kzg_recover_many_cases as M

R = C.R
KGS_E_ARG = -1
SHAPES = [(nbits, lbits) for nbits in range(7) for lbits in range(nbits + 1)]


def check_case(case):
    n, l, m = C.sizes(case.nbits, case.lbits)
    assert len(case.poly_of) == len(case.index) == len(case.rows)
    assert len(set(zip(case.poly_of, case.index))) == len(case.index)
    assert all(b < case.polys and i < m and len(r) == l for b, i, r in zip(case.poly_of, case.index, case.rows))
    assert sum(len(ix) for ix, _ in case.cells_of) == len(case.index)
    for b in range(case.polys):
        assert M.reference(case, b) == case.expect[b], (case.nbits, case.lbits, b)


@pytest.mark.parametrize("nbits,lbits", SHAPES)
def test_every_polynomial_of_a_case_is_pinned_to_the_references(nbits, lbits):
    for polys in (1, 3, 7):
        for shared in (False, True):
            for kind in M.LEN_KINDS if nbits <= 4 else M.LEN_KINDS[:1]:
                case = M.make_many(100 * nbits + 10 * lbits + polys, nbits, lbits, polys, shared, kind)
                assert case.polys == polys and case.status() == [M.OK] * polys
                if shared:
                    assert len({tuple(sorted(ix)) for ix, _ in case.cells_of}) == 1
                check_case(case)


def test_cells_are_shuffled_across_polynomials():
    case = M.make_many(5, 5, 2, 5)
    assert case.poly_of != sorted(case.poly_of)
    assert len({tuple(sorted(ix)) for ix, _ in case.cells_of}) > 1


@pytest.mark.parametrize("nbits,lbits", [s for s in SHAPES if s[0] - s[1] >= 2])
def test_the_statuses_of_a_mixed_case(nbits, lbits):
    case = M.make_statuses(900 + 10 * nbits + lbits, nbits, lbits)
    assert case.status() == [M.OK, M.NO_POLY, M.OK, M.TOO_FEW, M.TOO_FEW, M.OK]
    assert case.cells_of[4] == ([], []) and len(case.cells_of[3][0]) == M.need(case.length, lbits) - 1
    assert len(case.cells_of[2][0]) << lbits == case.length
    check_case(case)


@pytest.mark.parametrize("nbits,lbits", SHAPES)
def test_the_blocked_size_n_side_is_the_steps(nbits, lbits):
    for p, pattern in enumerate(C.PATTERNS):
        index, rows, length, coefs = C.make_case(4000 * nbits + 100 * lbits + p, nbits, lbits, pattern, "odd")
        assert M.blocked_nside(index, rows, nbits, lbits, length) == C.steps(index, rows, nbits, lbits, length) == (1, coefs)
        if len(index) << lbits > length:
            rows[p % len(rows)][0] = (rows[p % len(rows)][0] + 1) % R
            assert M.blocked_nside(index, rows, nbits, lbits, length)[0] == C.steps(index, rows, nbits, lbits, length)[0] == 0


def test_the_transforms_of_the_restatement_are_the_oracle_s():
    import random
    from oracle import poly as OP
    rng = random.Random(3)
    for logn in range(6):
        a = [rng.randrange(R) for _ in range(1 << logn)]
        f = OP.ntt(a, False)
        assert M.dif(a, logn) == [f[M.bitrev(x, logn)] for x in range(1 << logn)]
        assert M.dit(M.dif(a, logn), logn, inverse=True) == a


def test_the_library_exports_the_calls_and_refuses_a_null_context():
    """no GPU is opened: the refusal comes before anything touches a device"""
    L = common.load_pkg().lib()
    for name in ("kgs_kzg_recover_cosets_many", "kgs_kzg_recover_cosets_many_device", "kgs_bench_kzg_recover_cosets_many"):
        assert hasattr(L, name), name
    po = (ctypes.c_uint32 * 2)(0, 0)
    idx = (ctypes.c_uint64 * 2)(0, 1)
    ys = common.mont_bytes([1, 2, 3, 4])
    coef = ctypes.create_string_buffer(32 * 4)
    status = ctypes.create_string_buffer(b"\x07", 1)
    pp, pi = ctypes.cast(po, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)
    pys = ctypes.cast(ctypes.c_char_p(ys), ctypes.c_void_p)
    assert L.kgs_kzg_recover_cosets_many(None, 2, 1, 1, pp, pi, pys, 2, 4, 4, coef, None, status) == KGS_E_ARG
    assert "kgs_kzg_recover_cosets_many: NULL ctx" in L.kgs_last_error().decode()
    assert L.kgs_kzg_recover_cosets_many_device(None, 2, 1, 1, pp, pi, pys, 2, 4, 4, coef, None, status) == KGS_E_ARG
    assert "kgs_kzg_recover_cosets_many_device: NULL ctx" in L.kgs_last_error().decode()
    ms = (ctypes.c_double * 1)()
    assert L.kgs_bench_kzg_recover_cosets_many(None, 2, 1, 1, pp, pi, pys, 2, 4, 4, coef, 0, 1, ms) == KGS_E_ARG
    assert "kgs_bench_kzg_recover_cosets_many: NULL ctx" in L.kgs_last_error().decode()
    assert status.raw == b"\x07" and coef.raw == bytes(32 * 4)  # nothing written
