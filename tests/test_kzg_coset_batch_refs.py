"""kgs_kzg_verify_cosets_batch and kgs_coset_interp_fold on the host path (device=None, no GPU is touched) against
the integer references of kzg_coset_batch_cases.py: verdicts, rho, D and the folded points byte for byte, tampered
and structurally invalid openings named by valid_out, the bisection's check count, the argument errors."""
import ctypes
import random

import pytest

import common
import g1_ntt_cases as N
import kzg_coset_batch_cases as B
import kzg_coset_cases as C
import kzg_open_cases as Z

R = N.R
KGS_E_ARG = -1


def K():
    return common.load_pkg()


def coefs(nbits, count, seed=0):
    rnd = random.Random(7000 * nbits + count + seed)
    return [rnd.randrange(R) for _ in range(count)]


def run(batch, locate=True, seed=None, device=None):
    diag = {}
    got = K().kzg_verify_cosets_batch(batch.tau_l_g2(), batch.srs(), batch.nbits, batch.lbits, batch.commits(),
                                      batch.tuples(), device=device, locate=locate, seed=seed, diag=diag)
    return got, diag


def check_against_references(batch, got, diag, seed=None):
    """verdicts, rho, D and A || B of a run against the integer references"""
    rho = B.rho_of(seed if seed is not None else batch.seed())
    assert diag["rho"] == rho.to_bytes(32, "little")
    assert diag["interp"] == Z.mont(batch.interp(rho))
    assert diag["folded"] == batch.folded(rho)
    assert got == batch.verdicts()
    assert diag["pairing_checks"] <= B.check_bound(got.count(False), len(got))


def picks_for(nbits, lbits, npolys, count):
    n, l, m = C.sizes(nbits, lbits)
    rnd = random.Random(100 * nbits + 10 * lbits + count)
    if count == npolys * m:
        return [(ci, i) for ci in range(npolys) for i in range(m)]
    return [(rnd.randrange(npolys), rnd.randrange(m)) for _ in range(count)]


# ------------------------------------------------------------------ valid batches
@pytest.mark.parametrize("nbits", [3, 4, 5])
def test_valid_batches_match_the_references(nbits):
    for lbits in range(nbits + 1):
        n, l, m = C.sizes(nbits, lbits)
        npolys = 1 + (nbits + lbits) % 3
        polys = [coefs(nbits, n, 10 * lbits + p) for p in range(npolys)]
        for count in sorted({1, 2, 7, m * npolys}):
            batch = B.valid_batch(nbits, lbits, polys, picks_for(nbits, lbits, npolys, count))
            got, diag = run(batch)
            assert got == [True] * count, (lbits, count)
            assert diag["pairing_checks"] == 1 and diag["on_gpu"] == 0
            check_against_references(batch, got, diag)
            assert run(batch, locate=False)[0] is True


@pytest.mark.parametrize("nbits,lbits", [(3, 0), (3, 1), (3, 3), (5, 2)])
def test_count_one_is_the_single_check(nbits, lbits):
    k = K()
    n, l, m = C.sizes(nbits, lbits)
    c = coefs(nbits, n, 2)
    for i in sorted({0, m // 2, m - 1}):
        good = B.valid_batch(nbits, lbits, [c], [(0, i)])
        ci, idx, ys, pi = good.openings[0]
        bad_y = list(ys)
        bad_y[l // 2] = (bad_y[l // 2] + 1) % R
        for ys_, pi_ in ((ys, pi), (bad_y, pi), (ys, pi + 1)):
            one = B.Batch(nbits, lbits, [c], [(0, i, ys_, pi_)])
            (t,) = one.tuples()
            single = k.kzg_verify_coset(one.tau_l_g2(), one.srs(), one.commits()[0], nbits, lbits, i, t[2], t[3])
            got, diag = run(one)
            assert got == [single] and run(one, locate=False)[0] is single
            check_against_references(one, got, diag)


# ------------------------------------------------------------------ tampering
def base_batch(nbits=4, lbits=2, npolys=2):
    n, l, m = C.sizes(nbits, lbits)
    polys = [coefs(nbits, n, 40 + p) for p in range(npolys)]
    return B.valid_batch(nbits, lbits, polys, [(ci, i) for ci in range(npolys) for i in range(m)])


def with_opening(batch, k, **kw):
    ops = list(batch.openings)
    ci, i, ys, pi = ops[k]
    ops[k] = (kw.get("ci", ci), kw.get("i", i), kw.get("ys", ys), kw.get("pi", pi))
    return B.Batch(batch.nbits, batch.lbits, batch.polys, ops)


def test_tampered_openings_are_named():
    base = base_batch()
    ops = base.openings
    y1 = list(ops[3][2])
    y1[1] = (y1[1] + 1) % R
    cases = {
        "one value off by one": with_opening(base, 3, ys=y1),
        "the neighbouring coset's proof": with_opening(base, 5, pi=ops[6][3]),
        "the other polynomial's commitment": with_opening(base, 2, ci=1),
    }
    for name, batch in cases.items():
        got, diag = run(batch)
        assert got.count(False) == 1 and got == batch.verdicts(), name
        check_against_references(batch, got, diag)
        assert run(batch, locate=False)[0] is False, name


def test_errors_that_cancel_without_weights():
    """two openings of one coset with proofs pi + delta and pi - delta: sum pi_k and sum a_i pi_k are unchanged, so
    an unweighted sum of the equations would accept the pair"""
    base = base_batch()
    # openings 1 and 5 are coset 1 of polynomials 0 and 1
    assert base.openings[1][1] == base.openings[5][1] == 1
    delta = 12345
    batch = with_opening(with_opening(base, 1, pi=base.openings[1][3] + delta), 5, pi=base.openings[5][3] - delta)
    A1, B1 = batch.folded_scalars(1)
    A0, B0 = base.folded_scalars(1)
    assert (A1, B1) == (A0, B0)  # with every weight 1 the tampering does not show
    got, diag = run(batch)
    assert got == [k not in (1, 5) for k in range(len(got))]
    check_against_references(batch, got, diag)
    assert run(batch, locate=False)[0] is False


# ------------------------------------------------------------------ structural cases
def test_structural_cases():
    k = K()
    base = base_batch()
    n, l, m = C.sizes(base.nbits, base.lbits)
    big = list(base.openings[4][2])
    big[l - 1] = R  # r - 1 + 1
    for name, batch in {"a value of r": with_opening(base, 4, ys=big), "an index of m": with_opening(base, 0, i=m),
                        "commit_of = ncommits": with_opening(base, 7, ci=2)}.items():
        got, diag = run(batch)
        assert got.count(False) == 1 and got == batch.verdicts(), name
        assert diag["pairing_checks"] == 1, name  # marked before the aggregate check, which then passes
        check_against_references(batch, got, diag)
        assert run(batch, locate=False)[0] is False
    # a proof off the curve
    t = base.tuples()
    off = bytearray(t[2][3])
    off[5] ^= 1
    t[2] = t[2][:3] + (bytes(off),)
    diag = {}
    got = k.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), base.nbits, base.lbits, base.commits(), t, device=None,
                                    diag=diag)
    assert got == [j != 2 for j in range(len(t))] and diag["pairing_checks"] == 1
    # a commitment off the curve takes every opening of it along; an SRS point off the curve the whole batch
    cm = base.commits()
    cm[1] = bytes(off)
    got = k.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), base.nbits, base.lbits, cm, base.tuples(), device=None)
    assert got == [ci == 0 for ci, _, _, _ in base.openings]
    srs = bytearray(base.srs())
    srs[64 + 3] ^= 1
    assert k.kzg_verify_cosets_batch(base.tau_l_g2(), bytes(srs), base.nbits, base.lbits, base.commits(), base.tuples(),
                                     device=None) == [False] * len(t)
    # a value of the wrong length does not reach the library
    t = base.tuples()
    t[1] = (t[1][0], t[1][1], t[1][2][:-32], t[1][3])
    diag = {}
    got = k.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), base.nbits, base.lbits, base.commits(), t, device=None,
                                    diag=diag)
    assert got == [j != 1 for j in range(len(t))] and diag["indices"] == [0] + list(range(2, len(t)))


def test_identity_proofs_and_the_zero_polynomial():
    nbits, lbits = 4, 2
    n, l, m = C.sizes(nbits, lbits)
    low = coefs(nbits, l - 1, 3)  # deg < l: every quotient is zero, every proof the identity
    batch = B.valid_batch(nbits, lbits, [low, []], [(0, 0), (0, m - 1), (1, 1), (1, 2)])
    assert all(pi == 0 for _, _, _, pi in batch.openings) and batch.commits()[1] == bytes(64)
    got, diag = run(batch)
    assert got == [True] * 4
    check_against_references(batch, got, diag)


def test_count_zero_and_seed():
    k = K()
    base = base_batch()
    assert k.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), base.nbits, base.lbits, base.commits(), [],
                                     device=None) == []
    assert k.kzg_verify_cosets_batch(base.tau_l_g2(), base.srs(), base.nbits, base.lbits, [], [], device=None,
                                     locate=False) is True
    L = k.lib()
    assert L.kgs_kzg_verify_cosets_batch(None, 3, 1, None, 0, None, None, None, None, 0, None, base.tau_l_g2(), None,
                                         None, None) == 1
    _, derived = run(base)
    seeds = [bytes(32), bytes(range(32))]
    rhos = {derived["rho"]}
    for s in seeds:
        got, diag = run(base, seed=s)
        assert got == [True] * len(base.openings)
        check_against_references(base, got, diag, seed=s)
        rhos.add(diag["rho"])
    assert len(rhos) == 3
    with pytest.raises(ValueError):
        run(base, seed=bytes(31))


# ------------------------------------------------------------------ the bisection's cost
@pytest.mark.parametrize("bad", [(37,), (0, 63), (5, 6, 40)])
def test_check_count_is_within_the_bound(bad):
    """b invalid openings among 64: at most 1 + 2 b ceil(log2 64) = 1 + 12 b checks, wherever they lie (first and
    last, neighbours, one alone)"""
    nbits, lbits = 5, 0
    n, l, m = C.sizes(nbits, lbits)
    polys = [coefs(nbits, n, 60), coefs(nbits, n, 61)]
    batch = B.valid_batch(nbits, lbits, polys, [(ci, i) for ci in range(2) for i in range(m)])
    assert len(batch.openings) == 64
    for k in bad:
        batch = with_opening(batch, k, pi=batch.openings[k][3] + 1)
    got, diag = run(batch)
    assert got == [k not in bad for k in range(64)]
    assert 1 < diag["pairing_checks"] <= B.check_bound(len(bad), 64) == 1 + 12 * len(bad)
    _, agg = run(batch, locate=False)
    assert agg["pairing_checks"] == 1


# ------------------------------------------------------------------ kgs_coset_interp_fold, host path
@pytest.mark.parametrize("nbits,lbits", [(0, 0), (3, 0), (3, 3), (5, 2), (6, 5)])
def test_interp_fold_host(nbits, lbits):
    k = K()
    n, l, m = C.sizes(nbits, lbits)
    rnd = random.Random(nbits * 10 + lbits)
    count = 9
    index = [0, 1 % m, m - 1, m - 1] + [rnd.randrange(m) for _ in range(count - 4)]
    edge = [0, 1, R - 1]
    rows = [[edge[(r + j) % 3] if r < 2 else rnd.randrange(R) for j in range(l)] for r in range(count)]
    weights = [1, R - 1, 0] + [rnd.randrange(R) for _ in range(count - 3)]
    got = k.coset_interp_fold(nbits, lbits, index, Z.mont([y for row in rows for y in row]), Z.mont(weights),
                              device=None)
    assert got == Z.mont(B.interp_fold_reference(nbits, lbits, index, rows, weights))
    assert B.interp_fold_reference_grouped(nbits, lbits, index, rows, weights) == \
        B.interp_fold_reference(nbits, lbits, index, rows, weights)
    assert k.coset_interp_fold(nbits, lbits, [], b"", b"", device=None) == bytes(32 * l)


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    k = K()
    L = k.lib()
    base = base_batch(3, 1, 1)
    t = base.tuples()
    count = len(t)
    cm = ctypes.create_string_buffer(b"".join(base.commits()), 64)
    cof = (ctypes.c_uint32 * count)(*[x[0] for x in t])
    idx = (ctypes.c_uint64 * count)(*[x[1] for x in t])
    ys = ctypes.create_string_buffer(b"".join(x[2] for x in t), 64 * count)
    pf = ctypes.create_string_buffer(b"".join(x[3] for x in t), 64 * count)
    srs = ctypes.create_string_buffer(base.srs(), 128)
    t2 = base.tau_l_g2()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    good = [None, 3, 1, cm, 1, p(cof), p(idx), ys, pf, count, srs, t2, None, None, None]
    assert L.kgs_kzg_verify_cosets_batch(*good) == 1
    for pos in (3, 5, 6, 7, 8, 10, 11):
        args = list(good)
        args[pos] = None
        assert L.kgs_kzg_verify_cosets_batch(*args) == KGS_E_ARG, pos
    off = bytearray(t2)
    off[3] ^= 1
    assert L.kgs_kzg_verify_cosets_batch(*good[:11], bytes(off), None, None, None) == KGS_E_ARG
    for nbits, lbits in ((-1, 0), (29, 1), (3, 4), (3, -1)):
        args = list(good)
        args[1], args[2] = nbits, lbits
        assert L.kgs_kzg_verify_cosets_batch(*args) == KGS_E_ARG, (nbits, lbits)
    # the device twin needs a context and a seed
    assert L.kgs_kzg_verify_cosets_batch_device(*good) == KGS_E_ARG and "ctx" in L.kgs_last_error().decode()
    out = ctypes.create_string_buffer(64)
    w = ctypes.create_string_buffer(32 * count)
    assert L.kgs_coset_interp_fold(None, 3, 1, p(idx), ys, w, count, out) == 0
    for args in ((None, 3, 1, None, ys, w, count, out), (None, 3, 1, p(idx), None, w, count, out),
                 (None, 3, 1, p(idx), ys, None, count, out), (None, 3, 1, p(idx), ys, w, count, None),
                 (None, 3, 4, p(idx), ys, w, count, out), (None, 29, 1, p(idx), ys, w, count, out)):
        assert L.kgs_coset_interp_fold(*args) == KGS_E_ARG
    far = (ctypes.c_uint64 * count)(*([4] * count))  # m = 4
    one = ctypes.create_string_buffer(Z.mont([1] * count), 32 * count)
    assert L.kgs_coset_interp_fold(None, 3, 1, p(far), ys, one, count, out) == KGS_E_ARG
    assert L.kgs_coset_interp_fold_device(None, 3, 1, p(idx), ys, w, count, out) == KGS_E_ARG
