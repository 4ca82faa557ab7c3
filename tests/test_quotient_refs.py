"""The references of tests/quotient_cases.py pinned to the protocol restatement (no GPU): ref_quotient
between the transforms of ntt_cases.ref_py gives the oracle's own quotient polynomial, single (oracle/
protocol.py) and multi-argument (multi_oracle._numerator), and ref_divcheck accepts exactly the oracle's
honest round-3 state. So a GPU test that equals these references equals the protocol."""
import pytest

import multi_oracle as MO
import ntt_cases as N
import quotient_cases as Q
from oracle import poly as OP
from oracle.poly import Polynomial

R = Q.R
FWD = N.COSET | N.BITREV
INV = N.INVERSE | N.COSET | N.BITREV | N.NO_SCALE
NBITS = 3


def _coset_arg(case, lcs):
    ev = {k: (N.ref_py(v, lcs, FWD) if v is not None else None) for k, v in case["coef"].items()}
    return dict(ev, kind=case["kind"])


def _padded(coef, cs):
    assert not any(coef[cs:])
    return (list(coef) + [0] * cs)[:cs]


@pytest.mark.parametrize("build", Q.BUILD_NAMES)
def test_quotient_is_the_oracles_Q(build):
    case = Q.honest_case(build, NBITS, 9100 + Q.BUILD_NAMES.index(build))
    lcs = case["lcs"]
    assert lcs == (NBITS if build == "gp" else NBITS + 1)  # lcs = nbits only where deg N < 2n
    q = Q.ref_quotient(NBITS, lcs, [_coset_arg(case, lcs)], case["alpha"], case["gamma"])
    assert N.ref_py(q, lcs, INV) == _padded(case["Q_coef"], 1 << lcs)
    assert any(case["Q_coef"])


def test_unselected_grand_product_on_the_larger_coset_too():
    """the same polynomial from cs = 2n: the (nbits, nbits + 1) form of the build that also runs at cs = n"""
    case = Q.honest_case("gp", NBITS, 9102)
    q = Q.ref_quotient(NBITS, NBITS + 1, [_coset_arg(case, NBITS + 1)], case["alpha"], case["gamma"])
    assert N.ref_py(q, NBITS + 1, INV) == _padded(case["Q_coef"], 2 << NBITS)


def _restated_arg(case):
    a = MO._Arg()
    a.gs, a.lookup, a.sel = case["kind"] != Q.GRANDPRODUCT, case["kind"] == Q.LOOKUP, case["sel"]
    c = case["coef"]
    a.polS, a.polF, a.polT = Polynomial(list(c["S"])), Polynomial(list(c["F"])), Polynomial(list(c["T"]))
    a.selF = Polynomial(list(c["sel_f"])) if a.sel else None
    a.selT = Polynomial(list(c["sel_t"])) if a.sel else None
    return a


def test_multi_argument_quotient_is_the_restatement():
    """Three arguments (gs-sel, gp, lookup) that are honest under one gamma: sum_j delta^j N_j / Z_H of
    multi_oracle against ref_quotient with count = 3."""
    rnd = Q.seeded(9200)
    n, lcs = 1 << NBITS, NBITS + 1
    alpha, gamma, delta = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    cases = []
    for j, build in enumerate(("gs-sel", "gp", "lookup")):
        kind, sel = Q.BUILDS[build]
        F, T, sF, sT = Q.honest_inputs(build, NBITS, 9210 + j)
        H = {"F": [int.from_bytes(F[32 * i:32 * i + 32], "little") for i in range(n)],
             "T": [int.from_bytes(T[32 * i:32 * i + 32], "little") for i in range(n)],
             "sel_f": Q.unmont(sF) if sel else None, "sel_t": Q.unmont(sT) if sel else None}
        S, s_end = Q.honest_run(kind, n, H["F"], H["T"], H["sel_f"], H["sel_t"], gamma)
        assert s_end == S[0]  # the multisets are equal: the run closes
        H["S"] = S
        coef = {k: (list(Polynomial.from_evaluations(v).coef)[:n] if v is not None else None) for k, v in H.items()}
        cases.append({"kind": kind, "sel": sel, "coef": coef, "H": H})
    saved = OP.QUIRKS
    OP.QUIRKS = False
    try:
        total, dj = None, 1
        for c in cases:
            Nj = MO._numerator(_restated_arg(c), NBITS, alpha, gamma).mul_scalar(dj)
            total = Nj if total is None else total.add(Nj)
            dj = dj * delta % R
        total.div_zh(n)
    finally:
        OP.QUIRKS = saved
    q = Q.ref_quotient(NBITS, lcs, [_coset_arg(c, lcs) for c in cases], alpha, gamma, delta)
    assert N.ref_py(q, lcs, INV) == _padded(total.coef, 1 << lcs)
    # delta matters: the same arguments under another separator give another quotient
    assert Q.ref_quotient(NBITS, lcs, [_coset_arg(c, lcs) for c in cases], alpha, gamma, delta + 1) != q
    # and the natural-order state passes the divisibility reference argument by argument
    for c in cases:
        H = c["H"]
        assert Q.ref_divcheck(c["kind"], H["S"], H["F"], H["T"], H["sel_f"], H["sel_t"], alpha, gamma) == 0


@pytest.mark.parametrize("build", Q.BUILD_NAMES)
def test_divisibility_reference_on_honest_and_changed_inputs(build):
    case = Q.honest_case(build, NBITS, 9100 + Q.BUILD_NAMES.index(build))
    H, alpha, gamma = case["H"], case["alpha"], case["gamma"]

    n = 1 << NBITS

    def check(S=H["S"], F=H["F"], T=H["T"], lo=0, hi=n, **kw):
        sf, st = (H["sel_f"][lo:hi], H["sel_t"][lo:hi]) if case["sel"] else (None, None)
        return Q.ref_divcheck(case["kind"], S[lo:hi], F[lo:hi], T[lo:hi], sf, st, alpha, gamma, gbase=lo, **kw)

    assert check() == 0
    assert check(s_next=H["S"][0]) == 0
    for name, sel in (("S", None), ("F", H["sel_f"]), ("T", H["sel_t"])):
        # a row that its selector switches off (or a table row of multiplicity zero) is free to change
        live = [i for i in range(n) if sel is None or sel[i]]
        for i in (live[0], live[len(live) // 2], live[-1]):
            v = list(H[name])
            v[i] = (v[i] + 1) % R
            assert check(**{name: v}) == 1, (name, i)
    assert check(s_next=(H["S"][0] + 1) % R) == 1
    # a block of the run away from index 0 with its true continuation
    assert check(lo=2, hi=5, s_next=H["S"][5]) == 0
    assert check(lo=2, hi=5) == 1  # wraps to S[2] instead


def test_lincomb_reference():
    rnd = Q.seeded(9300)
    a, b = Q.rand_vec(rnd, 5), Q.rand_vec(rnd, 3)
    out = Q.ref_lincomb([a, b, a], [5, 2, 9], [2, R - 1, 0], 7, 4)
    assert out == [(2 * a[0] - b[0] + 7) % R, (2 * a[1] - b[1]) % R, 2 * a[2] % R, 2 * a[3] % R]
    assert Q.ref_lincomb([], [], [], R - 1, 2) == [R - 1, 0]
