"""References of kgs_quotient_ex, kgs_divcheck and kgs_lincomb (include/kgs.h), written from the header's
formulas with Python integers, and the seeded inputs of their tests. Nothing here calls the library;
tests/test_quotient_refs.py pins the references to the protocol restatement (oracle/protocol.py,
tests/multi_oracle.py).

Values are standard-form integers in [0, r); the tests convert with common.mont_bytes / unmont.
An argument is a dict {"kind": int, "S", "F", "T": lists, "sel_f", "sel_t": lists or None}.
"""
import os
import random
import re

import common
from oracle import bn254 as bn

R = bn.R
_HDR = open(os.path.join(common.ROOT, "include", "kgs.h")).read()


def _define(name):
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, _HDR, flags=re.M).group(1))


GRANDSUM, GRANDPRODUCT, LOOKUP = _define("KGS_GRANDSUM"), _define("KGS_GRANDPRODUCT"), _define("KGS_LOOKUP")
QUOT_FUSED = _define("KGS_QUOT_FUSED")
COSET_GEN = _define("KGS_NTT_COSET_GEN")
MAX_ARGS = _define("KGS_MAX_ARGS")

# the five kernel builds: name -> (kind, selected)
BUILDS = {"gs": (GRANDSUM, False), "gs-sel": (GRANDSUM, True), "gp": (GRANDPRODUCT, False),
          "gp-sel": (GRANDPRODUCT, True), "lookup": (LOOKUP, True)}
BUILD_NAMES = list(BUILDS)


def rev(k, bits):
    return int(format(k, "0%db" % bits)[::-1], 2) if bits else 0


def inv(x):
    return pow(x, R - 2, R)


# ------------------------------------------------------------------ the per-point numerator (poly_math.hpp)
def core(kind, s, sw, f, t, sf, st, alpha, gamma):
    """core: the numerator without its L1 term, before the outer factor alpha. sf is None: unselected."""
    fg, tg = (f + gamma) % R, (t + gamma) % R
    acc = 0
    if sf is not None:
        alpha_t = 0 if kind == LOOKUP else alpha
        acc = ((st - st * st) * alpha_t + (sf - sf * sf)) * alpha % R
    if kind != GRANDPRODUCT:
        q1 = (sw - s) * fg * tg
        q1 += (st * fg - sf * tg) if sf is not None else (f - t)
    else:
        dT, dF = tg, fg
        if sf is not None:
            dT, dF = st * (tg - 1) + 1, sf * (fg - 1) + 1
        q1 = sw * dT - s * dF
    return (acc + q1) % R


def l1op(kind, s):
    return (s - 1) % R if kind == GRANDPRODUCT else s


# ------------------------------------------------------------------ kgs_quotient_ex
_DOMAIN = {}


def coset_domain(nbits, lcs):
    """-> (zinv, nxm1): 1/(x_i^n - 1) and 1/(n (x_i - 1)) for natural i, x_i = g w_cs^i"""
    if (nbits, lcs) not in _DOMAIN:
        cs, n = 1 << lcs, 1 << nbits
        w = bn.FR_W[lcs]
        x, xs = COSET_GEN, []
        for _ in range(cs):
            xs.append(x)
            x = x * w % R
        _DOMAIN[nbits, lcs] = ([inv(pow(v, n, R) - 1) for v in xs], [inv(n * (v - 1)) for v in xs])
    return _DOMAIN[nbits, lcs]


def ref_quotient(nbits, lcs, args, alpha, gamma, delta=1):
    """q[p], p the bit-reversed coset index, as include/kgs.h states kgs_quotient_ex"""
    cs = 1 << lcs
    rot = cs >> nbits
    zinv, nxm1 = coset_domain(nbits, lcs)
    inv_cs = inv(cs)
    if len(args) == 1:
        delta = 1
    out = []
    for p in range(cs):
        i = rev(p, lcs)
        pw = rev((i + rot) % cs, lcs)
        c = l = 0
        dj = 1
        for a in args:
            sel = a["sel_f"] is not None
            c += dj * core(a["kind"], a["S"][p], a["S"][pw], a["F"][p], a["T"][p], a["sel_f"][p] if sel else None,
                           a["sel_t"][p] if sel else None, alpha, gamma)
            l += dj * l1op(a["kind"], a["S"][p])
            dj = dj * delta % R
        out.append(inv_cs * (alpha * zinv[i] % R * c + nxm1[i] * l) % R)
    return out


def ref_nxm1(nbits, lcs):
    """1/(cs n (x_i - 1)) at p = rev(i): what kgs_quotient_ex returns for alpha = 0, a grand-sum, S = 1"""
    cs = 1 << lcs
    nx = coset_domain(nbits, lcs)[1]
    ic = inv(cs)
    return [ic * nx[rev(p, lcs)] % R for p in range(cs)]


# ------------------------------------------------------------------ kgs_divcheck
def ref_divcheck(kind, S, f, t, sel_f, sel_t, alpha, gamma, s_next=None, gbase=0):
    n = len(S)
    for i in range(n):
        sw = S[i + 1] if i + 1 < n else (S[0] if s_next is None else s_next)
        v = alpha * core(kind, S[i], sw, f[i], t[i], sel_f[i] if sel_f is not None else None,
                         sel_t[i] if sel_f is not None else None, alpha, gamma)
        if gbase + i == 0:
            v += l1op(kind, S[i])
        if v % R:
            return 1
    return 0


def honest_run(kind, n, f, t, sel_f, sel_t, gamma, s0=None):
    """S[0 .. n] by the recurrence from S[0] (default: 0 for a sum, 1 for a product): core(i) == 0 for every
    i < n whatever f, t and binary selectors are. -> (S[:n], S[n])"""
    s = (1 if kind == GRANDPRODUCT else 0) if s0 is None else s0
    out = [s]
    for i in range(n):
        fg, tg = (f[i] + gamma) % R, (t[i] + gamma) % R
        sf, st = (sel_f[i], sel_t[i]) if sel_f is not None else (1, 1)
        if kind != GRANDPRODUCT:
            s = (s + sf * inv(fg) - st * inv(tg)) % R
        else:
            s = s * (sf * (fg - 1) + 1) % R * inv(st * (tg - 1) + 1) % R
        out.append(s)
    return out[:n], out[n]


# ------------------------------------------------------------------ kgs_lincomb
def ref_lincomb(srcs, lens, coefs, c0, out_len):
    out = [0] * out_len
    for src, ln, c in zip(srcs, lens, coefs):
        for i in range(min(ln, out_len)):
            out[i] = (out[i] + c * src[i]) % R
    out[0] = (out[0] + c0) % R
    return out


# ------------------------------------------------------------------ seeded inputs
def rand_vec(rnd, count):
    return [rnd.randrange(R) for _ in range(count)]


def quot_arg(rnd, build, cs, pattern="random"):
    """One argument of `build` over cs points. pattern: "random", a constant ("r-1", "0", "1"), "sel-random"
    (random non-binary selectors) or "sel-r-1" (selectors all r - 1), the last two with S, F, T random."""
    kind, sel = BUILDS[build]
    const = {"r-1": R - 1, "0": 0, "1": 1}.get(pattern)
    if const is not None:
        vec = lambda: [const] * cs  # noqa: E731
        sv = vec
    else:
        vec = lambda: rand_vec(rnd, cs)  # noqa: E731
        sv = {"random": lambda: [rnd.randrange(2) for _ in range(cs)], "sel-random": vec,
              "sel-r-1": lambda: [R - 1] * cs}[pattern]
        if pattern == "random" and kind == LOOKUP:
            sv = lambda: [rnd.randrange(4) for _ in range(cs)]  # noqa: E731  (multiplicities)
    a = {"kind": kind, "S": vec(), "F": vec(), "T": vec(), "sel_f": None, "sel_t": None}
    if sel:
        a["sel_f"], a["sel_t"] = sv(), sv()
    return a


# ------------------------------------------------------------------ honest proofs of the oracle
_ORACLE_KIND = {GRANDSUM: "grandsum", GRANDPRODUCT: "grandproduct", LOOKUP: "lookup"}
_HONEST = {}


def honest_inputs(build, nbits, seed):
    """-> (F std bytes, T std bytes, selF mont bytes | None, selT mont bytes | None), one column"""
    kind, sel = BUILDS[build]
    if kind == LOOKUP:
        Fs, Ts, sF, sT = common.make_lookup_inputs(seed, nbits, 1, 1)
    else:
        Fs, Ts, sF, sT = common.make_inputs(seed, nbits, 1, sel)
    return Fs[0], Ts[0], sF, sT


def honest_case(build, nbits, seed):
    """One honest proof of the oracle (oracle.protocol.prove, exact-math mode) with its round-3 state: the
    coefficient vectors of S, F, T (+ selectors), their values on H, alpha, gamma and the quotient's
    coefficients. Computed once per case; callers do not modify it."""
    key = (build, nbits, seed)
    if key not in _HONEST:
        from oracle import poly as OP
        from oracle import protocol as P
        import multi_cases as MC
        kind, sel = BUILDS[build]
        F, T, sF, sT = honest_inputs(build, nbits, seed)
        tr = {}
        P.prove(_ORACLE_KIND[kind], MC.srs(), P.EvalBuffer(F), P.EvalBuffer(T), P.EvalBuffer(sF) if sel else None,
                P.EvalBuffer(sT) if sel else None, trace=tr, quirks=False)
        n = 1 << nbits
        H = {"F": [int.from_bytes(F[32 * i:32 * i + 32], "little") for i in range(n)],
             "T": [int.from_bytes(T[32 * i:32 * i + 32], "little") for i in range(n)],
             "sel_f": unmont(sF) if sel else None, "sel_t": unmont(sT) if sel else None}
        coef = {k: (list(OP.Polynomial.from_evaluations(v).coef)[:n] if v is not None else None) for k, v in H.items()}
        coef["S"] = (list(tr["S_coef"]) + [0] * n)[:n]
        assert not any(tr["S_coef"][n:])
        H["S"] = OP.ntt(coef["S"], False)
        _HONEST[key] = {"kind": kind, "sel": sel, "nbits": nbits, "lcs": nbits if build == "gp" else nbits + 1,
                        "coef": coef, "H": H, "alpha": tr["challenges"]["alpha"], "gamma": tr["challenges"]["gamma"],
                        "Q_coef": list(tr["Q_coef"])}
    return _HONEST[key]


def unmont(data):
    return [bn.fr_from_bytes(data[32 * i:32 * i + 32]) for i in range(len(data) // 32)]


def seeded(seed):
    return random.Random(seed)
