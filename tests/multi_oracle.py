"""Pure-Python restatement of the multi-argument protocol (include/kgs.h kgs_prove_multi),
built from the CPU oracle's pieces (oracle.poly, oracle.protocol) in exact-math mode (OP.QUIRKS = False).

m arguments over one domain share beta, gamma, alpha, xi, v, u; for m > 1 a separator delta, drawn after
alpha, weights argument j's quotient numerator N_j and linearisation r_j by delta^j. Per argument N_j and
r_j are exactly what oracle.protocol._prove computes for that argument alone (the same operations in
the same order). An argument is a dict
    {"kind": "grandsum" | "grandproduct" | "lookup", "Fs": [std bytes], "Ts": [std bytes],
     "selF": mont bytes | None, "selT": mont bytes | None}
and a shape is (kind, npols, selected). Proofs are (commitments, evaluations): two lists of bytes in the
order of kgs.h.

unchecked=True is for the tests only (a cheating prover): S_j is built without the wrap-around check and
the division by Z_H discards the remainder.
"""
from oracle import bn254 as bn
from oracle import poly as OP
from oracle import protocol as P
from oracle.poly import Polynomial, batch_inverse

R = bn.R
KINDS = {"grandsum": 0, "grandproduct": 1, "lookup": 2}


def shape_of(arg):
    return (arg["kind"], len(arg["Fs"]), arg.get("selF") is not None)


def proof_counts(shapes):
    """(commitments, evaluations) by the layout rule."""
    nc = sum(2 * k + (2 if s else 0) for _, k, s in shapes) + len(shapes) + 3
    ne = sum((1 if kind == "grandproduct" else 2) * k + (2 if s else 0) for kind, k, s in shapes) + len(shapes)
    return nc, ne


def _vals_std(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") % R for i in range(len(b) // 32)]


def _vals_mont(b):
    return [bn.fr_from_bytes(b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]


def _unchecked_S(gs, evF, evT, selF, selT, gamma):
    """P._grandsum_S / P._grandproduct_Z without the final check."""
    n = len(evF)
    num, den = [0] * n, [0] * n
    for i in range(n):
        f, t = (evF[i] + gamma) % R, (evT[i] + gamma) % R
        j = (i + 1) % n
        if gs:
            num[j], den[j] = (t * selF[i] - f * selT[i]) % R, f * t % R
        else:
            num[j], den[j] = (selF[i] * (f - 1) + 1) % R, (selT[i] * (t - 1) + 1) % R
    den = batch_inverse(den)
    last = 0 if gs else 1
    for i in range(n):
        j = (i + 1) % n
        last = (num[j] * den[j] + last) % R if gs else num[j] * den[j] * last % R
        num[j] = last
    return Polynomial.from_evaluations(num)


class _Arg:
    pass


def _numerator(a, nbits, alpha, gamma):
    """N_j: oracle.protocol._prove round 3 (prover.js:233-286) up to, not including, divZh."""
    n = 1 << nbits
    polS, polF, polT, selF, selT = a.polS, a.polF, a.polT, a.selF, a.selT
    polQ = Polynomial.zero(n)
    if a.sel:
        if not a.lookup:
            b1 = selT.clone()
            b1.multiply(selT.clone())
            polQ.add(selT.clone().sub(b1))
        polQ.mul_scalar(alpha)
        b1 = selF.clone()
        b1.multiply(selF.clone())
        polQ.add(selF.clone().sub(b1)).mul_scalar(alpha)
    polQ1 = polS.clone()
    polQ1.shift_omega()
    polFG = polF.clone().add_scalar(gamma)
    polTG = polT.clone().add_scalar(gamma)
    if a.gs:
        polQ1.sub(polS)
        polQ1.multiply(polFG)
        polQ1.multiply(polTG)
        if a.sel:
            sfg = selF.clone()
            sfg.multiply(polTG)
            stg = selT.clone()
            stg.multiply(polFG)
            polQ1.add(stg)
            polQ1.sub(sfg)
        else:
            polQ1.add(polF)
            polQ1.sub(polT)
        polQ.add(polQ1).mul_scalar(alpha)
        polQ2 = polS.clone()
        polQ2.multiply(Polynomial.lagrange1(nbits))
        polQ.add(polQ2)
    else:
        polQ2 = polS.clone()
        if a.sel:
            polTG.sub_scalar(1)
            polTG.multiply(selT.clone())
            polTG.add_scalar(1)
            polQ1.multiply(polTG)
            polFG.sub_scalar(1)
            polFG.multiply(selF.clone())
            polFG.add_scalar(1)
            polQ2.multiply(polFG)
        else:
            polQ1.multiply(polTG)
            polQ2.multiply(polFG)
        polQ1.sub(polQ2)
        polQ.add(polQ1).mul_scalar(alpha)
        polQ3 = polS.clone()
        polQ3.sub_scalar(1)
        polQ3.multiply(Polynomial.lagrange1(nbits))
        polQ.add(polQ3)
    return polQ


def _linearisation(a, nbits, alpha, gamma, xi, zh, l1):
    """r_j without its Q term: oracle.protocol._prove round 5 (prover.js:320-413)."""
    n = 1 << nbits
    polS, polF, polT = a.polS, a.polF, a.polT
    polR = Polynomial.zero(n)
    if a.sel:
        sT, sF = a.sTx, a.sFx
        polR.add_scalar(0 if a.lookup else (sT - sT * sT) % R).mul_scalar(alpha)
        polR.add_scalar((sF - sF * sF) % R).mul_scalar(alpha)
    fxi = polF.evaluate(xi)
    if a.gs:
        polR1 = polS.clone().mul_scalar(R - 1).add_scalar(a.sxiw)
        txi = polT.evaluate(xi)
        fg, tg = (fxi + gamma) % R, (txi + gamma) % R
        polR1.mul_scalar(fg)
        polR1.mul_scalar(tg)
        if a.sel:
            polR1.add_scalar(a.sTx * fg % R)
            polR1.sub_scalar(a.sFx * tg % R)
        else:
            polR1.add_scalar(fxi)
            polR1.sub_scalar(txi)
        polR.add(polR1).mul_scalar(alpha)
        polR.add(polS.clone().mul_scalar(l1))
    else:
        polR1 = Polynomial.zero(n)
        fg = (fxi + gamma) % R
        tgp = polT.clone().add_scalar(gamma)
        if a.sel:
            fg = (fg - 1) % R
            tgp.sub_scalar(1)
            sfg = (a.sFx * fg + 1) % R
            stg = tgp.mul_scalar(a.sTx).add_scalar(1)
            stg.mul_scalar(a.sxiw)
            polR1.add(stg)
            polR1.sub(polS.clone().mul_scalar(sfg))
        else:
            tgp.mul_scalar(a.sxiw)
            polR1.add(tgp)
            polR1.sub(polS.clone().mul_scalar(fg))
        polR.add(polR1).mul_scalar(alpha)
        polR.add(polS.clone().sub_scalar(1).mul_scalar(l1))
    return polR


def prove_multi(srs, args, unchecked=False):
    saved = OP.QUIRKS
    OP.QUIRKS = False
    try:
        return _prove_multi(srs, args, unchecked)
    finally:
        OP.QUIRKS = saved


def _prove_multi(srs, args, unchecked):
    m = len(args)
    assert 1 <= m <= 16
    n = len(args[0]["Fs"][0]) // 32
    nbits = n.bit_length() - 1
    assert n == 1 << nbits and srs.power >= nbits

    def C(poly):
        return poly.multi_exponentiation(srs)

    tr = P.Transcript()
    A = []
    com1 = []
    # ---------------- round 1
    for arg in args:
        a = _Arg()
        a.kind = arg["kind"]
        a.gs = a.kind != "grandproduct"
        a.lookup = a.kind == "lookup"
        a.k = len(arg["Fs"])
        a.sel = arg.get("selF") is not None
        assert a.k >= 1 and len(arg["Ts"]) == a.k and (a.sel or not a.lookup)
        a.evFs = [_vals_std(b) for b in arg["Fs"]]
        a.evTs = [_vals_std(b) for b in arg["Ts"]]
        assert all(len(x) == n for x in a.evFs + a.evTs)
        a.polFs = [Polynomial.from_evaluations(x) for x in a.evFs]
        a.polTs = [Polynomial.from_evaluations(x) for x in a.evTs]
        for i in range(a.k):
            com1 += [C(a.polFs[i]), C(a.polTs[i])]
        a.selFv = _vals_mont(arg["selF"]) if a.sel else [1] * n
        a.selTv = _vals_mont(arg["selT"]) if a.sel else [1] * n
        a.selF = a.selT = None
        if a.sel:
            a.selF = Polynomial.from_evaluations(a.selFv)
            a.selT = Polynomial.from_evaluations(a.selTv)
            com1 += [C(a.selF), C(a.selT)]
        A.append(a)
    # ---------------- round 2
    for p in com1:
        tr.add_pol_commitment(p)
    beta = 0
    if any(a.k > 1 for a in A):
        beta = tr.get_challenge()
        tr.add_field_element(beta)
    gamma = tr.get_challenge()
    comS = []
    for j, a in enumerate(A):
        if a.k > 1:
            a.polF = Polynomial.zero(n)
            a.polT = Polynomial.zero(n)
            for i in range(a.k - 1, -1, -1):
                a.polF.mul_scalar(beta).add(a.polFs[i])
                a.polT.mul_scalar(beta).add(a.polTs[i])
            evF = OP.Evaluations.from_polynomial(a.polF, 1).vals
            evT = OP.Evaluations.from_polynomial(a.polT, 1).vals
        else:
            a.polF, a.polT = a.polFs[0], a.polTs[0]
            evF, evT = a.evFs[0], a.evTs[0]
        try:
            a.polS = (P._grandsum_S if a.gs else P._grandproduct_Z)(evF, evT, a.selFv, a.selTv, gamma)
        except ValueError as e:
            if not unchecked:
                raise ValueError(f"argument {j}: {e}") from None
            a.polS = _unchecked_S(a.gs, evF, evT, a.selFv, a.selTv, gamma)
        comS.append(C(a.polS))
    # ---------------- round 3
    tr.add_field_element(gamma)
    for p in comS:
        tr.add_pol_commitment(p)
    alpha = tr.get_challenge()
    delta = 1
    if m > 1:
        tr.add_field_element(alpha)
        delta = tr.get_challenge()
    polQ = None
    dj = 1
    for j, a in enumerate(A):
        N = _numerator(a, nbits, alpha, gamma)
        if not unchecked:
            try:
                N.clone().div_zh(n)
            except ValueError as e:
                raise ValueError(f"argument {j}: {e}") from None
        N.mul_scalar(dj)
        polQ = N if polQ is None else polQ.add(N)
        dj = dj * delta % R
    if unchecked:
        if polQ.degree() < n:
            polQ = Polynomial.zero(n)
        else:
            polQ.div_by_vanishing(n, 1)
    else:
        polQ.div_zh(n)
    comQ = C(polQ)
    # ---------------- round 4
    tr.add_field_element(delta if m > 1 else alpha)
    tr.add_pol_commitment(comQ)
    xi = tr.get_challenge()
    w = bn.FR_W[nbits]
    evals = []
    opened = []  # (polynomial, value at xi) in the opening order
    for a in A:
        a.fx = [p.evaluate(xi) for p in a.polFs]
        a.tx = [p.evaluate(xi) for p in a.polTs] if a.gs else []
        for i in range(a.k):
            evals.append(a.fx[i])
            if a.gs:
                evals.append(a.tx[i])
        opened += list(zip(a.polFs, a.fx)) + list(zip(a.polTs, a.tx))
        if a.sel:
            a.sFx, a.sTx = a.selF.evaluate(xi), a.selT.evaluate(xi)
            evals += [a.sFx, a.sTx]
            opened += [(a.selF, a.sFx), (a.selT, a.sTx)]
    for a in A:
        a.sxiw = a.polS.evaluate(xi * w % R)
        evals.append(a.sxiw)
    # ---------------- round 5
    tr.add_field_element(xi)
    for e in evals:
        tr.add_field_element(e)
    v = tr.get_challenge()
    zh = P.zh_eval(xi, nbits)
    l1 = P.l1_eval(xi, zh, nbits)
    polR = Polynomial.zero(n)
    dj = 1
    for a in A:
        polR.add(_linearisation(a, nbits, alpha, gamma, xi, zh, l1).mul_scalar(dj))
        dj = dj * delta % R
    polR.sub(polQ.clone().mul_scalar(zh))
    polW = Polynomial.zero(n)
    for pol, val in reversed(opened):
        polW.mul_scalar(v).add(pol.clone().sub_scalar(val))
    polW.mul_scalar(v).add(polR)
    polWw = Polynomial.zero(n)
    for a in reversed(A):
        polWw.mul_scalar(v).add(a.polS.clone().sub_scalar(a.sxiw))
    if unchecked:
        polW = _div_discard(polW, xi)
        polWw = _div_discard(polWw, xi * w % R)
    else:
        polW.div_by_x_sub_value(xi)
        polWw.div_by_x_sub_value(xi * w % R)
    coms = com1 + comS + [comQ, C(polW), C(polWw)]
    return [bn.g1_to_lem(p) for p in coms], [bn.fr_to_bytes(x) for x in evals]


def _div_discard(poly, value):
    """Quotient of poly by (X - value), remainder discarded (the cheating prover's openings)."""
    L = poly.length()
    q = [0] * L
    q[L - 2] = poly.coef[L - 1]
    for i in range(L - 3, -1, -1):
        q[i] = (poly.coef[i + 1] + value * q[i + 1]) % R
    return Polynomial(q)


def verify_multi(shapes, proof, nbits, tau):
    """The verifier of kgs.h with the trapdoor test tau * A == B in place of the pairing check."""
    coms, evs = proof
    nc, ne = proof_counts(shapes)
    if len(coms) != nc or len(evs) != ne:
        return False
    m = len(shapes)
    com = [bn.g1_from_lem(b) for b in coms]
    if not all(bn.g1_is_on_curve(p) for p in com):
        return False
    if any(int.from_bytes(b, "little") >= R for b in evs):
        return False
    ev = [bn.fr_from_bytes(b) for b in evs]
    ncom1 = nc - m - 3
    comS, Q, Wxi, Wxiw = com[ncom1:ncom1 + m], com[nc - 3], com[nc - 2], com[nc - 1]
    tr = P.Transcript()
    for p in com[:ncom1]:
        tr.add_pol_commitment(p)
    beta = 0
    if any(k > 1 for _, k, _ in shapes):
        beta = tr.get_challenge()
        tr.add_field_element(beta)
    gamma = tr.get_challenge()
    tr.add_field_element(gamma)
    for p in comS:
        tr.add_pol_commitment(p)
    alpha = tr.get_challenge()
    tr.add_field_element(alpha)
    delta = 1
    if m > 1:
        delta = tr.get_challenge()
        tr.add_field_element(delta)
    tr.add_pol_commitment(Q)
    xi = tr.get_challenge()
    tr.add_field_element(xi)
    for e in ev:
        tr.add_field_element(e)
    v = tr.get_challenge()
    tr.add_field_element(v)
    tr.add_pol_commitment(Wxi)
    tr.add_pol_commitment(Wxiw)
    u = tr.get_challenge()
    zh = P.zh_eval(xi, nbits)
    l1 = P.l1_eval(xi, zh, nbits)
    w = bn.FR_W[nbits]
    M, Ad = bn.g1_mul, bn.g1_add
    B = Ad(M(Wxi, xi), M(Wxiw, u * xi % R * w % R))
    B = Ad(B, bn.g1_neg(M(Q, zh)))
    E = 0
    c0 = e0 = 0
    dj = vj = 1
    pw = v
    for j, (kind, k, sel) in enumerate(shapes):
        gs, lookup = kind != "grandproduct", kind == "lookup"
        per = 2 if gs else 1
        F = [com[c0 + 2 * i] for i in range(k)]
        T = [com[c0 + 2 * i + 1] for i in range(k)]
        fx = [ev[e0 + per * i] for i in range(k)]
        tx = [ev[e0 + per * i + 1] for i in range(k)] if gs else []
        sxiw = ev[ne - m + j]
        r0 = 0
        sF = sT = 0
        if sel:
            selF, selT = com[c0 + 2 * k], com[c0 + 2 * k + 1]
            sF, sT = ev[e0 + per * k], ev[e0 + per * k + 1]
            r0 = (r0 + (0 if lookup else sT - sT * sT)) * alpha % R
            r0 = (r0 + sF - sF * sF) * alpha % R
        fxi = txi = 0
        for i in range(k - 1, -1, -1):
            fxi = (fxi * beta + fx[i]) % R
            if gs:
                txi = (txi * beta + tx[i]) % R
        if gs:
            fg, tg = (fxi + gamma) % R, (txi + gamma) % R
            r01 = sxiw * fg * tg % R
            r01 = (r01 + sT * fg - sF * tg) % R if sel else (r01 + fxi - txi) % R
            r0 = (r0 + r01) * alpha % R
            bS = (l1 - alpha * fg * tg) % R
        else:
            r01 = sxiw * (((gamma - 1) * sT + 1) if sel else gamma) % R
            r0 = ((r0 + r01) * alpha - l1) % R
            fg = (fxi + gamma) % R
            if sel:
                fg = ((fg - 1) * sF + 1) % R
            bS = (l1 - alpha * fg) % R
            c = sxiw * alpha % R * dj % R * (sT if sel else 1) % R
            for i in range(k):
                B = Ad(B, M(T[i], c))
                c = c * beta % R
        B = Ad(B, M(comS[j], (dj * bS + u * vj) % R))
        E = (E + u * vj % R * sxiw - dj * r0) % R
        for P_, val in list(zip(F, fx)) + list(zip(T, tx)) + ([(selF, sF), (selT, sT)] if sel else []):
            B = Ad(B, M(P_, pw))
            E = (E + pw * val) % R
            pw = pw * v % R
        c0 += 2 * k + (2 if sel else 0)
        e0 += per * k + (2 if sel else 0)
        dj = dj * delta % R
        vj = vj * v % R
    B = Ad(B, bn.g1_neg(M(bn.G1_GEN, E)))
    A_ = Ad(Wxi, M(Wxiw, u))
    return M(A_, tau) == B
