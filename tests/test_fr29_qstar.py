"""CPU checks of mul29's CIOS rows that reduce by R* = k*r = -1 mod 2^32 (fr29.hpp): the constants,
the exact row schedule with the header's row count (KGS_QSTAR_ROWS_FR rows by R*, then the 32-bit-m
rows up to row 7, the 29-bit m in row 8) on Python integers, and the column and output bounds over all
inputs (a < 2^256, w < r): every accumulator below 2^64, the result below 2r.

The GPU side is tests/test_gpu_qstar.py."""
import math
import random
import re

import test_fr29 as tr

R, MASK, P, INV, INV32 = tr.R, tr.MASK, tr.P, tr.INV, tr.INV32
T = tr._hdr()
QS = int(re.search(r"#define KGS_QSTAR_ROWS_FR (\d+)", T).group(1))
QSTAR_K = tr._const("QSTAR_K", T)
QSTAR_R = tr._arr("QSTAR_R", T)
RSTAR = QSTAR_K * R


def test_constants():
    assert 0 <= QS <= 7
    assert QSTAR_K == (-pow(R, -1, 1 << 32)) % (1 << 32)
    assert RSTAR % (1 << 32) == (1 << 32) - 1 and RSTAR % R == 0
    s = [QSTAR_R[0] - 8] + QSTAR_R[1:]                # limb 0 carries the 8*m of the column-0 carry
    assert all(0 <= x <= MASK for x in s)
    sv = sum(x << (29 * j) for j, x in enumerate(s))
    assert sv % 8 == 0 and sv < (1 << 257)
    assert ((1 << 32) - 1) + (sv << 29) == RSTAR     # the limbs recompose


def _extra(qs):
    """largest sum_i m_i * modulus_i * 2^(29 i) the reduction rows can add to a*w"""
    return sum((((1 << (32 if i < 8 else 29)) - 1) * (RSTAR if i < qs else R)) << (29 * i) for i in range(9))


def mul29(al, wl, qs):
    """fr29.hpp mul29 step by step on limb lists; returns (result value, largest accumulator seen)"""
    t, worst = [0] * 9, 0
    for i in range(9):
        for j in range(9):
            t[j] += al[i] * wl[j]
        worst = max(worst, max(t))
        if i < qs:
            m, h = t[0] & 0xffffffff, t[0] >> 32
            assert t[0] + m * ((1 << 32) - 1) == (h + m) << 32
            t = [m * QSTAR_R[j] + t[j + 1] for j in range(8)] + [m * QSTAR_R[8]]
            t[0] += 8 * h
        elif i < 8:
            m = (t[0] * INV32) % (1 << 32)
            u = m * P[0] + t[0]
            assert u % (1 << 32) == 0
            for j in range(1, 9):
                t[j] += m * P[j]
            worst = max(worst, u, max(t))
            t = t[1:] + [0]
            t[0] += (u >> 32) * 8
        else:
            m = (t[0] * INV) & MASK
            u = m * P[0] + t[0]
            assert u % (1 << 29) == 0
            for j in range(1, 9):
                t[j] += m * P[j]
            worst = max(worst, u, max(t))
            t = t[1:] + [0]
            t[0] += u >> 29
        worst = max(worst, max(t))
    return sum(x << (29 * j) for j, x in enumerate(t)), worst


def check(a, w, qs=QS):
    v, worst = mul29(tr.unpack(a), tr.unpack(w), qs)
    assert worst < (1 << 64), "column overflow"
    assert v % R == a * w * pow(2, -261, R) % R
    assert v <= (a * w + _extra(qs)) >> 261
    assert v < 2 * R
    return worst


def test_row_schedule_extremes_and_random():
    rnd = random.Random(31)
    wmax = R - 1
    cases = [((1 << 256) - 1, wmax), (4 * R - 1, wmax), (2 * R - 1, wmax), (0, wmax), ((1 << 256) - 1, 0),
             ((1 << 256) - 1, (1 << 254) % R), (1, 1), (R - 1, R - 1), (0, 0),
             (sum(MASK << (29 * j) for j in range(8)) + (((1 << 24) - 1) << 232), wmax)]
    for _ in range(3000):
        a = rnd.randrange(1 << 256) if rnd.random() < 0.5 else rnd.randrange(4 * R)
        cases.append((a, rnd.randrange(R)))
    for a, w in cases:
        check(a, w)
    # knobs 0 and QS agree modulo r (the parent's rows against the new ones)
    for a, w in cases[:200]:
        assert mul29(tr.unpack(a), tr.unpack(w), 0)[0] % R == mul29(tr.unpack(a), tr.unpack(w), QS)[0] % R


def test_column_and_output_bounds():
    """worst case over ALL inputs: per-limb maxima (a < 2^256: limbs < 2^29, the top < 2^24; w < r)"""
    amax = [MASK] * 8 + [(1 << 24) - 1]
    wmax = [MASK] * 8 + [R >> 232]
    t, worst = [0] * 9, 0
    for i in range(9):
        for j in range(9):
            t[j] += amax[i] * wmax[j]
        worst = max(worst, max(t))
        if i < QS:
            m, h = (1 << 32) - 1, t[0] >> 32
            t = [m * QSTAR_R[j] + t[j + 1] for j in range(8)] + [m * QSTAR_R[8]]
            t[0] += 8 * h
        else:
            mbits = 32 if i < 8 else 29
            m = (1 << mbits) - 1
            u = m * P[0] + t[0]
            for j in range(1, 9):
                t[j] += m * P[j]
            worst = max(worst, u, max(t))
            t = t[1:] + [0]
            t[0] += u >> 29
        worst = max(worst, max(t))
    print("mul29 accumulators < 2^%.3f" % math.log2(worst))
    assert worst < (1 << 64)
    out = (((1 << 256) - 1) * (R - 1) + _extra(QS) >> 261) + 1
    print("mul29 output < %.4f r" % (out / R))
    assert out < 2 * R
    # the exact schedule on those limb maxima (a real input of the row code) stays below 2^64 too
    v, w2 = mul29(amax, wmax, QS)
    assert w2 <= worst
