"""CPU checks of the CIOS rows that reduce by Q* = k*q = -1 mod 2^32 (field29.hpp,
fq29::reduce_row_qstar): the constants, the exact row schedule of mul / sqr / mul2 on Python integers
with the row counts the header selects (KGS_QSTAR_ROWS, KGS_QSTAR_ROWS_CSUB, KGS_QSTAR_ROWS_MUL2 in
front of KGS_M32_ROWS*), and the interval analysis of g1_acc29::add_aff and g1_acc29::add redone with
those rows: every column accumulator below 2^64, every column carry_sub reads within the type it
declares, coordinates below 2^258.6.

The step-by-step models of add_aff and add are test_field29.py's (madd_bound, add_bound); this file
swaps in product models that know the Q* rows. The GPU side is tests/test_gpu_qstar.py.
"""
import math
import random
import re

import pytest

import test_field29 as tf

Q, MASK, RBITS = tf.Q, tf.MASK, tf.RBITS
QL = tf.QL


def _knob(name, t):
    return int(re.search(r"#define %s (\d+)" % name, t).group(1))


T = tf._hdr()
QS_MUL, QS_CSUB, QS_MUL2 = _knob("KGS_QSTAR_ROWS", T), _knob("KGS_QSTAR_ROWS_CSUB", T), _knob("KGS_QSTAR_ROWS_MUL2", T)
M32, M32_MUL2 = tf._m32_rows()
QSTAR_K = int(re.search(r"QSTAR_K = (0x[0-9a-f]+)u", T).group(1), 16)
QSTAR_R = tf._words("L9 QSTAR_R", T)
QSTAR = QSTAR_K * Q


def test_constants():
    assert all(0 <= k <= 7 for k in (QS_MUL, QS_CSUB, QS_MUL2))
    assert QSTAR_K == (-pow(Q, -1, 1 << 32)) % (1 << 32)
    assert QSTAR % (1 << 32) == (1 << 32) - 1 and QSTAR % Q == 0
    r = [QSTAR_R[0] - 8] + QSTAR_R[1:]               # limb 0 carries the 8*m of the column-0 carry
    assert all(0 <= x <= MASK for x in r) and QSTAR_R[0] < (1 << 32)
    rv = tf._d29(r)
    assert rv % 8 == 0 and rv < (1 << 257)
    assert ((1 << 32) - 1) + (rv << 29) == QSTAR    # the limbs recompose


def _extra(qs, m32):
    """largest sum_i m_i * modulus_i * 2^(29 i) the reduction rows can add to a*b"""
    e = 0
    for i in range(9):
        m = (1 << (32 if i < max(qs, m32) else 29)) - 1
        e += m * (QSTAR if i < qs else Q) << (29 * i)
    return e


def test_value_excess():
    # rows 0..6 by Q* < 2^286, row 7 by q with a 32-bit m, row 8 with a 29-bit m: the result stays
    # below a*b/2^261 + q(1 + 2^-22)
    for qs in range(8):
        assert (_extra(qs, 8) >> RBITS) < Q + (Q >> 22)
    assert (_extra(7, 8) >> RBITS) - (_extra(0, 0) >> RBITS) < (Q >> 22)


# ---- the exact schedule on Python integers ----------------------------------------------------

def _cios(rows, qs, m32):
    """fq29's CIOS loop as the header runs it: rows(i) -> [(column, product)] added in row i; rows
    < qs run reduce_row_qstar, rows < m32 reduce_row32, the others reduce_row. Every 64-bit
    accumulator is checked. Returns (value of the 9 output columns, largest output column)."""
    inv = (-pow(Q, -1, 1 << 29)) % (1 << 29)
    inv32 = (-pow(QL[0], -1, 1 << 32)) % (1 << 32)
    t = [0] * 9
    for i in range(9):
        for j, p in rows(i):
            t[j] += p
            assert t[j] < (1 << 64)
        if i < qs:
            m, h = t[0] & 0xffffffff, t[0] >> 32
            assert (t[0] + m * ((1 << 32) - 1)) == (h + m) << 32
            t = [m * QSTAR_R[j] + t[j + 1] for j in range(8)] + [m * QSTAR_R[8]]
            t[0] += 8 * h
            assert max(t) < (1 << 64)
            continue
        if i < m32:
            m = ((t[0] & 0xffffffff) * inv32) & 0xffffffff
            u = m * QL[0] + t[0]
            assert u < (1 << 64) and u % (1 << 32) == 0
            c = 8 * (u >> 32)
        else:
            m = (t[0] * inv) & MASK
            c = (m * QL[0] + t[0]) >> 29
        for j in range(1, 9):
            t[j] += m * QL[j]
            assert t[j] < (1 << 64)
        t = t[1:] + [0]
        t[0] += c
        assert t[0] < (1 << 64)
    return sum(x << (29 * j) for j, x in enumerate(t)), max(t)


def _rows_mul(al, bl):
    return lambda i: [(j, al[i] * bl[j]) for j in range(9)]


def _rows_sqr(al):
    return lambda i: [(i, al[i] * al[i])] + [(j, 2 * al[i] * al[j]) for j in range(i + 1, 9)]


def _rows_mul2(al, bl, cl, dl):
    return lambda i: [(j, al[i] * bl[j] + cl[i] * dl[j]) for j in range(9)]


def _check(rows, qs, m32, s):
    v, outc = _cios(rows, qs, m32)
    assert v % Q == s * pow(2, -RBITS, Q) % Q
    assert v <= ((s + _extra(qs, m32)) >> RBITS)
    assert v < (s >> RBITS) + Q + (Q >> 22) + 1
    return outc


def test_row_schedule_random_and_maximal():
    rnd = random.Random(2029)
    big = (1 << 261) - 1                              # every limb at 2^29 - 1
    for it in range(400):
        a = big if it == 0 else rnd.randrange(1 << 259)
        b = big if it == 0 else rnd.randrange(1 << 259)
        al, bl = tf._limbs(a), tf._limbs(b)
        for qs in {QS_MUL, QS_CSUB}:
            _check(_rows_mul(al, bl), qs, M32, a * b)
            _check(_rows_sqr(al), qs, M32, a * a)
        # mul2's operand shapes in add_aff / add: b unnormalised (T = Qv + spread(64, 1) - X3, limbs
        # up to 2^30.6), d = spread(3, 1) - PPP (limbs up to 2^29.6), a and c normalised
        c, e = (big, (1 << 256) - 1) if it == 0 else (rnd.randrange(1 << 259), rnd.randrange(1 << 256))
        cl = tf._limbs(c)
        K64, K3 = tf._spread(64, 1), tf._spread(3, 1)
        tl = [x + k for x, k in zip(bl, K64)] if it == 0 else [x + k - y for x, k, y in zip(bl, K64, tf._limbs(e))]
        dl = K3 if it == 0 else [k - y for k, y in zip(K3, tf._limbs(e % (2 * Q)))]
        assert all(0 <= x < (1 << 32) for x in tl + dl)
        _check(_rows_mul2(al, tl, cl, dl), QS_MUL2, M32_MUL2, a * tf._d29(tl) + c * tf._d29(dl))


# ---- interval analysis with the new rows -------------------------------------------------------

def _col_bounds(rows, qs, m32):
    """upper bounds of the column accumulators (largest at any point, largest output column)"""
    t, worst = [0] * 9, 0
    for i in range(9):
        for j, p in rows(i):
            t[j] += p
        worst = max(worst, max(t))
        if i < qs:
            m, h = (1 << 32) - 1, t[0] >> 32
            t = [m * QSTAR_R[j] + t[j + 1] for j in range(8)] + [m * QSTAR_R[8]]
            t[0] += 8 * h
        else:
            m = (1 << (32 if i < m32 else 29)) - 1
            u = m * QL[0] + t[0]
            worst = max(worst, u)
            for j in range(1, 9):
                t[j] += m * QL[j]
            worst = max(worst, max(t))
            t = t[1:] + [0]
            t[0] += u >> 29
        worst = max(worst, max(t))
    return worst, max(t)


def _carry_sub_type():
    body = T[T.index("static fq29 carry_sub("):]
    return re.search(r"\b(u?int64_t) c = 0;", body[:body.index("return r;")]).group(1)


class Model:
    """product models for test_field29's madd_bound / add_bound, recording the worst bounds seen"""

    def __init__(self):
        self.acc = self.fused = self.acc_mul2 = 0
        self.mul2_args = []

    def out(self, s, qs, m32):
        o = ((s + _extra(qs, m32)) >> RBITS) + 1
        assert o <= (1 << RBITS)
        return tf.V(o, MASK)

    def _prod(self, rows, s, fused):
        worst, outc = _col_bounds(rows, QS_CSUB if fused else QS_MUL, M32)
        assert worst < (1 << 64), "column overflow %.3f" % math.log2(worst)
        self.acc = max(self.acc, worst)
        if fused:
            # carry_sub adds K_j - b_j < 2^32 and the running carry (< 2^36) to each column
            limit = (1 << 63) if _carry_sub_type() == "int64_t" else (1 << 64)
            assert outc + (1 << 32) + (1 << 36) < limit, "carry_sub column %.3f" % math.log2(outc)
            self.fused = max(self.fused, outc)
        return self.out(s, QS_CSUB if fused else QS_MUL, M32)

    def mul(self, a, b, fused=False):
        return self._prod(_rows_mul(tf._limbs_max(a), tf._limbs_max(b)), a.val * b.val, fused)

    def sqr(self, a, fused=False):
        return self._prod(_rows_sqr(tf._limbs_max(a)), a.val * a.val, fused)

    def mul2(self, a, b, c, d):
        ls = [tf._limbs_max(x) for x in (a, b, c, d)]
        self.mul2_args.append(ls)
        worst, _ = _col_bounds(_rows_mul2(*ls), QS_MUL2, M32_MUL2)
        assert worst < (1 << 64), "column overflow %.3f" % math.log2(worst)
        self.acc_mul2 = max(self.acc_mul2, worst)
        s = a.val * b.val + c.val * d.val
        assert s < (1 << RBITS) * ((1 << RBITS) - Q)
        return self.out(s, QS_MUL2, M32_MUL2)


@pytest.fixture
def model(monkeypatch):
    m = Model()
    monkeypatch.setattr(tf, "_mul", m.mul)
    monkeypatch.setattr(tf, "_sqr", m.sqr)
    monkeypatch.setattr(tf, "_mul2", m.mul2)
    return m


def _fixed_point():
    vb = 2 * Q
    for _ in range(50):
        nxt = max(tf.madd_bound(vb), vb)
        if nxt == vb:
            break
        vb = nxt
    return vb


def test_add_aff_and_add_bounds(model):
    vb = _fixed_point()
    assert tf.madd_bound(vb) <= vb
    assert tf.add_bound(vb) <= vb
    assert 2 * Q <= vb and math.log2(vb) < 258.6     # field29.hpp: coordinates < 2^258.6
    assert model.acc < (1 << 64) and model.acc_mul2 < (1 << 64) and model.fused > 0
    print("coordinates < 2^%.3f, mul/sqr accumulators < 2^%.3f, mul2 < 2^%.3f, carry_sub columns < 2^%.3f (%s)"
          % (math.log2(vb), math.log2(model.acc), math.log2(model.acc_mul2), math.log2(model.fused),
             _carry_sub_type()))


def test_mul2_exact_schedule_at_the_interval_maxima(model):
    # the limb maxima the interval analysis hands to mul2, run through the exact schedule: the
    # analysis' worst case is a real input of the row code, and it does not overflow
    vb = _fixed_point()
    tf.add_bound(vb)
    assert model.mul2_args
    for al, bl, cl, dl in model.mul2_args[-2:]:
        _check(_rows_mul2(al, bl, cl, dl), QS_MUL2, M32_MUL2, tf._d29(al) * tf._d29(bl) + tf._d29(cl) * tf._d29(dl))
