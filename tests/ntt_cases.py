"""References of kgs_ntt_ex (include/kgs.h), written from the header's formulas over the plain transform:
with Python integers and oracle/poly.py up to 2^12 (`ref_py`), with the C restatement above (`ref_c`:
oracle.c's ntt and scale_powers). tests/test_oracle_c.py pins the two to each other. `ref_blocks` is the
reference of kgs_ntt_blocks: the same references block by block.

Flags are the header's values, read from it together with the coset generator.
"""
import functools
import os
import re

import common
from oracle import bn254 as bn
from oracle import poly as OP

R = bn.R
_HDR = open(os.path.join(common.ROOT, "include", "kgs.h")).read()


def _define(name):
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, _HDR, flags=re.M).group(1))


COSET_GEN = _define("KGS_NTT_COSET_GEN")
INVERSE, COSET, BITREV = _define("KGS_NTT_INVERSE"), _define("KGS_NTT_COSET"), _define("KGS_NTT_BITREV")
NO_SCALE, INPLACE, INFLIGHT = _define("KGS_NTT_NO_SCALE"), _define("KGS_NTT_INPLACE"), _define("KGS_NTT_INFLIGHT")
PY_MAX_LOGM = 12


@functools.lru_cache(None)
def rev(k, logm):
    return int(format(k, "0%db" % logm)[::-1], 2) if logm else 0


def ref_py(vals, logm, flags):
    """vals: standard-form ints (in_len of them, forward; m, inverse) -> m ints"""
    m = 1 << logm
    if not flags & INVERSE:
        a = list(vals) + [0] * (m - len(vals))
        if flags & COSET:
            a = [x * pow(COSET_GEN, j, R) % R for j, x in enumerate(a)]
        A = OP.ntt(a, False)
        return [A[rev(k, logm)] for k in range(m)] if flags & BITREV else A
    assert len(vals) == m
    e = [vals[rev(j, logm)] for j in range(m)] if flags & BITREV else list(vals)
    B = OP.ntt(e, True)
    if flags & NO_SCALE:
        B = [x * m % R for x in B]
    if flags & COSET:
        gi = pow(COSET_GEN, R - 2, R)
        B = [x * pow(gi, k, R) % R for k, x in enumerate(B)]
    return B


def _rev_rows(data, logm):
    """row k of the result = row rev(k) of data (2^logm rows of 32 bytes)"""
    import numpy as np
    m = 1 << logm
    idx = np.arange(m, dtype=np.int64)
    r = np.zeros(m, dtype=np.int64)
    for b in range(logm):
        r |= ((idx >> b) & 1) << (logm - 1 - b)
    return np.frombuffer(data, dtype=np.uint8).reshape(m, 32)[r].tobytes()


def ref_c(data, logm, flags):
    """Montgomery bytes -> Montgomery bytes, through oracle/c. Without 1/m the inverse is the forward
    transform read backwards: sum_j e_j w^(-jk) = NTT(e)[(m - k) mod m]."""
    import numpy as np
    from oracle import cbackend as C
    m = 1 << logm
    if not flags & INVERSE:
        x = bytes(data) + bytes(32 * m - len(data))
        if flags & COSET:
            x = C.scale_powers(x, COSET_GEN)
        A = C.ntt(x, False)
        return _rev_rows(A, logm) if flags & BITREV else A
    assert len(data) == 32 * m
    e = _rev_rows(data, logm) if flags & BITREV else bytes(data)
    if flags & NO_SCALE:
        rows = np.frombuffer(C.ntt(e, False), dtype=np.uint8).reshape(m, 32)
        B = rows[(m - np.arange(m, dtype=np.int64)) % m].tobytes()
    else:
        B = C.ntt(e, True)
    if flags & COSET:
        B = C.scale_powers(B, pow(COSET_GEN, R - 2, R))
    return B


def unmont(data):
    return [bn.fr_from_bytes(data[32 * i:32 * i + 32]) for i in range(len(data) // 32)]


def ref(data, logm, flags):
    """The expected bytes of Context.ntt_ex(data, logm, flags); the pass build and the buffer the
    transform writes do not change them."""
    flags &= ~(INPLACE | INFLIGHT)
    if logm <= PY_MAX_LOGM:
        return common.mont_bytes(ref_py(unmont(data), logm, flags))
    return ref_c(data, logm, flags)


def ref_blocks(data, logtotal, s, flags):
    """The expected bytes of Context.ntt_blocks(data, logtotal, s, flags) (kgs_ntt_blocks, include/kgs.h): the
    2^(logtotal - s) consecutive blocks of 2^s elements, each through `ref` on its own: forward natural in,
    bit-reversed out; inverse bit-reversed in, natural out, with 1/2^s unless NO_SCALE."""
    assert 0 <= s <= logtotal and len(data) == 32 << logtotal and not flags & ~(INVERSE | NO_SCALE | INFLIGHT)
    f = BITREV | (flags & INVERSE) | (flags & NO_SCALE if flags & INVERSE else 0)
    if s <= PY_MAX_LOGM:  # `ref` of every block, the bytes converted once for all of them
        vals, m = unmont(data), 1 << s
        return common.mont_bytes([y for at in range(0, len(vals), m) for y in ref_py(vals[at:at + m], s, f)])
    size = 32 << s
    return b"".join(ref_c(data[at:at + size], s, f) for at in range(0, len(data), size))


def random_elements(seed, count):
    """count canonical Montgomery-form elements (uniform 64-bit words, the top one cut to 60 bits: < r)"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.integers(0, 2**64 - 1, size=(count, 4), dtype=np.uint64, endpoint=True)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    return w.tobytes()
