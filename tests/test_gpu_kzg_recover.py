"""kgs_kzg_recover_cosets on the GPU, byte for byte: every (nbits, lbits) up to 2^8 with every missing pattern against
the integer references of kzg_recover_cases.py; the seams of the product tree and of its batched transforms (leaf
size and tile size read from the sources) against the polynomial each case is built from; the 0 verdict; a round
trip through kgs_kzg_open_cosets and the batch verifier; every refusal; the context contract; the device twin."""
import ctypes
import os
import random
import re

import pytest

import common
import kzg_coset_cases as CC
import kzg_open_cases as Z
import kzg_recover_cases as C

pytestmark = pytest.mark.gpu
R = C.R
KGS_E_ARG = -1

_CSRC = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "csrc")
LEAF_LOG = int(re.search(r"RC_LEAF_LOG = (\d+)", open(os.path.join(_CSRC, "kernels.hpp")).read()).group(1))
TILE_LOG = int(re.search(r"#define KGS_NTT_ELOG (\d+)", open(os.path.join(_CSRC, "ntt.hip")).read()).group(1))


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def plain(K):
    """a context without an SRS: recovery needs none"""
    c = K.Context(0)
    yield c
    c.close()


def _hip(K):
    K.lib()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


class DevBuf:
    def __init__(self, hip, data):
        self.hip, self.n, self.p = hip, len(data), ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(self.p), max(self.n, 64)) == 0
        assert hip.hipMemcpy(self.p, bytes(data), self.n, 1) == 0

    def read(self):
        out = ctypes.create_string_buffer(self.n)
        assert self.hip.hipMemcpy(out, self.p, self.n, 2) == 0
        return out.raw

    def free(self):
        self.hip.hipFree(self.p)


def ys_bytes(rows):
    return Z.mont(C.flat(rows))


def recover(c, nbits, lbits, index, rows, length, evals=False):
    got = c.kzg_recover_cosets(nbits, lbits, index, ys_bytes(rows), length, evals=evals)
    assert c.idle()
    return got


# ------------------------------------------------------------------ every small shape against the references
@pytest.mark.parametrize("nbits", range(9))
def test_every_shape_and_pattern(plain, nbits):
    """len = 1, len = n with count = m, and an odd len that is no multiple of l are among the lengths"""
    for lbits in range(nbits + 1):
        for p, pattern in enumerate(C.PATTERNS):
            for kind in C.LEN_KINDS if pattern in ("none", "minimum") else ("odd",):
                index, rows, length, coefs = C.make_case(5000 * nbits + 100 * lbits + p, nbits, lbits, pattern, kind)
                what = (nbits, lbits, pattern, kind)
                assert C.steps(index, rows, nbits, lbits, length) == (1, coefs), what
                if nbits <= 5:
                    assert C.lagrange(index, rows, nbits, lbits, length) == (1, coefs), what
                ok, got, ev = recover(plain, nbits, lbits, index, rows, length, evals=True)
                assert ok is True and got == Z.mont(coefs), what
                assert ev == Z.mont(C.evals(coefs, nbits)), what
                assert recover(plain, nbits, lbits, index, rows, length) == (True, Z.mont(coefs)), what


# ------------------------------------------------------------------ the seams of the tree
# m = 2^logm cosets, leaves of B = 2^LEAF_LOG, tile 2^TILE_LOG. A level multiplies polynomials of degree d by transforms
# of size 2d over an array of 2m (forward) and of m (inverse) elements: below one tile the radix passes, one LDS pass
# up to 2^9, a radix-2 pass beside it at 2^10, the multi-pass plans from 2^TILE_LOG on.
SEAM_LOGM = [LEAF_LOG - 1,   # below one leaf
             LEAF_LOG,       # exactly one leaf: no level
             LEAF_LOG + 1,   # two leaves: one level, arrays below a tile
             TILE_LOG - 1,   # the forward array is one tile: the one-pass levels and the 2^10 level; inverse by radix
             TILE_LOG,       # the top level is the first multi-pass transform (2^TILE_LOG), both directions
             TILE_LOG + 1,   # the first level wider than one tile (2^12)
             TILE_LOG + 2]   # 2^13
SEAMS = [(logm, 0) for logm in SEAM_LOGM] + [(TILE_LOG, 1), (TILE_LOG + 1, 1)]
SETS = ("random", "one leaf", "one per leaf", "leaf present")


def seam_missing(kind, m, rng):
    B = min(1 << LEAF_LOG, m)
    leaves = m // B
    if kind == "random":
        return {i for i in range(m) if rng.random() < 0.5} - {rng.randrange(m)}
    if kind == "one leaf":  # all in one leaf
        b = leaves // 2
        return set(rng.sample(range(b * B, (b + 1) * B), max(B // 2, 1) if m > 1 else 0))
    if kind == "one per leaf":
        return {b * B + rng.randrange(B) for b in range(leaves)} if m > 1 else set()
    b = rng.randrange(leaves)  # a whole leaf present, half of the others missing
    return {i for i in range(m) if i // B != b and rng.random() < 0.5}


def seam_case(nbits, lbits, kind, seed):
    n, l, m = C.sizes(nbits, lbits)
    rng = random.Random(seed)
    missing = seam_missing(kind, m, rng)
    index = [i for i in range(m) if i not in missing]
    rng.shuffle(index)
    return C.case_from(index, nbits, lbits, C.length_for(len(index) * l, l, "odd"), rng)


@pytest.mark.parametrize("logm,lbits", SEAMS)
def test_tree_seams(plain, logm, lbits):
    nbits = logm + lbits
    for s, kind in enumerate(SETS):
        index, rows, length, coefs = seam_case(nbits, lbits, kind, 7000 + 100 * logm + 10 * lbits + s)
        ok, got = recover(plain, nbits, lbits, index, rows, length)
        assert ok is True and got == Z.mont(coefs), (logm, lbits, kind, len(index), length)


def test_verdicts_of_tampered_values(plain):
    # values to spare at a seam shape: one wrong value and no polynomial of degree < len is left
    nbits, lbits = TILE_LOG + 1, 0
    index = seam_case(nbits, lbits, "random", 99)[0]
    index, rows, length, coefs = C.case_from(index, nbits, lbits, len(index) - 3, random.Random(98))
    rows[len(rows) // 3][0] = (rows[len(rows) // 3][0] + 1) % R
    assert recover(plain, nbits, lbits, index, rows, length)[0] is False
    # nothing to spare: every input is consistent, the answer is Lagrange's polynomial
    for nbits, lbits, pattern in ((5, 2, "minimum"), (4, 0, "random"), (3, 3, "none")):
        index, rows, length, coefs = C.make_case(41 + nbits, nbits, lbits, pattern, "max")
        assert len(index) << lbits == length
        rows[-1][-1] = (rows[-1][-1] + 5) % R
        verdict, lag = C.lagrange(index, rows, nbits, lbits, length)
        assert verdict == 1 and lag != coefs
        assert recover(plain, nbits, lbits, index, rows, length) == (True, Z.mont(lag))


# ------------------------------------------------------------------ open, lose half, verify, recover, open again
def test_round_trip_through_the_openings(K):
    nbits, lbits = 10, 4
    n, l, m = C.sizes(nbits, lbits)
    hip = _hip(K)
    c = K.Context(0)
    bufs = []
    try:
        c.load_ptau(common.oracle_ptau(11), nbits)
        rng = random.Random(2024)
        coefs = [rng.randrange(R) for _ in range(n // 2)]
        proofs, ev = c.kzg_open_cosets(Z.mont(coefs), nbits, lbits, evals=True)
        kept = sorted(rng.sample(range(m), m // 2))
        rng.shuffle(kept)
        ys = [b"".join(ev[32 * (i + m * j):32 * (i + m * j + 1)] for j in range(l)) for i in kept]
        tuples = [(0, i, y, proofs[64 * i:64 * (i + 1)]) for i, y in zip(kept, ys)]
        assert c.kzg_verify_cosets_batch(CC.tau_l_g2(lbits), CC.srs_g1(lbits), nbits, lbits, [Z.commitment(coefs)],
                                         tuples) == [True] * len(kept)
        ins = [b"".join(i.to_bytes(8, "little") for i in kept), b"".join(ys)]
        bufs = [DevBuf(hip, x) for x in ins] + [DevBuf(hip, bytes(32 * len(coefs))), DevBuf(hip, bytes(64 * m)),
                                                DevBuf(hip, bytes(32 * n))]
        d_index, d_ys, d_coef, d_proofs, d_ev = bufs
        assert c.kzg_recover_cosets_device(nbits, lbits, d_index.p, d_ys.p, len(kept), len(coefs), d_coef.p) is True
        assert c.idle() and [d_index.read(), d_ys.read()] == ins  # the inputs are only read
        c.kzg_open_cosets_device(d_coef.p, len(coefs), nbits, lbits, d_proofs.p, d_ev.p)
        assert d_coef.read() == Z.mont(coefs)
        assert d_proofs.read() == proofs and d_ev.read() == ev
    finally:
        for b in bufs:
            b.free()
        c.close()


# ------------------------------------------------------------------ refusals and the context contract
def test_refusals(K, plain):
    nbits, lbits = 4, 1
    n, l, m = C.sizes(nbits, lbits)
    index, rows, length, coefs = C.make_case(77, nbits, lbits, "alternate", "odd")
    ys = ys_bytes(rows)

    def good(c=plain):
        assert c.kzg_recover_cosets(nbits, lbits, index, ys, length) == (True, Z.mont(coefs)) and c.idle()

    def refused(word, *args, c=plain):
        with pytest.raises(K.KgsError) as e:
            c.kzg_recover_cosets(*args)
        assert e.value.code == KGS_E_ARG and word in str(e.value) and c.idle(), (word, str(e.value))
        good(c)

    good()
    for nb in (-1, 24):
        refused("nbits", nb, 0, index, ys, length)
    for lb in (-1, nbits + 1):
        refused("lbits", nbits, lb, index, ys, length)
    for ln in (0, n + 1):
        refused("len", nbits, lbits, index, ys, ln)
    refused("count", nbits, lbits, index[:1], ys[:32 * l], 2 * l + 1)                    # fewer than ceil(len / l)
    refused("count", nbits, lbits, index + [1, 3, 5, 7, 9], ys + bytes(32 * l * 5), length)  # more than m
    refused("index[2]", nbits, lbits, index[:2] + [m] + index[3:], ys, length)
    refused("index[3]", nbits, lbits, index[:3] + [index[0]] + index[4:], ys, length)
    big = R.to_bytes(32, "little")
    refused("row 1", nbits, lbits, index, ys[:32 * (l + 1)] + big + ys[32 * (l + 2):], length)
    L = K.lib()
    idx = (ctypes.c_uint64 * len(index))(*index)
    p = ctypes.cast(idx, ctypes.c_void_p)
    out = ctypes.create_string_buffer(32 * length)
    for args in ((None, ys, out), (p, None, out), (p, ys, None)):
        assert L.kgs_kzg_recover_cosets(plain.handle, nbits, lbits, args[0], args[1], len(index), length, args[2],
                                        None) == KGS_E_ARG
        assert "NULL" in L.kgs_last_error().decode() and plain.idle()
        good()
    assert L.kgs_kzg_recover_cosets(None, nbits, lbits, p, ys, len(index), length, out, None) == KGS_E_ARG
    assert L.kgs_kzg_recover_cosets_device(None, nbits, lbits, p, ys, len(index), length, out, None) == KGS_E_ARG
    c = K.Context(0)
    try:
        c.load_ptau(common.oracle_ptau(11), 10)
        c.set_shard(0, 2, lambda b: b + b)
        with pytest.raises(K.KgsError) as e:
            c.kzg_recover_cosets(nbits, lbits, index, ys, length)
        assert e.value.code == KGS_E_ARG and "shard" in str(e.value)
        c.set_shard(0, 1)
        good(c)
        c.set_group(K.Group.local(2), 0)
        with pytest.raises(K.KgsError) as e:
            c.kzg_recover_cosets(nbits, lbits, index, ys, length)
        assert e.value.code == KGS_E_ARG and "rank group" in str(e.value)
        c.set_group(None)
        good(c)
    finally:
        c.close()


def test_context_state_is_left_alone(K):
    nbits, lbits = 6, 2
    c = K.Context(0)
    try:
        c.load_ptau(common.oracle_ptau(11), 10)
        rng = random.Random(5)
        p = [rng.randrange(R) for _ in range(1 << nbits)]
        info, lag = c.srs_info(), c.srs_lagrange(nbits)
        all_ = c.kzg_open_all(Z.mont(p), nbits)
        cos = c.kzg_open_cosets(Z.mont(p), nbits, lbits)
        assert c.kzg_open_cosets_cached(nbits, lbits) and c.kzg_open_cosets_cached(nbits, 0)
        for pattern in ("random", "none"):
            index, rows, length, coefs = C.make_case(12, nbits, lbits, pattern, "odd")
            assert recover(c, nbits, lbits, index, rows, length) == (True, Z.mont(coefs))
        index, rows, length, coefs = C.make_case(13, 12, 0, "random", "odd")  # grows the shared domain tables
        assert recover(c, 12, 0, index, rows, length) == (True, Z.mont(coefs))
        with pytest.raises(K.KgsError):
            c.kzg_recover_cosets(nbits, lbits, [0, 0], bytes(64 << lbits), 1)
        assert c.idle()
        assert c.kzg_open_cosets_cached(nbits, lbits) and c.kzg_open_cosets_cached(nbits, 0)
        assert c.srs_info() == info and c.srs_lagrange(nbits) == lag
        assert c.kzg_open_all(Z.mont(p), nbits) == all_ and c.kzg_open_cosets(Z.mont(p), nbits, lbits) == cos
    finally:
        c.close()


def test_host_and_device_entry_points_agree(K, plain):
    hip = _hip(K)
    for nbits, lbits, pattern in ((7, 3, "shuffled"), (9, 0, "random"), (0, 0, "none")):
        n = 1 << nbits
        index, rows, length, coefs = C.make_case(300 + nbits, nbits, lbits, pattern, "odd")
        host = recover(plain, nbits, lbits, index, rows, length, evals=True)
        ins = [b"".join(i.to_bytes(8, "little") for i in index), ys_bytes(rows)]
        bufs = [DevBuf(hip, x) for x in ins] + [DevBuf(hip, bytes(32 * length)), DevBuf(hip, bytes(32 * n))]
        try:
            ok = plain.kzg_recover_cosets_device(nbits, lbits, bufs[0].p, bufs[1].p, len(index), length, bufs[2].p, bufs[3].p)
            assert plain.idle() and (ok, bufs[2].read(), bufs[3].read()) == host == (True, Z.mont(coefs), host[2])
            assert [bufs[0].read(), bufs[1].read()] == ins
            rows[0][0] = (rows[0][0] + 1) % R
            bad = DevBuf(hip, ys_bytes(rows))
            bufs.append(bad)
            spare = len(index) << lbits > length
            assert plain.kzg_recover_cosets_device(nbits, lbits, bufs[0].p, bad.p, len(index), length, bufs[2].p) is not spare
            assert recover(plain, nbits, lbits, index, rows, length)[0] is not spare
        finally:
            for b in bufs:
                b.free()


def test_module_level_call(K):
    index, rows, length, coefs = C.make_case(8, 5, 2, "run", "odd")
    assert K.kzg_recover_cosets(5, 2, index, ys_bytes(rows), length) == (True, Z.mont(coefs))
