"""kgs_kzg_recover_cosets_many on the GPU, byte for byte: every small shape and polys in {1, 2, 3, 5}, with independent
and shared sets, against the single call per polynomial and against the integer references; polys = 1 against the single
call up to 2^8; the seams of the batched tree, of m below one leaf, of the size-n block transforms and of the padding to
a power of two; every status in one call; the stride; a round trip through kgs_kzg_open_cosets_many and the batch
verifier; every refusal; the context contract; the device twin; the timing helper."""
import ctypes
import json
import os
import random

import pytest

import common
import kzg_coset_cases as CC
import kzg_open_cases as Z
import kzg_recover_cases as C
import kzg_recover_many_cases as M
import test_gpu_kzg_recover as G  # LEAF_LOG / TILE_LOG read from the sources, SEAM_LOGM, seam_missing, DevBuf

pytestmark = pytest.mark.gpu
R = C.R
KGS_E_ARG = -1
LEAF_LOG, TILE_LOG = G.LEAF_LOG, G.TILE_LOG
DevBuf = G.DevBuf
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def plain(K):
    """a context without an SRS: recovery needs none"""
    c = K.Context(0)
    yield c
    c.close()


def ys_bytes(rows):
    return Z.mont(C.flat(rows))


def recover_many(c, case, evals=False, **kw):
    got = c.kzg_recover_cosets_many(case.nbits, case.lbits, case.poly_of, case.index, ys_bytes(case.rows), case.length,
                                    case.polys, evals=evals, **kw)
    assert c.idle()
    return got


def check_expected(case, got, what):
    """the statuses, and the bytes of every recovered polynomial against what the case was built from"""
    status, coefs, ev = got
    assert status == case.status(), what
    L, n = 32 * case.length, 32 << case.nbits
    for b, (s, want) in enumerate(case.expect):
        if s == M.OK:
            assert coefs[L * b:L * (b + 1)] == Z.mont(want), (what, b)
            if ev is not None:
                assert ev[n * b:n * (b + 1)] == Z.mont(C.evals(want, case.nbits)), (what, b)


def check_single(c, case, got, what):
    """polynomial by polynomial against kgs_kzg_recover_cosets on its own cells: verdict and bytes"""
    status, coefs, ev = got
    L, n = 32 * case.length, 32 << case.nbits
    for b, (index, rows) in enumerate(case.cells_of):
        if len(index) < M.need(case.length, case.lbits):
            assert status[b] == M.TOO_FEW, (what, b)
            continue
        one = c.kzg_recover_cosets(case.nbits, case.lbits, index, ys_bytes(rows), case.length, evals=ev is not None)
        assert status[b] == (M.OK if one[0] else M.NO_POLY), (what, b)
        if one[0]:
            assert coefs[L * b:L * (b + 1)] == one[1], (what, b)
            if ev is not None:
                assert ev[n * b:n * (b + 1)] == one[2], (what, b)


# ------------------------------------------------------------------ every small shape
@pytest.mark.parametrize("nbits", range(7))
def test_every_small_shape(plain, nbits):
    """lengths 1, n and odd; per-polynomial patterns and one shared set"""
    for lbits in range(nbits + 1):
        for polys in (1, 2, 3, 5):
            for shared in (False, True):
                for kind in M.LEN_KINDS:
                    case = M.make_many(3000 * nbits + 100 * lbits + 10 * polys + shared, nbits, lbits, polys, shared, kind,
                                       first_pattern=lbits + polys)
                    what = (nbits, lbits, polys, shared, kind, case.length)
                    for b in range(polys):
                        assert M.reference(case, b, with_lagrange=nbits <= 4) == case.expect[b], (what, b)
                    got = recover_many(plain, case, evals=True)
                    check_expected(case, got, what)
                    check_single(plain, case, got, what)
                    assert recover_many(plain, case)[:2] == got[:2], what


@pytest.mark.parametrize("nbits", range(9))
def test_one_polynomial_is_the_single_call(plain, nbits):
    for lbits in range(nbits + 1):
        for p, pattern in enumerate(C.PATTERNS):
            index, rows, length, coefs = C.make_case(6000 * nbits + 100 * lbits + p, nbits, lbits, pattern, "odd")
            one = plain.kzg_recover_cosets(nbits, lbits, index, ys_bytes(rows), length, evals=True)
            got = plain.kzg_recover_cosets_many(nbits, lbits, [0] * len(index), index, ys_bytes(rows), length, 1, evals=True)
            assert plain.idle() and one[0] is True and one[1] == Z.mont(coefs)
            assert got == ([1], one[1], one[2]), (nbits, lbits, pattern)


# ------------------------------------------------------------------ the seams
def seam_many(nbits, lbits, polys, seed, shift=0):
    """polynomial b over seam_missing's kind (b + shift) mod 4, so neighbours differ; one odd length for all"""
    n, l, m = C.sizes(nbits, lbits)
    rng = random.Random(seed)
    sets = []
    for b in range(polys):
        missing = G.seam_missing(G.SETS[(b + shift) % len(G.SETS)], m, rng)
        s = [i for i in range(m) if i not in missing]
        rng.shuffle(s)
        sets.append(s)
    length = C.length_for(min(len(s) for s in sets) * l, l, "odd")
    return M.from_sets(seed + 1, nbits, lbits, sets, length)


def run_seam(c, nbits, lbits, polys, seed, shifts=(0, 1), evals=False):
    for shift in shifts:  # two calls: all four kinds of sets meet every position of three
        case = seam_many(nbits, lbits, polys, seed + shift, shift)
        check_expected(case, recover_many(c, case, evals=evals), (nbits, lbits, polys, shift, case.length))


@pytest.mark.parametrize("logm", G.SEAM_LOGM)
def test_tree_seams(plain, logm):
    """polys = 3, P = 4: the array of P m slots crosses a tile where the single tree does not"""
    run_seam(plain, logm, 0, 3, 11000 + 10 * logm)


def test_many_polynomials_below_one_leaf(plain):
    """m = 2^(LEAF_LOG - 1), 70 polynomials: P m exceeds a tile and two polynomials share a would-be leaf"""
    polys = 70
    assert (128 << (LEAF_LOG - 1)) > 1 << TILE_LOG
    run_seam(plain, LEAF_LOG - 1, 0, polys, 12000, shifts=(0,), evals=True)
    run_seam(plain, LEAF_LOG + 1, 2, polys, 12100, shifts=(1,))  # and with l > 1


@pytest.mark.parametrize("nbits,polys", [(3, 300), (4, 3), (8, 3), (9, 3), (10, 3), (11, 3), (12, 3), (13, 3)])
def test_block_transform_seams(plain, nbits, polys):
    """a trivial tree (m = 8): the radix passes alone on an array above a tile (2^3 x 300), below a tile (2^8 x 3), one
    LDS pass, the 2^10 radix-2 companion, the multi-pass plans"""
    run_seam(plain, nbits, nbits - 3, polys, 13000 + 10 * nbits, shifts=(0,), evals=True)
    run_seam(plain, nbits, nbits - 3, polys, 13500 + 10 * nbits, shifts=(1,))


@pytest.mark.parametrize("nbits,lbits", [(4, 0), (4, 1)])
def test_the_four_stage_pass(plain, nbits, lbits):
    """130 polynomials, P = 256: blocks of 2^4 over an array of 2^12 take the one LDS pass of four stages (two register
    rounds of two), which no whole transform and no shape above launches. (4, 0): on the m side and the n side;
    (4, 1): on the n side, beside m = 8 by the radix pass"""
    assert 4 + 8 >= TILE_LOG
    run_seam(plain, nbits, lbits, 130, 15000 + 10 * lbits, evals=True)


@pytest.mark.parametrize("polys", [7, 8, 9, 31, 32, 33])
def test_padding_to_a_power_of_two(plain, polys):
    run_seam(plain, 6, 3, polys, 14000 + polys, evals=True)


# ------------------------------------------------------------------ statuses
def status_cases():
    yield M.make_statuses(21, 5, 2)
    nbits, lbits = LEAF_LOG + 1 + 4, 4  # two leaves and one level per tree; P n = 8 tiles
    rng = random.Random(22)
    m = 1 << (nbits - lbits)
    sets = []
    for kind in ("one leaf", "one per leaf", "leaf present"):
        missing = G.seam_missing(kind, m, rng)
        sets.append([i for i in range(m) if i not in missing])
    yield M.make_statuses(23, nbits, lbits, sets)


def test_every_status_in_one_call(K, plain):
    for case in status_cases():
        what = (case.nbits, case.lbits)
        assert case.status() == [1, 0, 1, 2, 2, 1], what
        got = recover_many(plain, case, evals=True)
        check_expected(case, got, what)
        check_single(plain, case, got, what)
        L = K.lib()
        po = (ctypes.c_uint32 * len(case.poly_of))(*case.poly_of)
        idx = (ctypes.c_uint64 * len(case.index))(*case.index)
        ys = ys_bytes(case.rows)
        coef = ctypes.create_string_buffer(32 * case.length * case.polys)
        st = ctypes.create_string_buffer(case.polys)
        args = (plain.handle, case.nbits, case.lbits, case.polys, ctypes.cast(po, ctypes.c_void_p),
                ctypes.cast(idx, ctypes.c_void_p), ctypes.cast(ctypes.c_char_p(ys), ctypes.c_void_p), len(case.index),
                case.length, case.length, coef, None)
        assert L.kgs_kzg_recover_cosets_many(*args, st) == 0 and list(st.raw) == case.status() and plain.idle()
        assert L.kgs_kzg_recover_cosets_many(*args, None) == 0 and plain.idle()  # status_out == NULL: the same return
        ok = [b for b, s in enumerate(case.status()) if s == 1]
        for b in ok:
            assert coef.raw[32 * case.length * b:32 * case.length * (b + 1)] == Z.mont(case.expect[b][1])
        # the recovered polynomials alone: the return is 1
        keep = [k for k, b in enumerate(case.poly_of) if b in ok]
        sub = plain.kzg_recover_cosets_many(case.nbits, case.lbits, [ok.index(case.poly_of[k]) for k in keep],
                                            [case.index[k] for k in keep], ys_bytes([case.rows[k] for k in keep]),
                                            case.length, len(ok))
        assert sub[0] == [1] * len(ok)
        assert sub[1] == b"".join(Z.mont(case.expect[b][1]) for b in ok)


def test_no_polynomials_and_no_cells(K, plain):
    assert plain.kzg_recover_cosets_many(4, 1, [], [], b"", 5, 0) == ([], b"", None)
    status, _, _ = plain.kzg_recover_cosets_many(4, 1, [], [], b"", 5, 3, evals=True)
    assert status == [2, 2, 2] and plain.idle()
    L = K.lib()
    coef = ctypes.create_string_buffer(32 * 15)
    assert L.kgs_kzg_recover_cosets_many(plain.handle, 4, 1, 3, None, None, None, 0, 5, 5, coef, None, None) == 0
    assert L.kgs_kzg_recover_cosets_many(plain.handle, 4, 1, 0, None, None, None, 0, 5, 5, None, None, None) == 1


# ------------------------------------------------------------------ the stride
def test_stride_leaves_the_gaps_alone(K, plain):
    hip = G._hip(K)
    case = M.make_many(31, 7, 3, 5)
    length, polys, stride = case.length, case.polys, case.length + 3
    rnd = random.Random(32)
    sentinel = bytearray(rnd.randbytes(32 * stride * polys))
    want = bytearray(sentinel)
    for b, (_, coefs) in enumerate(case.expect):
        want[32 * stride * b:32 * (stride * b + length)] = Z.mont(coefs)
    out = bytearray(sentinel)
    status, got, _ = recover_many(plain, case, stride=stride, coefs_out=out)
    assert status == [1] * polys and got == bytes(want) and bytes(out) == bytes(want)
    ins = [b"".join(b.to_bytes(4, "little") for b in case.poly_of), b"".join(i.to_bytes(8, "little") for i in case.index),
           ys_bytes(case.rows)]
    bufs = [DevBuf(hip, x) for x in ins] + [DevBuf(hip, bytes(sentinel)), DevBuf(hip, bytes(32 * polys << case.nbits))]
    try:
        ok, st = plain.kzg_recover_cosets_many_device(case.nbits, case.lbits, polys, bufs[0].p, bufs[1].p, bufs[2].p,
                                                      len(case.index), length, stride, bufs[3].p, bufs[4].p)
        assert plain.idle() and ok is True and st == [1] * polys
        assert bufs[3].read() == bytes(want)
        assert bufs[4].read() == b"".join(Z.mont(C.evals(coefs, case.nbits)) for _, coefs in case.expect)
        assert [b.read() for b in bufs[:3]] == ins  # the inputs are only read
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------ open, lose half, verify, recover, open again
def test_round_trip_through_the_openings(K):
    nbits, lbits, polys = 8, 3, 5
    n, l, m = C.sizes(nbits, lbits)
    length, stride = n // 2, n // 2 + 5
    hip = G._hip(K)
    c = K.Context(0)
    bufs = []
    try:
        c.load_ptau(common.oracle_ptau(11), nbits)
        rng = random.Random(2025)
        ps = [[rng.randrange(R) for _ in range(length)] for _ in range(polys)]
        proofs, evs = c.kzg_open_cosets_many([Z.mont(p) for p in ps], nbits, lbits, evals=True)
        cells = [(b, i) for b in range(polys) for i in rng.sample(range(m), m // 2)]  # a different half per polynomial
        rng.shuffle(cells)
        ys = [b"".join(evs[b][32 * (i + m * j):32 * (i + m * j + 1)] for j in range(l)) for b, i in cells]
        ins = [b"".join(b.to_bytes(4, "little") for b, _ in cells), b"".join(i.to_bytes(8, "little") for _, i in cells),
               b"".join(ys), b"".join(proofs[b][64 * i:64 * (i + 1)] for b, i in cells)]
        sentinel = rng.randbytes(32 * stride * polys)
        bufs = [DevBuf(hip, x) for x in ins] + [DevBuf(hip, sentinel), DevBuf(hip, bytes(64 * m * polys)),
                                                DevBuf(hip, bytes(32 * n * polys))]
        d_of, d_index, d_ys, d_pi, d_coef, d_proofs, d_ev = bufs
        commits = [Z.commitment(p) for p in ps]
        assert c.kzg_verify_cosets_batch_device(CC.tau_l_g2(lbits), CC.srs_g1(lbits), nbits, lbits, commits, d_of.p,
                                                d_index.p, d_ys.p, d_pi.p, len(cells), bytes(range(32))) == [True] * len(cells)
        # the arrays just verified, commit_of as poly_of, straight into a strided buffer
        ok, st = c.kzg_recover_cosets_many_device(nbits, lbits, polys, d_of.p, d_index.p, d_ys.p, len(cells), length,
                                                  stride, d_coef.p)
        assert c.idle() and ok is True and st == [1] * polys
        assert [b.read() for b in bufs[:4]] == ins
        c.kzg_open_cosets_many_device(d_coef.p.value, polys, stride, length, nbits, lbits, d_proofs.p.value, d_ev.p.value)
        assert d_proofs.read() == b"".join(proofs) and d_ev.read() == b"".join(evs)
        got = d_coef.read()
        for b in range(polys):
            assert got[32 * stride * b:32 * (stride * b + length)] == Z.mont(ps[b])
            assert got[32 * (stride * b + length):32 * stride * (b + 1)] == sentinel[32 * (stride * b + length):32 * stride * (b + 1)]
    finally:
        for b in bufs:
            b.free()
        c.close()


# ------------------------------------------------------------------ refusals and the context contract
def test_refusals(K, plain):
    nbits, lbits, polys = 4, 1, 3
    n, l, m = C.sizes(nbits, lbits)
    case = M.make_many(77, nbits, lbits, polys)
    po, index, ys, length = case.poly_of, case.index, ys_bytes(case.rows), case.length
    count = len(index)
    want = b"".join(Z.mont(coefs) for _, coefs in case.expect)
    assert count >= 6

    def good(c=plain):
        assert c.kzg_recover_cosets_many(nbits, lbits, po, index, ys, length, polys)[:2] == ([1] * polys, want) and c.idle()

    def refused(word, *args, c=plain, **kw):
        with pytest.raises(K.KgsError) as e:
            c.kzg_recover_cosets_many(*args, **kw)
        assert e.value.code == KGS_E_ARG and word in str(e.value) and c.idle(), (word, str(e.value))
        assert "kgs_kzg_recover_cosets_many" in str(e.value)
        good(c)

    good()
    for nb in (-1, 24):
        refused("nbits", nb, 0, po, index, ys, length, polys)
    for lb in (-1, nbits + 1):
        refused("lbits", nbits, lb, po, index, ys, length, polys)
    for ln in (0, n + 1):
        refused("len", nbits, lbits, po, index, ys, ln, polys)
    refused("polys", nbits, lbits, po, index, ys, length, ((1 << 24) >> nbits) + 1)
    refused("count", nbits, lbits, [0] * (m + 1), list(range(m)) + [0], bytes(32 * l * (m + 1)), length, 1)  # above polys m
    refused("stride", nbits, lbits, po, index, ys, length, polys, stride=length - 1)

    def cells(changes):
        p2, i2 = list(po), list(index)
        for k, (b, i) in changes.items():
            p2[k], i2[k] = po[k] if b is None else b, index[k] if i is None else i
        return p2, i2

    # a polynomial or a coset out of range: one class, the lowest cell named in either order
    refused("poly_of[2] = 3", nbits, lbits, *cells({2: (polys, None), 4: (None, m)}), ys, length, polys)
    refused("index[2] = 8", nbits, lbits, *cells({2: (None, m), 4: (polys, None)}), ys, length, polys)
    refused("poly_of[1] = 4294967295", nbits, lbits, *cells({1: (2 ** 32 - 1, None)}), ys, length, polys)
    refused("index[5]", nbits, lbits, *cells({5: (None, 2 ** 64 - 1)}), ys, length, polys)
    # a pair named again: the later cell of the lowest such pair, whichever pair comes first
    refused("index[3]", nbits, lbits, *cells({3: (po[1], index[1]), 5: (po[0], index[0])}), ys, length, polys)
    refused("index[4]", nbits, lbits, *cells({5: (po[1], index[1]), 4: (po[0], index[0])}), ys, length, polys)
    refused("second time", nbits, lbits, *cells({count - 1: (po[0], index[0])}), ys, length, polys)
    # the same coset of two polynomials is no repetition
    big = R.to_bytes(32, "little")

    def with_big(*elems):
        y = bytearray(ys)
        for e in elems:
            y[32 * e:32 * (e + 1)] = big
        return bytes(y)

    refused("value 1 of row 1", nbits, lbits, po, index, with_big(l + 1, 4 * l), length, polys)
    refused("value 0 of row 2", nbits, lbits, po, index, with_big(3 * l + 1, 2 * l), length, polys)
    L = K.lib()
    cpo = (ctypes.c_uint32 * count)(*po)
    idx = (ctypes.c_uint64 * count)(*index)
    pp, pi = ctypes.cast(cpo, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)
    py = ctypes.cast(ctypes.c_char_p(ys), ctypes.c_void_p)
    out = ctypes.create_string_buffer(32 * length * polys)
    for args in ((None, pi, py, out), (pp, None, py, out), (pp, pi, None, out), (pp, pi, py, None)):
        assert L.kgs_kzg_recover_cosets_many(plain.handle, nbits, lbits, polys, args[0], args[1], args[2], count, length,
                                             length, args[3], None, None) == KGS_E_ARG
        assert "NULL" in L.kgs_last_error().decode() and plain.idle()
        good()
    for entry in (L.kgs_kzg_recover_cosets_many, L.kgs_kzg_recover_cosets_many_device):
        assert entry(None, nbits, lbits, polys, pp, pi, py, count, length, length, out, None, None) == KGS_E_ARG
    c = K.Context(0)
    try:
        c.load_ptau(common.oracle_ptau(11), 10)
        c.set_shard(0, 2, lambda b: b + b)
        with pytest.raises(K.KgsError) as e:
            c.kzg_recover_cosets_many(nbits, lbits, po, index, ys, length, polys)
        assert e.value.code == KGS_E_ARG and "shard" in str(e.value)
        c.set_shard(0, 1)
        good(c)
        c.set_group(K.Group.local(2), 0)
        with pytest.raises(K.KgsError) as e:
            c.kzg_recover_cosets_many(nbits, lbits, po, index, ys, length, polys)
        assert e.value.code == KGS_E_ARG and "rank group" in str(e.value)
        c.set_group(None)
        good(c)
    finally:
        c.close()


def _golden_proof(K):
    """the smallest golden grand-sum case through the module-level prover (as the sibling tests' helper)"""
    case = min((x for x in GOLD["cases"] if x["kind"] == "grandsum"), key=lambda x: (x["nbits"], x["npols"]))
    Fs, Ts, sF, sT = common.make_inputs(case["seed"], case["nbits"], case["npols"], case["selected"])
    eF, eT = [K.Evaluations(x) for x in Fs], [K.Evaluations(x) for x in Ts]
    proof = K.grandsum_prover(common.oracle_ptau(11), eF if case["npols"] > 1 else eF[0],
                              eT if case["npols"] > 1 else eT[0],
                              K.Evaluations(sF) if sF else None, K.Evaluations(sT) if sT else None)
    got = {sec: {k: v.hex() for k, v in proof[sec].items()} for sec in ("commitments", "evaluations")}
    return got, case["proof"], case["nbits"]


def test_context_state_is_left_alone(K):
    """on the context the prover uses: a golden proof, the SRS, the caches and the single call's results are the same
    before and after recover-many calls, among them a refused one and one that grows the domain tables"""
    got, want, gbits = _golden_proof(K)
    assert got == want
    c = K._context(0)  # the context the module-level prover keeps the SRS on
    nbits, lbits = 6, 2
    rng = random.Random(5)
    p = Z.mont([rng.randrange(R) for _ in range(1 << gbits)])
    info, lag = c.srs_info(), c.srs_lagrange(gbits)
    all_ = c.kzg_open_all(p, gbits)
    cos = c.kzg_open_cosets(p, gbits, 0)
    assert c.kzg_open_cosets_cached(gbits, 0)
    index, rows, length, coefs = C.make_case(12, nbits, lbits, "random", "odd")
    single = c.kzg_recover_cosets(nbits, lbits, index, ys_bytes(rows), length)
    for shared in (False, True):
        case = M.make_many(12 + shared, nbits, lbits, 3, shared)
        check_expected(case, recover_many(c, case, evals=True), shared)
    case = M.make_many(14, 12, 0, 2)  # grows the shared domain tables
    check_expected(case, recover_many(c, case), "grown")
    with pytest.raises(K.KgsError):
        c.kzg_recover_cosets_many(nbits, lbits, [0, 0], [0, 0], bytes(64 << lbits), 1, 2)  # a pair named twice
    assert c.idle()
    assert c.kzg_recover_cosets(nbits, lbits, index, ys_bytes(rows), length) == single == (True, Z.mont(coefs))
    assert c.kzg_open_cosets_cached(gbits, 0)
    assert c.srs_info() == info and c.srs_lagrange(gbits) == lag
    assert c.kzg_open_all(p, gbits) == all_ and c.kzg_open_cosets(p, gbits, 0) == cos
    assert _golden_proof(K)[0] == want


def test_host_and_device_entry_points_agree(K, plain):
    hip = G._hip(K)
    cases = [M.make_many(301, 7, 3, 3), M.make_many(302, 9, 0, 2), M.make_many(303, 0, 0, 4), M.make_statuses(304, 6, 2)]
    for case in cases:
        nbits, lbits, polys, length = case.nbits, case.lbits, case.polys, case.length
        host = recover_many(plain, case, evals=True)
        ins = [b"".join(b.to_bytes(4, "little") for b in case.poly_of), b"".join(i.to_bytes(8, "little") for i in case.index),
               ys_bytes(case.rows)]
        bufs = [DevBuf(hip, x) for x in ins] + [DevBuf(hip, bytes(32 * length * polys)), DevBuf(hip, bytes(32 * polys << nbits))]
        try:
            ok, st = plain.kzg_recover_cosets_many_device(nbits, lbits, polys, bufs[0].p, bufs[1].p, bufs[2].p,
                                                          len(case.index), length, length, bufs[3].p, bufs[4].p)
            assert plain.idle() and st == host[0] == case.status() and ok is (set(st) == {1})
            assert plain.kzg_recover_cosets_many_device(nbits, lbits, polys, bufs[0].p, bufs[1].p, bufs[2].p, len(case.index),
                                                        length, length, bufs[3].p, status=False) is ok
            coef, ev = bufs[3].read(), bufs[4].read()
            for b, s in enumerate(st):
                if s == 1:
                    assert coef[32 * length * b:32 * length * (b + 1)] == host[1][32 * length * b:32 * length * (b + 1)]
                    assert ev[(32 << nbits) * b:(32 << nbits) * (b + 1)] == host[2][(32 << nbits) * b:(32 << nbits) * (b + 1)]
            assert [b.read() for b in bufs[:3]] == ins
        finally:
            for b in bufs:
                b.free()
    # a refusal found on the device names the same cell through the device entry
    case = cases[0]
    index = list(case.index)
    index[3] = 1 << 40
    bufs = [DevBuf(hip, b"".join(b.to_bytes(4, "little") for b in case.poly_of)),
            DevBuf(hip, b"".join(i.to_bytes(8, "little") for i in index)), DevBuf(hip, ys_bytes(case.rows)),
            DevBuf(hip, bytes(32 * case.length * case.polys))]
    try:
        with pytest.raises(K.KgsError) as e:
            plain.kzg_recover_cosets_many_device(case.nbits, case.lbits, case.polys, bufs[0].p, bufs[1].p, bufs[2].p,
                                                 len(index), case.length, case.length, bufs[3].p)
        assert "kgs_kzg_recover_cosets_many_device: index[3] = %d" % (1 << 40) in str(e.value) and plain.idle()
    finally:
        for b in bufs:
            b.free()


def test_module_level_call(K):
    case = M.make_many(8, 5, 2, 3)
    got = K.kzg_recover_cosets_many(5, 2, case.poly_of, case.index, ys_bytes(case.rows), case.length, 3)
    assert got == ([1, 1, 1], b"".join(Z.mont(coefs) for _, coefs in case.expect), None)


def test_timing_helper(K, plain):
    hip = G._hip(K)
    nbits, lbits, polys, reps = 8, 3, 3, 2
    case = M.make_many(55, nbits, lbits, polys)
    order = sorted(range(len(case.index)), key=lambda k: case.poly_of[k])  # the yardstick takes the cells grouped
    po, index = [case.poly_of[k] for k in order], [case.index[k] for k in order]
    ys = ys_bytes([case.rows[k] for k in order])
    bufs = [DevBuf(hip, b"".join(b.to_bytes(4, "little") for b in po)), DevBuf(hip, b"".join(i.to_bytes(8, "little") for i in index)),
            DevBuf(hip, ys), DevBuf(hip, bytes(32 * case.length * polys))]
    want = b"".join(Z.mont(coefs) for _, coefs in case.expect)
    try:
        L = K.lib()
        for what in range(5):
            ms = (ctypes.c_double * reps)()
            rc = L.kgs_bench_kzg_recover_cosets_many(plain.handle, nbits, lbits, polys, bufs[0].p, bufs[1].p, bufs[2].p,
                                                     len(index), case.length, case.length, bufs[3].p, what, reps, ms)
            assert rc == 0, (what, L.kgs_last_error().decode())
            assert len(list(ms)) == reps and all(x > 0 for x in ms) and plain.idle(), what
            if what in (0, 4):
                assert bufs[3].read() == want, what
        ms = (ctypes.c_double * reps)()
        assert L.kgs_bench_kzg_recover_cosets_many(plain.handle, nbits, lbits, polys, bufs[0].p, bufs[1].p, bufs[2].p,
                                                   len(index), case.length, case.length, bufs[3].p, 5, reps, ms) == KGS_E_ARG
    finally:
        for b in bufs:
            b.free()
