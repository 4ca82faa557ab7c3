"""Batch verifier on the host path (kgs_verify_batch / kgs_g1_lincomb with ctx == NULL, device=None):
one pairing check for a batch of valid proofs, exact verdicts and a bounded number of further checks
for batches holding invalid ones, the weight derivation of include/kgs.h, and the segmented G1 linear
combination against the oracle. No GPU is touched."""
import ctypes

import pytest

import batch_cases as B
import common
from oracle import bn254 as O
from oracle import keccak as OK

PTAU = common.oracle_ptau(11)


def K():
    return common.load_pkg()


def run(items, ptau=PTAU, **kw):
    diag = {}
    return K().verify_batch(ptau, items, device=None, diag=diag, **kw), diag


def tau_g2(path=PTAU):
    buf = ctypes.create_string_buffer(128)
    assert K().lib().kgs_ptau_read_tau_g2(path.encode(), buf) == 0
    return buf.raw


def raw_refs(items):
    """kgs_proof_ref_t array of items that all reach the library"""
    k = K()
    refs = (k.ProofRef * max(len(items), 1))()
    keep = []
    for j, (kind, proof, nbits) in enumerate(items):
        npols, selected, com, ev = k._proof_buffers(kind, proof)
        cb, eb = ctypes.create_string_buffer(com, len(com)), ctypes.create_string_buffer(ev, len(ev))
        keep += [cb, eb]
        refs[j] = k.ProofRef(kind, nbits, npols, int(selected), ctypes.cast(cb, ctypes.c_void_p),
                             ctypes.cast(eb, ctypes.c_void_p))
    return refs, keep


def test_all_goldens_one_pairing_check():
    items = list(B.all_items())
    assert len(items) == 69
    got, diag = run(items)
    assert got == [True] * 69
    assert diag["pairing_checks"] == 1 and diag["on_gpu"] == 0
    assert diag["terms"] == sum(len(p["commitments"]) + 3 for _, p, _ in items)
    assert got == [B.single(K(), it, PTAU) for it in items]


@pytest.mark.parametrize("how", list(B.TAMPERS))
def test_one_bad_item(how):
    pos, structural, screened = B.TAMPERS[how]
    items = B.batch16()
    items[pos] = B.tamper(items[pos], how)
    got, diag = run(items)
    assert got == [i != pos for i in range(16)]
    assert B.single(K(), items[pos], PTAU) is False
    sent = 16 - int(screened)
    assert len(diag["indices"]) == sent
    if structural or screened:
        assert diag["pairing_checks"] == 1  # a structurally invalid item costs no pairing check
    else:
        assert 2 <= diag["pairing_checks"] <= 1 + 2 * 1 * B.log2_ceil(sent)
    if structural:
        j = diag["indices"].index(pos)
        assert diag["folded"][128 * j:128 * j + 128] == bytes(128)


def test_three_bad_items():
    items = B.batch16()
    for pos, how in ((0, "swapped_commitment"), (7, "wrong_nbits"), (15, "evaluation_plus_1")):
        items[pos] = B.tamper(items[pos], how)
    got, diag = run(items)
    assert got == [i not in (0, 7, 15) for i in range(16)]
    assert got == [B.single(K(), it, PTAU) for it in items]
    assert diag["pairing_checks"] <= min(1 + 2 * 3 * 4, 2 * 16 - 1)


def test_wrong_tau(tmp_path):
    from oracle import ptau as PT
    other = str(tmp_path / "other.ptau")
    PT.write_synthetic_ptau(other, 9, (common.tau() + 1) % O.R)
    items = B.batch16()[:8]
    got, diag = run(items, ptau=other)
    assert got == [False] * 8
    assert diag["pairing_checks"] <= 2 * 8 - 1
    assert K().verify_batch(other, items, device=None, locate=False) is False


def test_edge_calls():
    k = K()
    L = k.lib()
    items = B.batch16()
    items[4] = B.tamper(items[4], "evaluation_plus_1")
    refs, keep = raw_refs(items)
    t2 = ctypes.create_string_buffer(tau_g2(), 128)
    d = k.BatchDiag()
    # valid_out == NULL: the aggregate verdict only
    assert L.kgs_verify_batch(None, refs, 16, t2, None, ctypes.byref(d)) == 0
    assert d.pairing_checks == 1
    good, keep2 = raw_refs(B.batch16())
    assert L.kgs_verify_batch(None, good, 16, t2, None, ctypes.byref(d)) == 1
    assert d.pairing_checks == 1
    assert L.kgs_verify_batch(None, good, 16, t2, None, None) == 1  # diag is optional
    # count == 0
    assert L.kgs_verify_batch(None, None, 0, t2, None, ctypes.byref(d)) == 1
    assert d.pairing_checks == 0
    assert k.verify_batch(PTAU, [], device=None) == []
    # count == 1 agrees with kgs_verify
    for it in (items[3], items[4]):
        want = B.single(k, it, PTAU)
        assert k.verify_batch(PTAU, [it], device=None) == [want]


def weights_of(items, t2):
    """the derivation of include/kgs.h, restated"""
    k = K()
    msg = b"kgs-verify-batch-v1" + t2 + len(items).to_bytes(4, "little")
    for kind, proof, nbits in items:
        npols, selected, com, ev = k._proof_buffers(kind, proof)
        msg += b"".join(x.to_bytes(4, "little") for x in (kind, nbits, npols, int(selected))) + com + ev
    seed = OK.keccak256(msg)
    out = []
    for i in range(len(items)):
        rho = int.from_bytes(OK.keccak256(seed + i.to_bytes(4, "little"))[:16], "little")
        out.append(rho or 1)
    return out


def ints32(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def test_weights():
    items = B.batch16()
    _, diag = run(items)
    w = ints32(diag["weights"])
    assert w == weights_of(items, tau_g2())
    assert all(0 < x < 1 << 128 for x in w)
    kind, proof, nbits = items[-1]
    name = next(iter(proof["evaluations"]))
    v = bytearray(proof["evaluations"][name])
    v[0] ^= 1  # one byte of the LAST proof
    other = {"commitments": proof["commitments"], "evaluations": {**proof["evaluations"], name: bytes(v)}}
    _, diag2 = run(items[:-1] + [(kind, other, nbits)])
    w2 = ints32(diag2["weights"])
    assert all(a != b for a, b in zip(w, w2))


def test_weights_are_applied():
    items = B.batch16()
    p = items[5]
    _, alone = run([p])
    _, batch = run(items[:3] + [p] + items[6:9])
    rho1, rho3 = ints32(alone["weights"])[0], ints32(batch["weights"])[3]
    ratio = rho3 * O.fr_inv(rho1) % O.R
    for part in (0, 64):
        one = O.g1_from_lem(alone["folded"][part:part + 64])
        many = O.g1_from_lem(batch["folded"][128 * 3 + part:128 * 3 + part + 64])
        assert one is not None and many == O.g1_mul(one, ratio)


def test_determinism():
    items = B.batch16()
    items[2] = B.tamper(items[2], "swapped_commitment")
    a, b = run(items), run(items)
    assert a[0] == b[0]
    assert a[1]["folded"] == b[1]["folded"] and a[1]["weights"] == b[1]["weights"]
    assert a[1]["pairing_checks"] == b[1]["pairing_checks"]


def test_g1_lincomb_host_matches_oracle():
    points, scalars, off, segs = B.lincomb_cases()
    assert off[-1] <= 800
    got = K().g1_lincomb(points, scalars, off, device=None)
    want = B.lincomb_reference()
    assert len(got) == 64 * len(segs)
    for s in range(len(segs)):
        assert got[64 * s:64 * s + 64] == want[64 * s:64 * s + 64], (s, len(segs[s]))
    # r * P, {sP, s(-P)}, the zero point and the empty segments are the identity
    zero = [s for s in range(len(segs)) if got[64 * s:64 * s + 64] == bytes(64)]
    assert zero == [0, 4, 8, 11, 12, len(segs) - 1]


def test_g1_lincomb_argument_errors():
    k = K()
    g = O.g1_to_lem(O.G1_GEN)
    one = (1).to_bytes(32, "little")
    assert k.g1_lincomb(b"", b"", [0], device=None) == b""
    assert k.g1_lincomb(g, one, [0, 1], device=None) == g
    big_x = O.Q.to_bytes(32, "little") + bytes(32)  # a coordinate that is not < q
    for pts, off in ((O.fq_to_bytes(1) + O.fq_to_bytes(3), [0, 1]), (big_x, [0, 1]), (g, [1, 1])):
        with pytest.raises(k.KgsError) as e:
            k.g1_lincomb(pts, one, off, device=None)
        assert e.value.code == -1 and str(e.value)
    # offsets that decrease
    L = k.lib()
    rc = L.kgs_g1_lincomb(None, ctypes.create_string_buffer(g + g, 128), ctypes.create_string_buffer(one * 2, 64),
                          (ctypes.c_uint64 * 3)(0, 2, 1), 2, ctypes.create_string_buffer(128))
    assert rc == -1 and b"seg_off" in L.kgs_last_error()


def test_abi_errors():
    k = K()
    L = k.lib()
    t2 = ctypes.create_string_buffer(tau_g2(), 128)
    refs, keep = raw_refs(B.batch16()[:2])
    valid = ctypes.create_string_buffer(2)

    def fails(*args):
        assert L.kgs_verify_batch(*args) == -1
        assert L.kgs_last_error().decode()

    refs[1].kind = 7
    fails(None, refs, 2, t2, valid, None)
    refs[1].kind = 0
    refs[1].nbits = 29
    fails(None, refs, 2, t2, valid, None)
    refs[1].nbits = 3
    refs[1].npols = 0
    fails(None, refs, 2, t2, valid, None)
    refs[1].npols = 1
    com = refs[1].commitments
    refs[1].commitments = None
    fails(None, refs, 2, t2, valid, None)
    refs[1].commitments = com
    fails(None, refs, 2, None, valid, None)
    fails(None, None, 2, t2, valid, None)
    off = bytearray(t2.raw)
    off[64] ^= 1  # y.c0 changed: no longer on the twist
    fails(None, refs, 2, ctypes.create_string_buffer(bytes(off), 128), valid, None)
    assert L.kgs_verify_batch_ptau(None, b"/nonexistent.ptau", refs, 2, valid, None) == -6
