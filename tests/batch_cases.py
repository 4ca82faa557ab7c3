"""Shared inputs of test_verify_batch.py (host path) and test_gpu_verify_batch.py (GPU path): the
golden proofs as batch items, the tamper kinds of test_verifier.py, and the case list of the G1
linear combination with its pure-Python reference (computed once, never modified)."""
import functools
import json
import os
import random

import common
from oracle import bn254 as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "golden.json")))
LOOK = json.load(open(os.path.join(HERE, "golden", "lookup.json")))
KIND = {"grandsum": 0, "grandproduct": 1, "lookup": 2}


def proof_of(case):
    return {sec: {k: bytes.fromhex(v) for k, v in case["proof"][sec].items()} for sec in ("commitments", "evaluations")}


def item_of(case):
    return (KIND[case["kind"]], proof_of(case), case["nbits"])


@functools.lru_cache(None)
def all_items():
    """the 48 + 21 golden proofs: mixed kinds, k, selectors and nbits"""
    return tuple(item_of(c) for c in GOLD["cases"] + LOOK["cases"])


def single(K, item, ptau):
    kind, proof, nbits = item
    return (K.grandsum_verifier, K.grandproduct_verifier, K.lookup_verifier)[kind](ptau, proof, nbits)


def batch16():
    """16 golden proofs of mixed shapes; position 13 holds a lookup"""
    items = list(all_items()[1:61:4])
    items.insert(13, all_items()[50])
    assert len(items) == 16 and items[13][0] == 2
    return items


def _copy(proof):
    return {s: dict(v) for s, v in proof.items()}


def tamper(item, how):
    kind, proof, nbits = item
    bad = _copy(proof)
    if how == "swapped_commitment":
        name = "Q"
        g1 = O.g1_to_lem(O.G1_GEN)
        bad["commitments"][name] = g1 if proof["commitments"][name] != g1 else O.g1_to_lem(O.g1_mul(O.G1_GEN, 2))
    elif how == "evaluation_plus_1":
        name = next(iter(proof["evaluations"]))
        bad["evaluations"][name] = O.fr_to_bytes((O.fr_from_bytes(proof["evaluations"][name]) + 1) % O.R)
    elif how == "wrong_nbits":
        nbits += 1
    elif how == "off_curve":
        bad["commitments"]["Wxi"] = O.fq_to_bytes(1) + O.fq_to_bytes(3)  # (1, 3) is not on y^2 = x^3 + 3
    elif how == "evaluation_is_r":
        name = list(proof["evaluations"])[-1]
        bad["evaluations"][name] = O.R.to_bytes(32, "little")
    elif how == "missing_key":
        del bad["evaluations"][list(proof["evaluations"])[-1]]
    elif how == "lookup_without_selectors":
        assert kind == 2
        for k in ("selF", "selT"):
            del bad["commitments"][k]
    else:
        raise KeyError(how)
    return (kind, bad, nbits)


# how -> (position in batch16, structurally invalid for the library, screened before the library)
TAMPERS = {
    "swapped_commitment": (2, False, False),
    "evaluation_plus_1": (15, False, False),
    "wrong_nbits": (8, False, False),  # n = 2^5 checked as 2^6
    "off_curve": (0, True, False),
    "evaluation_is_r": (6, True, False),
    "missing_key": (11, False, True),
    "lookup_without_selectors": (13, False, True),
}


def log2_ceil(n):
    return max(n - 1, 0).bit_length()


# ------------------------------------------------------------------ g1_lincomb cases
def _points(n):
    pts, p = [], O.g1_mul(O.G1_GEN, 0x1234567)
    step = O.g1_mul(O.G1_GEN, 0xabcdef01)
    for _ in range(n):
        pts.append(p)
        p = O.g1_add(p, step)
    return pts


@functools.lru_cache(None)
def lincomb_cases():
    """-> (points_lem, scalars_std, seg_off, segments) with segments a list of [(point, scalar int)]"""
    rnd = random.Random(20260)
    pts = _points(48)
    special = [0, 1, 2, O.R - 1, O.R, O.R + 1, (1 << 256) - 1]
    segs = [[(pts[i], s)] for i, s in enumerate(special)]
    segs.append([(pts[10 + i], s) for i, s in enumerate(special)])
    s = rnd.getrandbits(256)
    segs.append([(None, s)])                                   # the zero point alone
    segs.append([(pts[3], rnd.getrandbits(256)), (None, s), (pts[4], rnd.getrandbits(256))])
    segs.append([(pts[5], s), (pts[5], s)])                    # equal summands
    segs.append([(pts[5], s), (O.g1_neg(pts[5]), s)])          # opposite summands: the identity
    segs.append([])                                            # empty
    segs.append([(pts[6], rnd.randrange(O.R)), (pts[6], rnd.randrange(O.R))])  # same point, two scalars
    for n in (1, 2, 63, 64, 65, 257):
        segs.append([(pts[rnd.randrange(48)], rnd.getrandbits(256)) for _ in range(n)])
    segs.append([])
    return _pack(segs) + (segs,)


def _pack(segs):
    points = b"".join(O.g1_to_lem(p) for seg in segs for p, _ in seg)
    scalars = b"".join(s.to_bytes(32, "little") for seg in segs for _, s in seg)
    off = [0]
    for seg in segs:
        off.append(off[-1] + len(seg))
    return points, scalars, off


@functools.lru_cache(None)
def lincomb_reference():
    """the case list's expected output from oracle.bn254 (g1_mul / g1_add), computed once"""
    out = []
    for seg in lincomb_cases()[3]:
        acc = None
        for p, s in seg:
            acc = O.g1_add(acc, O.g1_mul(p, s) if p is not None else None)
        out.append(O.g1_to_lem(acc))
    return b"".join(out)


def ragged(nseg, seed):
    """nseg segments of 0 .. 6 terms (points of the pool, random 256-bit scalars)"""
    rnd = random.Random(seed)
    pts = _points(16)
    return _pack([[(pts[rnd.randrange(16)], rnd.getrandbits(256)) for _ in range((5 * i + seed) % 7)] for i in range(nseg)])
