"""Shared cases of test_multi.py (host) and test_gpu_multi.py (GPU): the argument mixes of the
multi-argument prover, their inputs (common.make_inputs / make_lookup_inputs, a distinct seed per
argument), the restated proofs (multi_oracle, computed once per case and never modified) and the
conversions between the restatement's and the package's calling conventions."""
import ctypes
import functools
import hashlib
import json
import os

import common
import multi_oracle as MO
from oracle import protocol as P

HERE = os.path.dirname(os.path.abspath(__file__))
KIND = MO.KINDS
MULTI_JSON = os.path.join(HERE, "golden", "multi.json")


def gs(seed, nbits, k=1, sel=False):
    Fs, Ts, sF, sT = common.make_inputs(seed, nbits, k, sel)
    return {"kind": "grandsum", "Fs": Fs, "Ts": Ts, "selF": sF, "selT": sT}


def gp(seed, nbits, k=1, sel=False):
    return dict(gs(seed, nbits, k, sel), kind="grandproduct")


def lk(seed, nbits, k=1, unselected=1):
    Fs, Ts, sF, sM = common.make_lookup_inputs(seed, nbits, k, min(unselected, (1 << nbits) - 1))
    return {"kind": "lookup", "Fs": Fs, "Ts": Ts, "selF": sF, "selT": sM}


# name -> nbits -> arguments; seeds are distinct per argument and depend on the size
MIXES = {
    "gs": lambda b: [gs(7100 + b, b)],
    "gs-k2-sel": lambda b: [gs(7110 + b, b, 2, True)],
    "gp": lambda b: [gp(7120 + b, b)],
    "gp-sel": lambda b: [gp(7130 + b, b, 1, True)],
    "lookup": lambda b: [lk(7140 + b, b)],
    "gs,lookup": lambda b: [gs(7150 + b, b), lk(7160 + b, b)],
    "gs,gs": lambda b: [gs(7200 + b, b), gs(7210 + b, b)],
    "gp,gp": lambda b: [gp(7220 + b, b), gp(7230 + b, b)],
    "gs,gp,lookup": lambda b: [gs(7240 + b, b), gp(7250 + b, b), lk(7260 + b, b)],
    "gs3sel,gp2,lookup,gpsel": lambda b: [gs(7270 + b, b, 3, True), gp(7280 + b, b, 2), lk(7290 + b, b, 2),
                                          gp(7300 + b, b, 1, True)],
    "alt9": lambda b: [(gs, gp, lk)[j % 3](7400 + 10 * j + b, b) for j in range(9)],
    "alt16": lambda b: [(gs, gp, lk)[j % 3](7600 + 10 * j + b, b) for j in range(16)],
}
SINGLES = ["gs", "gs-k2-sel", "gp", "gp-sel", "lookup"]
MULTIS = ["gs,gs", "gp,gp", "gs,gp,lookup", "gs3sel,gp2,lookup,gpsel", "alt9"]
# (mix, nbits) of the issue's acceptance list: every mix at 1, 2, 3, 5; 16 arguments at nbits 2 only
CPU_CASES = [(mix, b) for mix in MULTIS for b in (1, 2, 3, 5)] + [("alt16", 2)]
FIXTURE_CASES = [(mix, b) for mix in ("gs,gp,lookup", "gs3sel,gp2,lookup,gpsel") for b in (8, 11)]


def case_id(c):
    return f"{c[0]}-n{c[1]}"


@functools.lru_cache(None)
def srs():
    return P.SRS(common.oracle_ptau(11), common.tau())


@functools.lru_cache(None)
def arguments(mix, nbits):
    return tuple(MIXES[mix](nbits))


def shapes_of(args):
    return [MO.shape_of(a) for a in args]


@functools.lru_cache(None)
def restated(mix, nbits):
    """(commitments, evaluations) of the restated honest prover"""
    coms, evs = MO.prove_multi(srs(), list(arguments(mix, nbits)))
    return tuple(coms), tuple(evs)


def digest(args):
    h = hashlib.sha256()
    for a in args:
        h.update(a["kind"].encode())
        h.update(bytes.fromhex(common.inputs_digest(a["Fs"], a["Ts"], a["selF"], a["selT"])))
    return h.hexdigest()


@functools.lru_cache(None)
def fixture():
    return {(c["mix"], c["nbits"]): c for c in json.load(open(MULTI_JSON))["cases"]}


# ------------------------------------------------------------------ the package's conventions
def native_shapes(shapes):
    return [(KIND[kind], k, sel) for kind, k, sel in shapes]


def native_args(args):
    """Context.prove_multi's tuples"""
    return [(KIND[a["kind"]], a["Fs"], a["Ts"], a["selF"], a["selT"]) for a in args]


@functools.lru_cache(None)
def tau_g2():
    K = common.load_pkg()
    out = ctypes.create_string_buffer(128)
    assert K.lib().kgs_ptau_read_tau_g2(os.fsencode(common.oracle_ptau(11)), out) == 0
    return out.raw


def native_verify(shapes, proof, nbits, tau2=None):
    """kgs_verify_multi on (commitments, evaluations) lists; returns the raw code"""
    K = common.load_pkg()
    sh = native_shapes(shapes)
    arr = (K.ArgShape * max(len(sh), 1))(*[K.ArgShape(k, p, 1 if s else 0) for k, p, s in sh])
    com, ev = b"".join(proof[0]), b"".join(proof[1])
    return K.lib().kgs_verify_multi(nbits, arr, len(sh), K._buf(com), K._buf(ev), K._buf(tau2 or tau_g2()))
