"""The multi-argument prover on the GPU (kgs_prove_multi / kgs_prove_multi_device; csrc/prover_multi.cpp and
the fused quotient kernel k_quotient_multi of poly.hip) against the pure-Python restatement
(multi_oracle.py), the committed vectors (golden/multi.json), the single-argument prover and the native
verifier. Every output is integer arithmetic, so every comparison is byte for byte."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import batch_cases as BC
import common
import multi_cases as MC
import multi_oracle as MO
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu
R = bn.R
E_ARG, E_NOT_WELL_CALC, E_NOT_DIVISIBLE = -1, -3, -4


@pytest.fixture(scope="module")
def K():
    return common.load_pkg()


@pytest.fixture(scope="module")
def ctx(K):
    c = K.Context(0)
    c.load_ptau(common.oracle_ptau(11))
    yield c
    c.close()


def prove(ctx, args, nbits):
    coms, evs = ctx.prove_multi(nbits, MC.native_args(args))
    return tuple(coms), tuple(evs)


# ------------------------------------------------------------------ 1. byte-exact against the restatement
# nbits 1: a 4-point coset with rot = 2; 8: more than one block; alt9 crosses QM_MAX (two launches of the
# fused kernel); gp,gp: the n-point coset; every other mix: the 2n-point coset for its grand-products too
EXACT_CASES = [(mix, b) for mix in MC.SINGLES + MC.MULTIS for b in (1, 2, 3, 5, 8)] + [("alt16", 2)]


@pytest.mark.parametrize("case", EXACT_CASES, ids=MC.case_id)
def test_byte_exact_against_the_restatement(K, ctx, case):
    mix, nbits = case
    args = MC.arguments(mix, nbits)
    got = prove(ctx, args, nbits)
    assert got == MC.restated(mix, nbits)
    if len(args) == 1:  # one argument: the single prover in exact-math mode
        a = args[0]
        ctx.set_reference_quirks(False)
        one = ctx.prove(MC.KIND[a["kind"]], nbits, a["Fs"], a["Ts"], a["selF"], a["selT"], mont_out=False)[:2]
        ctx.set_reference_quirks(True)
        assert (tuple(one[0]), tuple(one[1])) == got


def test_one_argument_reproduces_the_golden_proofs(K, ctx):
    import test_multi
    for case in BC.GOLD["cases"] + BC.LOOK["cases"]:
        a = test_multi._single_case_args(case)
        cn, en = K.proof_names(MC.KIND[case["kind"]], case["npols"], a["selF"] is not None)
        coms, evs = prove(ctx, [a], case["nbits"])
        assert {"commitments": {k: v.hex() for k, v in zip(cn, coms)},
                "evaluations": {k: v.hex() for k, v in zip(en, evs)}} == case["proof"], test_multi._single_id(case)


# ------------------------------------------------------------------ 2. the committed vectors
@pytest.mark.parametrize("case", MC.FIXTURE_CASES, ids=MC.case_id)
def test_byte_exact_against_the_fixture(ctx, case):
    mix, nbits = case
    want = MC.fixture()[case]
    args = MC.arguments(mix, nbits)
    assert MC.digest(args) == want["inputs_sha256"]
    assert [list(s) for s in MC.shapes_of(args)] == want["shapes"]
    coms, evs = prove(ctx, args, nbits)
    assert [c.hex() for c in coms] == want["commitments"]
    assert [e.hex() for e in evs] == want["evaluations"]


# ------------------------------------------------------------------ 3. device pointers
def _hip():
    """the HIP runtime the library has loaded"""
    common.load_pkg().lib()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


class DeviceArgs:
    """the arguments' buffers copied to device memory; .args are prove_multi_device's tuples"""

    def __init__(self, args):
        self.hip = _hip()
        self.ptrs = []
        self.args = [(MC.KIND[a["kind"]], [self.up(x) for x in a["Fs"]], [self.up(x) for x in a["Ts"]],
                      self.up(a["selF"]), self.up(a["selT"])) for a in args]

    def up(self, b):
        if b is None:
            return None
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), len(b)) == 0
        assert self.hip.hipMemcpy(p, bytes(b), len(b), 1) == 0  # hipMemcpyHostToDevice
        self.ptrs.append(p)
        return p.value

    def down(self, ptr, nbytes):
        out = ctypes.create_string_buffer(nbytes)
        assert self.hip.hipMemcpy(out, ctypes.c_void_p(ptr), nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out.raw

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.mark.parametrize("case", [("gs3sel,gp2,lookup,gpsel", 5), ("alt9", 8)], ids=MC.case_id)
def test_device_and_host_entry_points_agree(ctx, case):
    mix, nbits = case
    args = MC.arguments(mix, nbits)
    dev = DeviceArgs(args)
    try:
        coms, evs = ctx.prove_multi_device(nbits, dev.args)
        assert (tuple(coms), tuple(evs)) == prove(ctx, args, nbits) == MC.restated(mix, nbits)
        # the inputs are read only: no Montgomery write-back
        assert dev.down(dev.args[0][1][0], 32 << nbits) == args[0]["Fs"][0]
        assert dev.down(dev.args[-1][2][0], 32 << nbits) == args[-1]["Ts"][0]
    finally:
        dev.free()


# ------------------------------------------------------------------ 4. properties at 2^16
def test_properties_at_2p16(K):
    from test_gpu_configs import gpu_ptau, np_inputs
    from test_lookup import np_lookup_inputs
    nbits = 16
    ptau = gpu_ptau(K, nbits)
    Fs, Ts, _, _ = np_inputs(1601, nbits, 1, False)
    a0 = {"kind": "grandsum", "Fs": Fs, "Ts": Ts, "selF": None, "selT": None}
    Fs, Ts, sF, sT = np_inputs(1602, nbits, 1, True)
    a1 = {"kind": "grandproduct", "Fs": Fs, "Ts": Ts, "selF": sF, "selT": sT}
    Fs, Ts, sF, sM = np_lookup_inputs(1603, nbits, 1, 100)[:4]
    a2 = {"kind": "lookup", "Fs": Fs, "Ts": Ts, "selF": sF, "selT": sM}
    args = [a0, a1, a2]
    c = K.Context(0)
    c.load_ptau(ptau, nbits)
    try:
        proof = prove(c, args, nbits)
        assert prove(c, args, nbits) == proof  # the same bytes on every run
        t2 = ctypes.create_string_buffer(128)
        assert K.lib().kgs_ptau_read_tau_g2(os.fsencode(ptau), t2) == 0
        shapes = MC.shapes_of(args)
        assert MC.native_verify(shapes, proof, nbits, t2.raw) == 1
        bad = list(proof[1])
        bad[3] = bn.fr_to_bytes((bn.fr_from_bytes(bad[3]) + 1) % R)
        assert MC.native_verify(shapes, (proof[0], bad), nbits, t2.raw) == 0
        # round 1 is transcript-independent: the single prover's commitments on the same inputs
        at = 0
        c.set_reference_quirks(False)
        for a in args:
            one = c.prove(MC.KIND[a["kind"]], nbits, a["Fs"], a["Ts"], a["selF"], a["selT"], mont_out=False)[0]
            n1 = 2 + (2 if a["selF"] else 0)
            assert tuple(one[:n1]) == proof[0][at:at + n1], a["kind"]
            at += n1
    finally:
        c.close()


# ------------------------------------------------------------------ 5. failures
def _not_divisible(nbits, kind):
    """test_gpu_parity.py's divcheck construction: F == T under a selector that is not binary at one row"""
    Fs, _, _, _ = common.make_inputs(5, nbits, 1, False)
    sel = common.mont_bytes([2] + [1] * ((1 << nbits) - 1))
    return {"kind": kind, "Fs": Fs, "Ts": Fs, "selF": sel, "selT": sel}


@pytest.mark.parametrize("nbits", [3, 8])
def test_failures_name_the_argument_and_leave_the_context_usable(K, ctx, nbits):
    mix = "gs3sel,gp2,lookup,gpsel"
    good = list(MC.arguments(mix, nbits))
    # one changed value in argument 1's T
    t = bytearray(good[1]["Ts"][1])
    t[64:96] = ((int.from_bytes(t[64:96], "little") + 1) % R).to_bytes(32, "little")
    bad = list(good)
    bad[1] = dict(good[1], Ts=[good[1]["Ts"][0], bytes(t)])
    with pytest.raises(K.KgsError, match="^argument 1: The grand-product polynomial Z is not well calculated$") as e:
        prove(ctx, bad, nbits)
    assert e.value.code == E_NOT_WELL_CALC
    assert ctx.idle() is True
    assert prove(ctx, good, nbits) == MC.restated(mix, nbits)
    # ... and in two arguments: the lowest is named
    bad[3] = dict(good[3], Ts=[bytes(t)])
    with pytest.raises(K.KgsError, match="^argument 1: ") as e:
        prove(ctx, bad, nbits)
    assert e.value.code == E_NOT_WELL_CALC
    # a quotient numerator that Z_H does not divide, in argument 2
    for kind in ("grandsum", "grandproduct"):
        bad = list(good)
        bad[2] = _not_divisible(nbits, kind)
        with pytest.raises(K.KgsError, match="^argument 2: Polynomial is not divisible$") as e:
            prove(ctx, bad, nbits)
        assert e.value.code == E_NOT_DIVISIBLE
        assert ctx.idle() is True
        assert prove(ctx, good, nbits) == MC.restated(mix, nbits)
        with pytest.raises(ValueError, match="^argument 2: Polynomial is not divisible$"):
            MO.prove_multi(MC.srs(), bad)


# ------------------------------------------------------------------ 5b. one round engine, two entry points
# (csrc/prover_rounds.cpp: the single and the multi prover share the rounds, the work buffers and the flag words)
def _single(ctx, a, nbits):
    coms, evs = ctx.prove(MC.KIND[a["kind"]], nbits, a["Fs"], a["Ts"], a["selF"], a["selT"], mont_out=False)[:2]
    return tuple(coms), tuple(evs)


def _builder_fails(nbits):
    """argument 1 of the mix of test_failures_name_the_argument_and_leave_the_context_usable with that test's
    one changed value in its T: a grand-product (k = 2) whose Z is not well calculated"""
    a = MC.arguments("gs3sel,gp2,lookup,gpsel", nbits)[1]
    t = bytearray(a["Ts"][1])
    t[64:96] = ((int.from_bytes(t[64:96], "little") + 1) % R).to_bytes(32, "little")
    return dict(a, Ts=[a["Ts"][0], bytes(t)])


@pytest.mark.parametrize("case", [("gs3sel,gp2,lookup,gpsel", 5), ("alt9", 3), ("gp,gp", 1)], ids=MC.case_id)
def test_one_lane_equals_two_lanes(ctx, case):
    mix, nbits = case
    args = MC.arguments(mix, nbits)
    try:
        ctx.set_msm_lanes(1)
        one = prove(ctx, args, nbits)
        ctx.set_msm_lanes(2)
        two = prove(ctx, args, nbits)
    finally:
        ctx.set_msm_lanes(2)
    assert one == MC.restated(mix, nbits)
    assert two == MC.restated(mix, nbits)


def test_both_entry_points_interleaved_on_one_context(K, ctx):
    mix, mbits = "gs3sel,gp2,lookup,gpsel", 5
    margs = MC.arguments(mix, mbits)
    Fs, Ts, sF, sT = common.make_inputs(77, 8, 1, True)
    sarg = {"kind": "grandproduct", "Fs": Fs, "Ts": Ts, "selF": sF, "selT": sT}
    single1 = _single(ctx, sarg, 8)
    multi1 = prove(ctx, margs, mbits)
    assert multi1 == MC.restated(mix, mbits)
    with pytest.raises(K.KgsError, match="^The grand-product polynomial Z is not well calculated$") as e:
        _single(ctx, _builder_fails(mbits), mbits)
    assert e.value.code == E_NOT_WELL_CALC
    assert prove(ctx, margs, mbits) == multi1
    assert _single(ctx, sarg, 8) == single1


def test_only_the_multi_entry_point_names_the_argument(K, ctx):
    nbits = 5
    bad = _builder_fails(nbits)
    with pytest.raises(K.KgsError, match="^argument 0: The grand-product polynomial Z is not well calculated$") as em:
        prove(ctx, [bad], nbits)
    with pytest.raises(K.KgsError, match="^The grand-product polynomial Z is not well calculated$") as es:
        _single(ctx, bad, nbits)
    assert em.value.code == es.value.code == E_NOT_WELL_CALC
    assert ctx.idle() is True


def test_argument_errors(K, ctx):
    nbits = 3
    good = MC.native_args(MC.arguments("gs,gp,lookup", nbits))

    def code(args, nb=nbits, c=ctx):
        with pytest.raises(K.KgsError) as e:
            c.prove_multi(nb, args)
        return e.value.code, str(e.value)
    assert code([])[0] == E_ARG
    assert code([good[0]] * 17)[0] == E_ARG
    assert code([good[0], (3,) + good[1][1:]]) == (E_ARG, "argument 1: unknown argument kind")
    assert code([good[0], (0, [], [], None, None)]) == (E_ARG, "argument 1: The number of multisets must be greater than 0.")
    rc, msg = code(good[:2] + [(2,) + good[2][1:3] + (None, None)])  # a lookup without selectors
    assert rc == E_ARG and msg.startswith("argument 2: ")
    big = MC.native_args(MC.arguments("gs", 8))
    from test_gpu_configs import private_copy
    small = K.Context(0)
    small.load_ptau(private_copy(common.oracle_ptau(9)), 5)  # its own file: an SRS for domains up to 2^5 only
    assert code(big, 8, small)[0] == E_ARG
    small.close()
    small = K.Context(0)
    small.load_ptau(common.oracle_ptau(3))
    assert code(big, 8, small) == (-7, "The Powers of Tau file is not sufficiently large to commit the polynomials.")
    small.close()
    assert ctx.idle() is True
    # a context with MSM point-range sharding switched on
    c = K.Context(0)
    c.load_ptau(common.oracle_ptau(11), nbits)
    c.set_shard(0, 2, lambda data: data * 2)
    rc, msg = code(good, nbits, c)
    assert rc == E_ARG and "kgs_ctx_set_shard" in msg
    c.set_shard(0, 1)
    assert prove(c, MC.arguments("gs,gp,lookup", nbits), nbits) == MC.restated("gs,gp,lookup", nbits)
    c.close()
    # a context attached to a rank group
    g = K.Group.local(1)
    c = K.Context(0)
    c.load_ptau(common.oracle_ptau(11), nbits)
    c.set_group(g, 0)
    rc, msg = code(good, nbits, c)
    assert rc == E_ARG and "rank group" in msg
    c.set_group(None)
    c.close()
    g.close()


# ------------------------------------------------------------------ 6. tampering
def test_tampered_gpu_proof_is_rejected(ctx):
    mix, nbits = "alt9", 5
    args = MC.arguments(mix, nbits)
    shapes = MC.shapes_of(args)
    coms, evs = prove(ctx, args, nbits)
    assert MC.native_verify(shapes, (coms, evs), nbits) == 1
    assert MO.verify_multi(shapes, (coms, evs), nbits, common.tau()) is True
    for i in (0, len(coms) // 2, len(coms) - 4, len(coms) - 3, len(coms) - 1):
        bad = list(coms)
        bad[i] = bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, 5))
        assert MC.native_verify(shapes, (bad, evs), nbits) == 0, i
    for i in (0, len(evs) // 2, len(evs) - 1):
        bad = list(evs)
        bad[i] = bn.fr_to_bytes((bn.fr_from_bytes(evs[i]) + 1) % R)
        assert MC.native_verify(shapes, (coms, bad), nbits) == 0, i


def test_python_drop_in(K):
    """multi_prover / multi_verifier on Evaluations, with the dict names"""
    mix, nbits = "gs,gp,lookup", 5
    args = MC.arguments(mix, nbits)
    ptau = common.oracle_ptau(11)
    call = [{"kind": MC.KIND[a["kind"]], "evalsFs": [K.Evaluations(x) for x in a["Fs"]],
             "evalsTs": [K.Evaluations(x) for x in a["Ts"]],
             "evalsSelF": K.Evaluations(a["selF"]) if a["selF"] else None,
             "evalsSelT": K.Evaluations(a["selT"]) if a["selT"] else None} for a in args]
    proof = K.multi_prover(ptau, call)
    sh = MC.native_shapes(MC.shapes_of(args))
    cn, en = K.proof_names_multi(sh)
    coms, evs = MC.restated(mix, nbits)
    assert proof == {"commitments": dict(zip(cn, coms)), "evaluations": dict(zip(en, evs))}
    assert list(proof["commitments"]) == cn and list(proof["evaluations"]) == en
    assert call[0]["evalsFs"][0].eval == args[0]["Fs"][0]  # left in standard form
    assert K.multi_verifier(ptau, proof, nbits, sh) is True
    # one argument: today's names and today's proof
    Fs, Ts, _, _ = common.make_inputs(BC.GOLD["cases"][3]["seed"], BC.GOLD["cases"][3]["nbits"], 1, False)
    one = K.multi_prover(ptau, [(K.GRANDSUM, K.Evaluations(Fs[0]), K.Evaluations(Ts[0]))])
    assert {s: {k: v.hex() for k, v in one[s].items()} for s in one} == BC.GOLD["cases"][3]["proof"]
    with pytest.raises(ValueError, match="^argument 1: The 0-th multiset buffers must have the same length.$"):
        K.multi_prover(ptau, [call[0], (K.GRANDSUM, K.Evaluations(Fs[0]), K.Evaluations(Ts[0][:64]))])
    Fs, Ts, _, _ = common.make_inputs(1, 3, 1, False)
    with pytest.raises(ValueError, match="^argument 1: every argument must have the domain of argument 0.$"):
        K.multi_prover(ptau, [call[0], (K.GRANDSUM, K.Evaluations(Fs[0]), K.Evaluations(Ts[0]))])


# ------------------------------------------------------------------ 7. JavaScript
JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
_HAVE_NODE = shutil.which("node") is not None and os.path.exists(os.path.join(JS, "build", "kgs_addon.node"))


def _js_names(K, shapes):
    return K.proof_names_multi(MC.native_shapes(shapes))


@pytest.mark.skipif(not _HAVE_NODE, reason="node or the N-API addon is missing")
def test_js_multi_prover_and_verifier(K, tmp_path):
    """mset_eq_kzg_multi_prover / _verifier through N-API on [gs, lookup] at nbits 5: byte-exact against
    the restatement, the names and their order, the verifier's verdicts, and a failing argument's message."""
    mix, nbits = "gs,lookup", 5
    args = MC.arguments(mix, nbits)
    shapes = MC.shapes_of(args)
    cn, en = _js_names(K, shapes)
    coms, evs = MC.restated(mix, nbits)

    def js_arg(a):
        return {"kind": a["kind"], "F": [x.hex() for x in a["Fs"]], "T": [x.hex() for x in a["Ts"]],
                "selF": a["selF"].hex() if a["selF"] else None, "selT": a["selT"].hex() if a["selT"] else None}
    js_shapes = [{"kind": k, "npols": p, "selected": s} for k, p, s in shapes]
    good = {"op": "verify", "shapes": js_shapes, "commitments": {k: v.hex() for k, v in zip(cn, coms)},
            "evaluations": {k: v.hex() for k, v in zip(en, evs)}}
    bad = json.loads(json.dumps(good))
    bad["evaluations"]["A1.sxiw"] = bn.fr_to_bytes((bn.fr_from_bytes(evs[-1]) + 1) % R).hex()
    broken = [js_arg(args[0]), js_arg(dict(args[1], Ts=args[0]["Ts"]))]  # the lookup's table replaced
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"ptau": common.oracle_ptau(11), "nbits": nbits, "cases": [
        {"op": "prove", "args": [js_arg(a) for a in args]}, good, bad, {"op": "prove", "args": broken},
        {"op": "prove", "args": [js_arg(args[0])]}]}))
    out = subprocess.run(["node", os.path.join(JS, "test", "multi_from_json.js"), str(spec)], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)["results"]
    assert list(res[0]["commitments"]) == cn and list(res[0]["evaluations"]) == en
    assert res[0]["commitments"] == good["commitments"] and res[0]["evaluations"] == good["evaluations"]
    assert res[0]["verified"] is True
    assert res[0]["F0"] == args[0]["Fs"][0].hex()
    assert res[1] == {"verdict": True} and res[2] == {"verdict": False}
    assert res[3] == {"error": "argument 1: The grand-sum polynomial S is not well calculated", "kgsCode": -3}
    # one argument: the single prover's names and proof
    cn1, en1 = _js_names(K, shapes[:1])
    assert list(res[4]["commitments"]) == cn1 == ["F", "T", "S", "Q", "Wxi", "Wxiw"]
    c1, e1 = MO.prove_multi(MC.srs(), [args[0]])
    assert res[4]["commitments"] == {k: v.hex() for k, v in zip(cn1, c1)}
    assert res[4]["evaluations"] == {k: v.hex() for k, v in zip(en1, e1)}
