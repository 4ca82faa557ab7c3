"""Batch verifier with the G1 fold on the GPU (kgs_verify_batch / kgs_g1_lincomb on a context): byte
parity with the host path (which test_verify_batch.py checks against the oracle), the context contract
(idle on return, no rank group, SRS and prover untouched), and the JavaScript module."""
import json
import os
import shutil
import subprocess

import pytest

import batch_cases as B
import common
from oracle import bn254 as O

pytestmark = pytest.mark.gpu
PTAU = common.oracle_ptau(11)
JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")


@pytest.fixture(scope="module")
def ctx():
    K = common.load_pkg()
    c = K.Context(0)
    yield c
    c.close()


@pytest.fixture()
def force_gpu(monkeypatch):
    monkeypatch.setenv("KGS_VERIFY_BATCH_FOLD", "gpu")


def host(items, **kw):
    diag = {}
    return common.load_pkg().verify_batch(PTAU, items, device=None, diag=diag, **kw), diag


def gpu(ctx, items, **kw):
    diag = {}
    return ctx.verify_batch(items, ptau=PTAU, diag=diag, **kw), diag


def test_lincomb_case_list_matches_host(ctx):
    K = common.load_pkg()
    points, scalars, off, segs = B.lincomb_cases()
    got = ctx.g1_lincomb(points, scalars, off)
    assert got == K.g1_lincomb(points, scalars, off, device=None)
    assert got == B.lincomb_reference()


@pytest.mark.parametrize("nseg", [1, 300])
def test_lincomb_ragged_segments(ctx, nseg):
    """more segments than a block and a wave hold, segment lengths 0 .. 6"""
    K = common.load_pkg()
    points, scalars, off = B.ragged(nseg, 3)
    assert len(set(b - a for a, b in zip(off, off[1:]))) == min(nseg, 7)
    assert ctx.g1_lincomb(points, scalars, off) == K.g1_lincomb(points, scalars, off, device=None)


def same(a, b):
    assert a[0] == b[0]
    for k in ("indices", "weights", "folded", "pairing_checks", "terms"):
        assert a[1][k] == b[1][k], k


def test_all_goldens_match_host(ctx, force_gpu):
    items = list(B.all_items())
    g = gpu(ctx, items)
    assert g[0] == [True] * 69 and g[1]["on_gpu"] == 1 and g[1]["pairing_checks"] == 1
    same(g, host(items))


@pytest.mark.parametrize("how", list(B.TAMPERS) + ["three"])
def test_bad_items_match_host(ctx, force_gpu, how):
    items = B.batch16()
    if how == "three":
        bad = {0: "swapped_commitment", 7: "wrong_nbits", 15: "evaluation_plus_1"}
    else:
        bad = {B.TAMPERS[how][0]: how}
    for pos, h in bad.items():
        items[pos] = B.tamper(items[pos], h)
    g = gpu(ctx, items)
    assert g[0] == [i not in bad for i in range(16)] and g[1]["on_gpu"] == 1
    same(g, host(items))


def test_host_override_on_a_context(ctx, monkeypatch):
    monkeypatch.setenv("KGS_VERIFY_BATCH_FOLD", "host")
    g = gpu(ctx, B.batch16())
    assert g[0] == [True] * 16 and g[1]["on_gpu"] == 0


def test_default_routing_by_batch_size(ctx, monkeypatch):
    """without the override a context folds a single proof on the host (faster there) and the 69
    goldens on the GPU; the bytes are the same either way"""
    monkeypatch.delenv("KGS_VERIFY_BATCH_FOLD", raising=False)
    one = gpu(ctx, [B.batch16()[5]])
    assert one[0] == [True] and one[1]["on_gpu"] == 0
    many = gpu(ctx, list(B.all_items()))
    assert many[0] == [True] * 69 and many[1]["on_gpu"] == 1
    same(many, host(list(B.all_items())))


def test_idle_after_success_and_after_an_argument_error(ctx, force_gpu):
    K = common.load_pkg()
    assert ctx.verify_batch(B.batch16()[:4], ptau=PTAU) == [True] * 4
    assert ctx.idle() is True
    kind, proof, nbits = B.batch16()[0]
    with pytest.raises(K.KgsError) as e:
        ctx.verify_batch([B.batch16()[1], (kind, proof, 29)], ptau=PTAU)
    assert e.value.code == -1
    assert ctx.idle() is True
    with pytest.raises(K.KgsError) as e:
        ctx.g1_lincomb(O.fq_to_bytes(1) + O.fq_to_bytes(3), bytes(32), [0, 1])
    assert e.value.code == -1
    assert ctx.idle() is True


def test_rank_group_context_is_refused():
    K = common.load_pkg()
    g = K.Group.local(1)
    c = K.Context(0)
    c.set_group(g, 0)
    with pytest.raises(K.KgsError, match="rank group") as e:
        c.verify_batch(B.batch16()[:2], ptau=PTAU)
    assert e.value.code == -1
    with pytest.raises(K.KgsError, match="rank group") as e:
        c.g1_lincomb(O.g1_to_lem(O.G1_GEN), (1).to_bytes(32, "little"), [0, 1])
    assert e.value.code == -1
    c.set_group(None)
    c.close()
    g.close()


def test_prover_and_srs_untouched(force_gpu):
    """prove, verify a batch on the same context, prove again: the same golden bytes, the same SRS"""
    K = common.load_pkg()
    case = next(c for c in B.GOLD["cases"]
                if (c["kind"], c["npols"], c["selected"], c["nbits"]) == ("grandsum", 3, True, 5))
    c = K.Context(0)
    c.load_ptau(PTAU)

    def prove():
        Fs, Ts, sF, sT = common.make_inputs(case["seed"], 5, 3, True)
        com, ev = c.prove(K.GRANDSUM, 5, Fs, Ts, sF, sT, mont_out=False)[:2]
        cn, en = K.proof_names(K.GRANDSUM, 3, True)
        return ({n: bytes(com[i]).hex() for i, n in enumerate(cn)}, {n: bytes(ev[i]).hex() for i, n in enumerate(en)})

    want = (case["proof"]["commitments"], case["proof"]["evaluations"])
    assert prove() == want
    info = c.srs_info()
    diag = {}
    assert c.verify_batch(B.batch16(), ptau=PTAU, diag=diag) == [True] * 16 and diag["on_gpu"] == 1
    assert c.srs_info() == info
    assert prove() == want
    c.close()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(JS, "build", "kgs_addon.node")),
                    reason="node or the N-API addon is missing")
def test_js_kzg_verifier_batch(tmp_path):
    cases = []
    for c in B.GOLD["cases"][::3]:
        cases.append({"kind": c["kind"], "nbits": c["nbits"], **c["proof"]})
        bad = json.loads(json.dumps(c["proof"]))
        k = next(iter(bad["evaluations"]))
        x = O.fr_from_bytes(bytes.fromhex(bad["evaluations"][k]))
        bad["evaluations"][k] = O.fr_to_bytes((x + 5) % O.R).hex()
        cases.append({"kind": c["kind"], "nbits": c["nbits"], **bad})
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"ptau": PTAU, "cases": cases}))
    out = subprocess.run(["node", os.path.join(JS, "test", "verify_batch_from_json.js"), str(spec)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["verdicts"] == [True, False] * (len(cases) // 2)
