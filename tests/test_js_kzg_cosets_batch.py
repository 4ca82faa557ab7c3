"""The JS export kzg_verify_cosets_batch (backend -> addon -> kgs_kzg_verify_cosets_batch) against the Python entry
point: the 8 coset openings of two polynomials at (nbits, lbits) = (4, 2) made by the JS kzg_open_cosets, one valid
batch and one with a proof exchanged, on the GPU path and on the host path."""
import json
import os
import random
import shutil
import subprocess

import pytest

import common
import g1_ntt_cases as N
import kzg_coset_cases as C
import kzg_open_cases as Z

JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_kzg_verify_cosets_batch_export(tmp_path):
    K = common.load_pkg()
    ptau = common.oracle_ptau(8)
    nbits, lbits = 4, 2
    n, l, m = C.sizes(nbits, lbits)
    rnd = random.Random(68)
    polys = [[rnd.randrange(N.R) for _ in range(n)] for _ in range(2)]
    for p, c in enumerate(polys):
        (tmp_path / f"coefs{p}.bin").write_bytes(Z.mont(c))
        (tmp_path / f"commit{p}.bin").write_bytes(Z.commitment(c))
    (tmp_path / "srs.bin").write_bytes(C.srs_g1(lbits))
    (tmp_path / "tau_l_g2.bin").write_bytes(C.tau_l_g2(lbits))
    script = f"""
const fs = require('fs');
const {{ kzg_open_cosets, kzg_verify_cosets_batch }} = require('./index.js');
const load = name => new Uint8Array(fs.readFileSync('{tmp_path}/' + name));
(async () => {{
  process.env.KGS_VERIFY_COSETS_FOLD = 'gpu';
  const commits = [load('commit0.bin'), load('commit1.bin')], srs = load('srs.bin'), t2 = load('tau_l_g2.bin');
  const openings = [];
  for (let p = 0; p < 2; p++) {{
    const r = await kzg_open_cosets('{ptau}', load('coefs' + p + '.bin'), {lbits});
    for (let i = 0; i < {m}; i++) {{
      const ys = new Uint8Array({32 * l});
      for (let j = 0; j < {l}; j++) ys.set(r.evals.subarray(32 * (i + {m} * j), 32 * (i + {m} * j) + 32), 32 * j);
      openings.push({{ commit: p, index: i, ys, proof: r.proofs.slice(64 * i, 64 * i + 64) }});
    }}
  }}
  const good = await kzg_verify_cosets_batch(commits, {nbits}, {lbits}, openings, srs, t2);
  const bad = openings.map(o => Object.assign({{}}, o));
  bad[5].proof = openings[6].proof;
  bad[2].ys = bad[2].ys.slice(32);
  const tampered = await kzg_verify_cosets_batch(commits, {nbits}, {lbits}, bad, srs, t2);
  const host = await kzg_verify_cosets_batch(commits, {nbits}, {lbits}, bad, srs, t2, {{ host: true }});
  process.stdout.write(JSON.stringify({{ good: good.valid, goodGpu: good.onGpu, checks: good.pairingChecks,
    tampered: tampered.valid, tamperedGpu: tampered.onGpu, host: host.valid, hostGpu: host.onGpu,
    sameChecks: host.pairingChecks === tampered.pairingChecks,
    ys: openings.map(o => Buffer.from(o.ys).toString('hex')), proofs: openings.map(o => Buffer.from(o.proof).toString('hex')) }}));
}})();
"""
    out = json.loads(subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300).decode())
    want = [k not in (2, 5) for k in range(2 * m)]
    assert out["good"] == [True] * (2 * m) and out["goodGpu"] is True and out["checks"] == 1
    assert out["tampered"] == want and out["tamperedGpu"] is True
    assert out["host"] == want and out["hostGpu"] is False and out["sameChecks"] is True
    # the Python entry point on the openings the JS module made
    tuples = [(k // m, k % m, bytes.fromhex(out["ys"][k]), bytes.fromhex(out["proofs"][k])) for k in range(2 * m)]
    commits = [Z.commitment(c) for c in polys]
    assert K.kzg_verify_cosets_batch(C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits, tuples,
                                     device=None) == [True] * (2 * m)
    tuples[5] = tuples[5][:3] + (tuples[6][3],)
    assert K.kzg_verify_cosets_batch(C.tau_l_g2(lbits), C.srs_g1(lbits), nbits, lbits, commits, tuples,
                                     device=None) == [k != 5 for k in range(2 * m)]
