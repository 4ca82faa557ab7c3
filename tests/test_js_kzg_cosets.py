"""The JS exports kzg_open_cosets and kzg_verify_coset (backend -> addon -> kgs_kzg_open_cosets /
kgs_kzg_verify_coset) against the Python entry point and the closed form, byte for byte: one (nbits, lbits) =
(4, 2) case, every one of its 4 proofs accepted, and rejected with a value changed."""
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


def test_kzg_open_cosets_export(tmp_path):
    K = common.load_pkg()
    ptau = common.oracle_ptau(8)
    nbits, lbits = 4, 2
    n, l, m = C.sizes(nbits, lbits)
    rnd = random.Random(67)
    c = [rnd.randrange(N.R) for _ in range(n)]
    proofs, ev = K.kzg_open_cosets(ptau, Z.mont(c), lbits)
    assert proofs == C.expected_proofs(c, nbits, lbits) and ev == Z.mont(Z.evals(c, nbits))
    (tmp_path / "coefs.bin").write_bytes(Z.mont(c))
    (tmp_path / "commit.bin").write_bytes(Z.commitment(c))
    (tmp_path / "srs.bin").write_bytes(C.srs_g1(lbits))
    (tmp_path / "tau_l_g2.bin").write_bytes(C.tau_l_g2(lbits))
    script = f"""
const fs = require('fs');
const {{ kzg_open_cosets, kzg_verify_coset }} = require('./index.js');
const load = name => new Uint8Array(fs.readFileSync('{tmp_path}/' + name));
(async () => {{
  const r = await kzg_open_cosets('{ptau}', load('coefs.bin'), {lbits});
  const commit = load('commit.bin'), srs = load('srs.bin'), t2 = load('tau_l_g2.bin');
  const ok = [], bad = [];
  for (let i = 0; i < {m}; i++) {{
    const ys = new Uint8Array({32 * l});
    for (let j = 0; j < {l}; j++) ys.set(r.evals.subarray(32 * (i + {m} * j), 32 * (i + {m} * j) + 32), 32 * j);
    const proof = r.proofs.subarray(64 * i, 64 * i + 64);
    ok.push(kzg_verify_coset(commit, {nbits}, {lbits}, i, ys, proof, srs, t2));
    ys[32] ^= 1;
    bad.push(kzg_verify_coset(commit, {nbits}, {lbits}, i, ys, proof, srs, t2));
  }}
  process.stdout.write(JSON.stringify({{ proofs: Buffer.from(r.proofs).toString('hex'),
                                         evals: Buffer.from(r.evals).toString('hex'), ok, bad }}));
}})();
"""
    out = subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300)
    assert json.loads(out.decode()) == {"proofs": proofs.hex(), "evals": ev.hex(), "ok": [True] * m, "bad": [False] * m}
