"""The JS export kzg_open_all (backend kzgOpenAll -> addon kzgOpenAll -> kgs_kzg_open_all) against the Python
entry point, byte for byte: 2^6 points from 64 coefficients and from 40 (the domain is rounded up)."""
import json
import os
import random
import shutil
import subprocess

import pytest

import common
import g1_ntt_cases as N
import kzg_open_cases as Z

JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_kzg_open_all_export(tmp_path):
    K = common.load_pkg()
    ptau = common.oracle_ptau(8)
    rnd = random.Random(66)
    want = {}
    for count in (64, 40):
        c = [rnd.randrange(N.R) for _ in range(count)]
        (tmp_path / f"coefs_{count}.bin").write_bytes(Z.mont(c))
        proofs, ev = K.kzg_open_all(ptau, Z.mont(c))
        assert proofs == Z.expected_proofs(c, 6)
        want[f"proofs_{count}"], want[f"evals_{count}"] = proofs.hex(), ev.hex()
    script = f"""
const fs = require('fs');
const {{ kzg_open_all }} = require('./index.js');
const load = name => new Uint8Array(fs.readFileSync('{tmp_path}/' + name));
(async () => {{
  const out = {{}};
  for (const count of [64, 40]) {{
    const r = await kzg_open_all('{ptau}', load('coefs_' + count + '.bin'));
    out['proofs_' + count] = Buffer.from(r.proofs).toString('hex');
    out['evals_' + count] = Buffer.from(r.evals).toString('hex');
  }}
  process.stdout.write(JSON.stringify(out));
}})();
"""
    out = subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300)
    assert json.loads(out.decode()) == want
