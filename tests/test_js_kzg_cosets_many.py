"""The JS export kzg_open_cosets_many (backend -> addon -> kgs_kzg_open_cosets_many) against the Python entry
point and the closed form, byte for byte: three polynomials of unequal lengths at (nbits, lbits) = (4, 2)."""
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


def test_kzg_open_cosets_many_export(tmp_path):
    K = common.load_pkg()
    ptau = common.oracle_ptau(8)
    nbits, lbits = 4, 2
    rnd = random.Random(68)
    ps = [[rnd.randrange(N.R) for _ in range(count)] for count in (16, 9, 1)]
    proofs, ev = K.kzg_open_cosets_many(ptau, [Z.mont(p) for p in ps], lbits)
    for b, p in enumerate(ps):
        assert proofs[b] == C.expected_proofs(p, nbits, lbits) and ev[b] == Z.mont(Z.evals(p, nbits))
    for b, p in enumerate(ps):
        (tmp_path / f"coefs{b}.bin").write_bytes(Z.mont(p))
    script = f"""
const fs = require('fs');
const {{ kzg_open_cosets_many }} = require('./index.js');
const load = name => new Uint8Array(fs.readFileSync('{tmp_path}/' + name));
(async () => {{
  const r = await kzg_open_cosets_many('{ptau}', [load('coefs0.bin'), load('coefs1.bin'), load('coefs2.bin')], {lbits});
  const none = await kzg_open_cosets_many('{ptau}', [], {lbits});
  const hex = a => a.map(x => Buffer.from(x).toString('hex'));
  process.stdout.write(JSON.stringify({{ proofs: hex(r.proofs), evals: hex(r.evals), none }}));
}})();
"""
    out = subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300)
    assert json.loads(out.decode()) == {"proofs": [x.hex() for x in proofs], "evals": [x.hex() for x in ev],
                                        "none": {"proofs": [], "evals": []}}
