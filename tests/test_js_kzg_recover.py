"""The JS export kzg_recover_cosets (backend -> addon -> kgs_kzg_recover_cosets) against the integer references at
(nbits, lbits) = (5, 2): a shuffled random half of the cosets, the 0 verdict for a tampered value, one refusal."""
import json
import os
import shutil
import subprocess

import pytest

import common
import kzg_open_cases as Z
import kzg_recover_cases as C

JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_kzg_recover_cosets_export(tmp_path):
    nbits, lbits = 5, 2
    n, l, m = C.sizes(nbits, lbits)
    index, rows, length, coefs = C.make_case(515, nbits, lbits, "shuffled", "odd")
    assert len(index) * l > length and C.steps(index, rows, nbits, lbits, length) == (1, coefs)
    (tmp_path / "ys.bin").write_bytes(Z.mont(C.flat(rows)))
    script = f"""
const fs = require('fs');
const {{ kzg_recover_cosets }} = require('./index.js');
(async () => {{
  const ys = new Uint8Array(fs.readFileSync('{tmp_path}/ys.bin'));
  const index = {json.dumps(index)};
  const cells = index.map((i, k) => ({{ index: i, ys: ys.slice({32 * l} * k, {32 * l} * (k + 1)) }}));
  const hex = b => Buffer.from(b).toString('hex');
  const good = await kzg_recover_cosets({nbits}, {lbits}, cells, {length});
  const bad = cells.map(c => ({{ index: c.index, ys: c.ys.slice() }}));
  bad[1].ys[3] ^= 1;
  const tampered = await kzg_recover_cosets({nbits}, {lbits}, bad, {length});
  let refusal = null;
  try {{
    await kzg_recover_cosets({nbits}, {lbits}, cells.concat([cells[0]]), {length});
  }} catch (e) {{
    refusal = {{ code: e.kgsCode, message: e.message }};
  }}
  const again = await kzg_recover_cosets({nbits}, {lbits}, cells, {length});
  process.stdout.write(JSON.stringify({{ ok: good.ok, coefs: hex(good.coefs), evals: hex(good.evals),
    tampered: tampered.ok, refusal, again: again.ok && hex(again.coefs) === hex(good.coefs) }}));
}})();
"""
    out = json.loads(subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300).decode())
    assert out["ok"] is True and bytes.fromhex(out["coefs"]) == Z.mont(coefs)
    assert bytes.fromhex(out["evals"]) == Z.mont(C.evals(coefs, nbits))
    assert out["tampered"] is False
    assert out["refusal"]["code"] == -1 and f"index[{len(index)}]" in out["refusal"]["message"]
    assert out["again"] is True
