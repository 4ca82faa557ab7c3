"""The JS export kzg_recover_cosets_many (backend -> addon -> kgs_kzg_recover_cosets_many) against the Python call and
the integer references at (nbits, lbits) = (5, 2): a call with every status, one refusal, and a valid call after it."""
import json
import os
import shutil
import subprocess

import pytest

import common
import kzg_open_cases as Z
import kzg_recover_cases as C
import kzg_recover_many_cases as M

JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_kzg_recover_cosets_many_export(tmp_path):
    nbits, lbits = 5, 2
    n, l, m = C.sizes(nbits, lbits)
    case = M.make_statuses(616, nbits, lbits)
    ys = Z.mont(C.flat(case.rows))
    K = common.load_pkg()
    status, coefs, evals = K.kzg_recover_cosets_many(nbits, lbits, case.poly_of, case.index, ys, case.length, case.polys,
                                                     evals=True)
    assert status == case.status() == [1, 0, 1, 2, 2, 1]
    (tmp_path / "ys.bin").write_bytes(ys)
    script = f"""
const fs = require('fs');
const {{ kzg_recover_cosets_many }} = require('./index.js');
(async () => {{
  const ys = new Uint8Array(fs.readFileSync('{tmp_path}/ys.bin'));
  const polyOf = {json.dumps(case.poly_of)};
  const index = {json.dumps(case.index)};
  const cells = index.map((i, k) => ({{ poly: polyOf[k], index: i, ys: ys.slice({32 * l} * k, {32 * l} * (k + 1)) }}));
  const hex = b => Buffer.from(b).toString('hex');
  const got = await kzg_recover_cosets_many({nbits}, {lbits}, cells, {case.length}, {case.polys});
  let refusal = null;
  try {{
    await kzg_recover_cosets_many({nbits}, {lbits}, cells.concat([cells[0]]), {case.length}, {case.polys});
  }} catch (e) {{
    refusal = {{ code: e.kgsCode, message: e.message }};
  }}
  const again = await kzg_recover_cosets_many({nbits}, {lbits}, cells, {case.length}, {case.polys});
  process.stdout.write(JSON.stringify({{ status: Array.from(got.status), coefs: hex(got.coefs), evals: hex(got.evals),
    refusal, again: hex(again.status) === hex(got.status) && hex(again.coefs) === hex(got.coefs) }}));
}})();
"""
    out = json.loads(subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300).decode())
    assert out["status"] == status
    L, E = 32 * case.length, 32 * n
    for b, (s, want) in enumerate(case.expect):
        if s == 1:
            assert bytes.fromhex(out["coefs"])[L * b:L * (b + 1)] == coefs[L * b:L * (b + 1)] == Z.mont(want)
            assert bytes.fromhex(out["evals"])[E * b:E * (b + 1)] == evals[E * b:E * (b + 1)]
    assert len(out["coefs"]) == 2 * L * case.polys and len(out["evals"]) == 2 * E * case.polys
    assert out["refusal"]["code"] == -1 and f"index[{len(case.index)}]" in out["refusal"]["message"]
    assert out["again"] is True
