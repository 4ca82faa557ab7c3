"""The curve shim's G1.fft / G1.ifft (addon g1Ntt -> kgs_g1_ntt) and the package's commit_evals (addon
commitEvals -> kgs_commit_evals) against the Python entry points: 2^4 and 2^8 points, affine and
Jacobian in and out, the bad-length error."""
import json
import os
import shutil
import subprocess

import pytest

import common
import degenerate_cases as D
import g1_ntt_cases as N
from oracle import ptau as opt

JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_shim_fft_ifft_and_commit_evals(tmp_path):
    K = common.load_pkg()
    ptau = common.oracle_ptau(8)
    bases = opt.PTau(ptau).g1_bytes
    want = {}
    for lg in (4, 8):
        x = bytearray(bases[:64 << lg])
        x[64 * 3:64 * 4] = bytes(64)  # an identity among the points
        (tmp_path / f"points_{lg}.bin").write_bytes(x)
        want[f"fft_{lg}"] = K.g1_ntt(bytes(x)).hex()
        want[f"ifft_{lg}"] = K.g1_ntt(bytes(x), inverse=True).hex()
    evals = N.scalar_bytes(D.random_scalars(256, 9))
    (tmp_path / "evals.bin").write_bytes(evals)
    want["commit"] = K.commit_evals(ptau, evals).hex()
    want["bad_length"] = "fft must be multiple of 2"
    script = f"""
const fs = require('fs');
const {{ getCurveFromName, commit_evals }} = require('./index.js');
const load = name => new Uint8Array(fs.readFileSync('{tmp_path}/' + name));
getCurveFromName('bn128').then(async c => {{
  const G1 = c.G1, out = {{}};
  const hex = b => Buffer.from(b).toString('hex');
  const map = (b, size, fn) => {{
    const parts = [];
    for (let i = 0; i < b.byteLength; i += size) parts.push(fn(b.subarray(i, i + size)));
    return Buffer.concat(parts);
  }};
  for (const lg of [4, 8]) {{
    const aff = load('points_' + lg + '.bin');
    const jac = new Uint8Array(map(aff, 64, G1.toJacobian));
    for (const op of ['fft', 'ifft']) {{
      const r = [await G1[op](aff), await G1[op](aff, 'affine', 'affine', null, 'ignored'),
                 map(await G1[op](aff, 'affine', 'jacobian'), 96, G1.toAffine),
                 await G1[op](jac, 'jacobian', 'affine'),
                 map(await G1[op](jac, 'jacobian', 'jacobian'), 96, G1.toAffine)].map(hex);
      if (!r.every(h => h === r[0])) throw new Error(op + ' ' + lg + ': the point formats disagree');
      out[op + '_' + lg] = r[0];
    }}
  }}
  out.commit = hex(await commit_evals('{ptau}', load('evals.bin')));
  try {{
    await G1.fft(load('points_4.bin').subarray(0, 64 * 12));
    out.bad_length = 'no error';
  }} catch (e) {{
    out.bad_length = e.message;
  }}
  process.stdout.write(JSON.stringify(out));
}});
"""
    out = subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300)
    assert json.loads(out.decode()) == want
