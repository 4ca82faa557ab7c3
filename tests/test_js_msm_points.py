"""The curve shim's G1.multiExpAffine over the variable-base MSM (addon msmPoints -> kgs_msm_points): two
calls in flight on the shim's one context, started without awaiting between them."""
import json
import os
import random
import shutil
import subprocess

import pytest

import common
from oracle import bn254 as bn

JS = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_two_multiexp_calls_in_flight(tmp_path):
    rnd = random.Random(17)
    want = {}
    for tag, n in (("a", 1000), ("b", 17)):
        ks = [rnd.randrange(1, bn.R) for _ in range(n)]
        ss = [rnd.randrange(bn.R) for _ in range(n)]
        (tmp_path / f"bases_{tag}.bin").write_bytes(b"".join(bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, k)) for k in ks))
        (tmp_path / f"scalars_{tag}.bin").write_bytes(b"".join(s.to_bytes(32, "little") for s in ss))
        want[tag] = bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, sum(k * s for k, s in zip(ks, ss)) % bn.R)).hex()
    script = f"""
const fs = require('fs');
const {{ getCurveFromName }} = require('./src/curve.js');
const load = name => new Uint8Array(fs.readFileSync('{tmp_path}/' + name));
getCurveFromName('bn128').then(async c => {{
  const pa = c.G1.multiExpAffine(load('bases_a.bin'), load('scalars_a.bin'));
  const pb = c.G1.multiExpAffine(load('bases_b.bin'), load('scalars_b.bin'));
  const [a, b] = await Promise.all([pa, pb]);
  const hex = p => Buffer.from(c.G1.toAffine(p)).toString('hex');
  process.stdout.write(JSON.stringify({{ a: hex(a), b: hex(b) }}));
}});
"""
    out = subprocess.check_output([NODE, "-e", script], cwd=JS, timeout=300)
    assert json.loads(out.decode()) == want
