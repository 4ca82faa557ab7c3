"""Register fit of the bucket accumulation (CPU: cross-compiles msm.hip to gfx950 assembly).

Two k_accumulate<3, .> waves must leave 176 of a SIMD's 512 VGPRs to the other in-flight proofs'
kernels ("Register budget"), so that build holds at most 168 VGPRs; the <2, .> build
reserves 176. Neither may touch scratch memory: a spilled loop-carried register costs more than the
CIOS rows of field29.hpp's fq29::reduce_row_qstar save. Read from the kernel metadata of the compiled
code object (vgpr_count, private_segment_fixed_size) and from the kernels' instruction streams.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kzg-grandsums-study_amd", "csrc", "msm.hip")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
LIMIT = {2: 176, 3: 168}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("acc") / "msm.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                           "-Wno-pass-failed", "-S", SRC, "-o", out], stderr=subprocess.DEVNULL)
    with open(out) as fh:
        return fh.read()


def _kernels(asm):
    """{(VW, ZP): (symbol, metadata block)} of the k_accumulate instantiations"""
    out = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s*\d+", asm, re.S):
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        m = re.match(r"_ZN3kgs12k_accumulateILi(\d)ELb([01])EEE", name)
        if m:
            out[(int(m.group(1)), bool(int(m.group(2))))] = (name, blk)
    return out


def test_accumulate_fits_its_register_budget_without_scratch(asm):
    ks = _kernels(asm)
    assert sorted(ks) == [(2, False), (2, True), (3, False), (3, True)]
    for (vw, zp), (name, blk) in sorted(ks.items()):
        field = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1))
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        scratch = [ln.strip() for ln in body.split("\n") if ln.strip().startswith("scratch_")]
        print(f"k_accumulate<{vw}, {zp}>: {field('vgpr_count')} VGPRs, private segment "
              f"{field('private_segment_fixed_size')} B, {len(scratch)} scratch instructions")
        assert field("vgpr_count") <= LIMIT[vw], (vw, zp)
        assert field("private_segment_fixed_size") == 0, (vw, zp)
        assert field("vgpr_spill_count") == 0, (vw, zp)
        assert not scratch, (vw, zp, scratch[:4])
