"""The thread mapping of the batched G1 transform stage (csrc/g1ntt_map.hpp, the index arithmetic of
k_g1ntt_stage_many and of its launch) without a GPU, and the NULL-context refusals of kgs_kzg_open_cosets_many.

A stand-alone host program (tests/native/g1ntt_map_dump.cpp, plain g++, nothing but the mapping header)
enumerates every block and lane of every stage of the sweep. The formulas below are restated from
k_g1ntt_stage (g1ntt.hip), which a single polynomial's transform runs; the header is not trusted for them.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

import common

CSRC = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "csrc")
SRC = os.path.join(common.ROOT, "tests", "native", "g1ntt_map_dump.cpp")
POLYS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 130)
LOGN = range(1, 9)
KGS_E_ARG = -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the library's host units; this test needs it too"
    out = os.path.join(str(tmp_path_factory.mktemp("g1ntt_map")), "g1ntt_map_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", out])
    return out


def dump(exe, shapes):
    """[(logn, logh, polys, uniform, blocks, [[lane or None] * 64 per block])]"""
    out = subprocess.run([exe, *shapes], capture_output=True, text=True, timeout=300, check=True).stdout
    res = []
    for line in out.splitlines():
        if line.startswith("S "):
            logn, logh, polys, uni, blocks = map(int, line.split()[1:])
            res.append((logn, logh, polys, bool(uni), blocks, []))
        else:
            res[-1][5].append([None if x == "-" else tuple(map(int, x.split(","))) for x in line.split()])
    assert len(res) == len(shapes)
    return res


def check_stage(logn, logh, polys, uni, blocks, lanes, want_uni):
    n, h = 1 << logn, 1 << logh
    G = n // (2 * h)
    where = (logn, logh, polys)
    assert uni == want_uni, where
    assert len(lanes) == blocks and all(len(b) == 64 for b in lanes), where
    seen = set()
    for block in lanes:
        live = [x for x in block if x is not None]
        if uni:  # one twiddle per 64-lane block, whatever G is
            assert len({x[2] for x in live}) <= 1, where
        for poly, g, t, pa, pb, tw in live:
            assert poly < polys and g < G and t < h, where  # an active lane is a butterfly of the stage
            # k_g1ntt_stage for this polynomial alone, its points at poly * n:
            #   pa = (g << (logh + 1)) + t, pb = pa + h, twiddle record t << logG
            assert pa == poly * n + g * 2 * h + t and pb == pa + h and tw == t * G, where
            assert pb < polys * n and tw < n // 2, where
            seen.add((poly, g, t))
    # each (polynomial, butterfly) exactly once; every other lane idle
    assert sum(x is not None for b in lanes for x in b) == len(seen) == polys * n // 2, where
    # no block beyond what the butterflies need: fewer than 64 idle lanes per twiddle (uniform) or in all (per lane)
    idle = 64 * blocks - len(seen)
    assert idle < 64 * (h if uni else 1), where


def test_library_mapping_covers_every_butterfly_once(exe):
    """every transform size 2^1 .. 2^8, every stage, every polys of the sweep, with the mapping the library takes:
    uniform from polys * G = 64 on in every stage but the first (whose only twiddle is 1)"""
    shapes = [f"{logn}:{logh}:{p}:a" for logn in LOGN for logh in range(logn) for p in POLYS]
    res = dump(exe, shapes)
    count = 0
    for logn, logh, polys, uni, blocks, lanes in res:
        G = (1 << logn) >> (logh + 1)
        check_stage(logn, logh, polys, uni, blocks, lanes, logh > 0 and polys * G >= 64)
        count += uni
    assert 0 < count < len(res)  # both mappings occur
    # the seams the GPU tests run: polys * G crosses 64 in the last (G = 1) and the second-last (G = 2) stage
    by = {(a, b, c): d for a, b, c, d, _, _ in res}
    assert [by[(3, 2, p)] for p in (63, 64, 65)] == [False, True, True]
    assert [by[(3, 1, p)] for p in (31, 32, 33)] == [False, True, True]
    assert by[(8, 1, 1)] and not by[(8, 2, 1)]  # one polynomial: k_g1ntt_stage's rule, G >= 64


def test_per_lane_mapping_forced(exe):
    """the other arm of the A/B (G1NTT_MAP_LANE): the per-lane mapping at every stage"""
    shapes = [f"{logn}:{logh}:{p}:l" for logn in range(1, 7) for logh in range(logn) for p in POLYS]
    for logn, logh, polys, uni, blocks, lanes in dump(exe, shapes):
        check_stage(logn, logh, polys, uni, blocks, lanes, False)


def test_null_context_is_refused():
    """both entries, on the built library, no GPU touched"""
    L = common.load_pkg().lib()
    b = ctypes.create_string_buffer(64)
    for name in ("kgs_kzg_open_cosets_many", "kgs_kzg_open_cosets_many_device"):
        for polys in (0, 1):
            rc = getattr(L, name)(None, b, polys, 1, 1, 0, 0, b, None)
            assert rc == KGS_E_ARG and "ctx" in L.kgs_last_error().decode(), (name, polys)
