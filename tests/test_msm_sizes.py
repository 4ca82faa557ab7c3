"""The MSM work-buffer sizes (csrc/msm_sizes.hpp msm_work_sizes) against the largest index each
kernel of csrc/msm.hip can form, for both drivers: the fixed-base commitment MSM (msm_run) and the
variable-base MSM (msm_points_run).

A stand-alone host program (tests/native/msm_sizes_dump.cpp, plain g++, nothing but the sizing
header) prints the header's constants and the sizes of every shape of the sweep. The bounds below
are restated here from the launch code with those constants; the header is not trusted for them.
No GPU, nothing loaded into Python.
"""
import json
import os
import shutil
import subprocess

import pytest

import common

CSRC = os.path.join(common.ROOT, "kzg-grandsums-study_amd", "csrc")
SRC = os.path.join(common.ROOT, "tests", "native", "msm_sizes_dump.cpp")

FIXED = [(n, c) for c in range(7, 21) for n in (1, 255, 1 << 12, (1 << 16) + 1, 1 << 21, 1 << 25)]
VAR_N = (1, 257, 4097, 1 << 16, 1 << 20, 1 << 26)


def windows(c):
    return (255 + c - 1) // c


VAR = [(n, c) for c in range(7, 17) for n in VAR_N if n * windows(c) <= 1 << 31]

# Work buffers of the parent commit 67a4f64 (ensure_msm_work and msm_points_sizes as they were), bytes,
# chunkcnt's 64 included: both lanes of the fixed base at 2^21 resident points with c = 17, and the
# variable base at 2^20 points with the automatic window (c = 16)
PARENT_FIXED_2P21_C17_BOTH_LANES = 835888976
PARENT_VAR_2P20_AUTO = 438482184
CHUNKCNT_BYTES = 64


def dump(tmp, shapes, flags=()):
    exe = os.path.join(tmp, "msm_sizes_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])
    out = subprocess.run([exe, *shapes], capture_output=True, text=True, timeout=120, check=True).stdout
    return json.loads(out)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the library's host units; this test needs it too"
    shapes = [f"f:{n}:{c}" for n, c in FIXED] + [f"v:{n}:{c}" for n, c in VAR]
    d = dump(str(tmp_path_factory.mktemp("msm_sizes")), shapes)
    assert len(d["shapes"]) == len(FIXED) + len(VAR)
    return d


def seg_len(E, resident, K):
    """msm_buckets: one segment per resident accumulate thread, at least SEG_MIN_LEN entries, at most
    SEG_MAX segments"""
    L = max(-(-E // resident), K["SEG_MIN_LEN"])
    if -(-E // L) > K["SEG_MAX"]:
        L = -(-E // K["SEG_MAX"])
    return L


def bounds(s, K):
    """{buffer: bytes the kernels can touch} for one shape, from the launch geometry"""
    N, c, cs, var = s["N"], s["c"], s["cs"], s["var"]
    W = windows(c)
    E = N * W  # entries: one per (scalar, window) with a nonzero digit
    keys = W << (c - 1) if var else 1 << (c - 1)
    wins = W if var else 1
    lob, NH = s["lob"], s["NH"]
    # the sort's partitions: NH partitions of 2^lob keys cover the 2^(cs-1) keys of the sort window, the
    # lo key fits k_sort_part's byte, and hi_off / cpre (NH + 1 words) fit their NH_MAX + 8 slots
    assert NH << lob == 1 << (cs - 1) and lob <= 8 and NH <= K["NH_MAX"]
    assert keys <= 1 << (cs - 1)
    nblk = -(-N // (256 * K["SORT_SPT"]))  # grid of k_sort_hist / k_sort_part
    chunks = min(NH * K["SL_G"], NH + E // K["SL_CHUNK"])  # lo-pass grid: sum_p clamp(ceil(size_p / SL_CHUNK), 1, SL_G)
    # segments for any chip: 1 CU .. far more resident threads than entries
    nseg = max(-(-E // seg_len(E, r, K)) for r in (256, 304 * 2 * 256, 256 * 2 * 256, 1 << 40))
    assert nseg <= min(K["SEG_MAX"], -(-E // K["SEG_MIN_LEN"]))
    nseg = min(K["SEG_MAX"], -(-E // K["SEG_MIN_LEN"]))
    h, l = c - 1 - c // 2, c // 2
    return {
        "digit": 4 * E,                                    # k_sort_part tval[g], g < E
        "sorted": 4 * max(E, 8 * N if var else 0),         # k_lo_scatter sorted[e], e < E; VAR: 8 words per scalar
        "lo": E + 16,                                      # k_sort_part tlo[g]; k_lo_count's 16-byte loads
        "blockhist": 4 * NH * nblk,                        # bh[p * nblk + block]
        "counts": 4 * NH,                                  # ptot[p]
        "offsets": 4 * (max(1 << (cs - 1), keys + 1) + 1),  # offsets[(p << lob) + lo + 1], offsets[keys + 1]
        "cursor": 4 * (2 * (K["NH_MAX"] + 8) + chunks),    # bpart[b] behind hi_off and cpre
        "segowner": 4 * nseg,                              # segowner[s]
        "locnt": 4 * (NH << lob) * K["SL_G"],              # locnt[((p << lob) + lo) * SL_G + g]
        "chunklist": 4 * K["CB_LEVELS"] * (nseg // K["CB_T"] + keys + 16),  # CB_LEVELS lists of lcap entries
        "raw29": 4 * K["RAW29_WORDS"] * (keys + 1 + nseg),  # run_rec(raw, nbins + s), nbins = keys + 1
        "part": 4 * K["RAW29_WORDS"] * wins * ((1 << h) + (1 << l)),  # rc[RAW29_WORDS * (win * lines + line)]
        "T": 128 * wins * c,                               # T[32 * (win * c + k)]
    }


def test_every_buffer_holds_its_largest_index(table):
    K = table["constants"]
    for s in table["shapes"]:
        need = bounds(s, K)
        assert set(need) == set(s["sizes"])
        for name, b in need.items():
            assert s["sizes"][name] >= b, (name, s["var"], s["N"], s["c"], s["sizes"][name], b)


def test_sizes_grow_with_the_point_count(table):
    """buffers sized for the resident SRS serve every shorter MSM (ensure_msm_work sizes once)"""
    by = {}
    for s in table["shapes"]:
        by.setdefault((s["var"], s["c"]), []).append(s)
    for group in by.values():
        group.sort(key=lambda s: s["N"])
        for a, b in zip(group, group[1:]):
            assert all(a["sizes"][k] <= b["sizes"][k] for k in a["sizes"]), (a["N"], b["N"], a["c"])


def shape(table, var, n, c):
    return next(s for s in table["shapes"] if (s["var"], s["N"], s["c"]) == (var, n, c))


def test_footprint_not_above_the_parent(table):
    fixed = 2 * (shape(table, False, 1 << 21, 17)["total"] + CHUNKCNT_BYTES)
    var = shape(table, True, 1 << 20, 16)["total"] + CHUNKCNT_BYTES
    print("fixed base, 2^21 points, c = 17, both lanes:", fixed, "parent", PARENT_FIXED_2P21_C17_BOTH_LANES)
    print("variable base, 2^20 points, c = 16:", var, "parent", PARENT_VAR_2P20_AUTO)
    assert fixed <= PARENT_FIXED_2P21_C17_BOTH_LANES
    assert var <= PARENT_VAR_2P20_AUTO


def test_build_knobs_resize_the_buffers(table, tmp_path):
    """-DKGS_SL_CHUNK / -DKGS_SL_G / -DKGS_SORT_SPT reach the sizes through the same constants the
    kernels index with"""
    shapes = ["f:2097152:17", "v:1048576:16", "f:4096:8", "v:257:7"]
    d = dump(str(tmp_path), shapes, ["-DKGS_SL_CHUNK=8192", "-DKGS_SL_G=128", "-DKGS_SORT_SPT=1"])
    K = d["constants"]
    assert (K["SL_CHUNK"], K["SL_G"], K["SORT_SPT"]) == (8192, 128, 1)
    for s in d["shapes"]:
        for name, b in bounds(s, K).items():
            assert s["sizes"][name] >= b, (name, s)
    big, ref = d["shapes"][0], shape(table, False, 1 << 21, 17)
    assert big["sizes"]["cursor"] > ref["sizes"]["cursor"] and big["sizes"]["locnt"] == 2 * ref["sizes"]["locnt"]
