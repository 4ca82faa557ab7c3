"""Shared inputs of test_msm_points.py (CPU, host path) and test_gpu_msm_points.py (GPU): bases with a
known answer for the variable-base MSM (kgs_msm_points).

The bases are the SRS of a trapdoor, P_i = tau^i G, so sum_i s_i P_i = (sum_i s_i tau^i mod r) G: one
oracle scalar multiplication per expected value. The degenerate families (all points equal, P / -P
alternating, a 4-cycle, G followed by zero points) come from degenerate_cases.py.
"""
import functools

import common
import degenerate_cases as D
from oracle import bn254 as bn

R = bn.R
WINDOWS = (0, 7, 8, 11, 13, 16)  # window_c: the library's choice, both ends of the range, odd and even widths


def scalar_bytes(vals):
    """any integers in [0, 2^256) as 32 B little-endian standard forms"""
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


@functools.lru_cache(None)
def _tau_powers(n):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * common.tau() % R
    return out


def closed_form(scalars):
    """(sum s_i tau^i) G for the bases tau^i G of a synthetic ptau with common.tau(), 64 B LEM"""
    acc = sum(s * t for s, t in zip(scalars, _tau_powers(len(scalars)))) % R
    return bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, acc))  # acc == 0: 64 zero bytes


def windows(c):
    return (255 + c - 1) // c


def auto_window(n):
    """the library's choice for window_c = 0: clamp(ceil(log2 n) - 4, 7, 16)"""
    return min(max((n - 1).bit_length() - 4, 7), 16)


def every_window(c, digit):
    """the scalar whose every window below the top holds `digit` (the top window holds 0)"""
    return sum(digit << (c * j) for j in range(windows(c) - 1))


def digit_edge_scalars(c):
    """(id, scalar) at the edges of the signed-digit recoding with window c: every window below the top
    exactly 2^(c-1) (key B, no carry); every one 2^(c-1) + 1 (a negative digit and a carry into the next
    window, all the way up); r - 1; zero"""
    half = 1 << (c - 1)
    out = [("half", every_window(c, half)), ("half+1", every_window(c, half + 1)), ("r-1", R - 1), ("zero", 0)]
    assert all(0 <= s < R for _, s in out)
    return out
