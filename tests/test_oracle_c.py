"""The C restatement (oracle/c, used for large-n parity and as bench.py's cpu_baseline) agrees with
the Python oracle: every golden vector, keccak, and MSM vs the closed form."""
import ctypes
import json
import os
import random

import pytest

import common
from oracle import bn254 as bn
from oracle import cbackend as C
from oracle import protocol as P
from oracle.keccak import keccak256

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


def test_keccak():
    out = ctypes.create_string_buffer(32)
    for m in (b"", b"abc", b"z" * 136, b"q" * 500):
        C.lib().orc_keccak256(m, len(m), out)
        assert out.raw == keccak256(m)


@pytest.mark.parametrize("logm", [0, 1, 2, 5, 8, 10])
def test_ntt_matches_python_oracle(logm):
    """oracle.c's transform (the checker of the GPU NTT at 2^18..2^22) against poly.ntt."""
    from oracle import poly as OP
    rnd = random.Random(logm)
    v = [rnd.randrange(bn.R) for _ in range(1 << logm)]
    for inverse in (False, True):
        assert C.ntt(common.mont_bytes(v), inverse) == common.mont_bytes(OP.ntt(v, inverse))


@pytest.mark.parametrize("m", [0, 1, 2, 63, 4096, 4097, 10000])
def test_scale_powers_matches_python_oracle(m):
    """oracle.c's orc_scale_powers (data[j] *= base^j; chunks of 4096 with their own starting power)
    against Python integers, for the coset generator, its inverse, 0, 1 and r - 1."""
    import ntt_cases as N
    rnd = random.Random(m)
    v = [rnd.randrange(bn.R) for _ in range(m)]
    for base in (N.COSET_GEN, pow(N.COSET_GEN, bn.R - 2, bn.R), 0, 1, bn.R - 1, rnd.randrange(bn.R)):
        want = [x * pow(base, j, bn.R) % bn.R for j, x in enumerate(v)]
        assert C.scale_powers(common.mont_bytes(v), base) == common.mont_bytes(want), base


def test_coset_reference_c_matches_python():
    """The two references of kgs_ntt_ex (tests/ntt_cases.py) agree at 2^10 on every flag combination the
    GPU tests use, with a full and a short forward input: the C one checks the GPU above 2^12."""
    import ntt_cases as N
    logm = 10
    m = 1 << logm
    x = N.random_elements(77, m)
    assert N.COSET_GEN == bn.FR_NQR  # g <w> misses <w>: g is the field's non-residue
    for flags in (0, N.BITREV, N.COSET, N.COSET | N.BITREV):
        for in_len in (m, m // 2, 65, 0):
            d = x[:32 * in_len]
            assert N.ref_c(d, logm, flags) == common.mont_bytes(N.ref_py(N.unmont(d), logm, flags)), (flags, in_len)
    for flags in (0, N.BITREV, N.NO_SCALE, N.COSET, N.COSET | N.BITREV, N.COSET | N.BITREV | N.NO_SCALE):
        f = flags | N.INVERSE
        assert N.ref_c(x, logm, f) == common.mont_bytes(N.ref_py(N.unmont(x), logm, f)), flags
    # and the inverse undoes the forward in every order
    for flags in (0, N.BITREV, N.COSET, N.COSET | N.BITREV):
        assert N.ref_c(N.ref_c(x, logm, flags), logm, flags | N.INVERSE) == x


def test_msm_closed_form():
    _, srs = C.load_srs_bytes(common.oracle_ptau(9))
    o = P.SRS(common.oracle_ptau(9), common.tau())
    rnd = random.Random(4)
    for n in (1, 5, 100, 1023):
        v = [rnd.randrange(bn.R) for _ in range(n)]
        assert C.msm(srs, common.mont_bytes(v), 2) == bn.g1_to_lem(o.msm(v))


@pytest.mark.parametrize("case", GOLD["cases"],
                         ids=lambda c: f'{c["kind"]}-k{c["npols"]}-s{int(c["selected"])}-n{c["nbits"]}')
def test_c_oracle_matches_golden(case):
    _, srs = C.load_srs_bytes(common.oracle_ptau(11))
    K = common.load_pkg()
    kind = 0 if case["kind"] == "grandsum" else 1
    Fs, Ts, sF, sT = common.make_inputs(case["seed"], case["nbits"], case["npols"], case["selected"])
    coms, evs = C.prove_raw(kind, case["nbits"], Fs, Ts, sF, sT, srs, 2)
    cn, en = K.proof_names(kind, case["npols"], case["selected"])
    got = {"commitments": {k: v.hex() for k, v in zip(cn, coms)},
           "evaluations": {k: v.hex() for k, v in zip(en, evs)}}
    assert got == case["proof"]


def test_c_oracle_errors():
    _, srs = C.load_srs_bytes(common.oracle_ptau(6))
    Fs, Ts, _, _ = common.make_inputs(5, 3, 1, False)
    Fs2, _, _, _ = common.make_inputs(6, 3, 1, False)
    with pytest.raises(ValueError, match="not well calculated"):
        C.prove_raw(0, 3, Fs, Fs2, None, None, srs, 1)
    sel = common.mont_bytes([2] + [1] * 7)
    with pytest.raises(ValueError, match="Polynomial is not divisible"):
        C.prove_raw(1, 3, Fs, Fs, sel, sel, srs, 1)
