#!/usr/bin/env python3
"""Generate tests/golden/multi.json: multi-argument proofs (include/kgs.h kgs_prove_multi) from the
pure-Python restatement tests/multi_oracle.py on the synthetic power-11 ptau (tau = the bench tau).

The cases are multi_cases.FIXTURE_CASES: the mixes [gs, gp, lookup] and [gs k=3 sel, gp k=2, lookup k=2,
gp sel] at nbits 8 and 11 (at 11 the W_xi numerator, 2n - 2 coefficients, spans two Horner tiles of
the GPU prover). Inputs are regenerated from their seeds by multi_cases (tests/common.make_inputs /
make_lookup_inputs); the file stores a digest of them and the hex proof only. Every proof is checked by
the restated verifier (trapdoor form of the pairing equation) before it is written. These vectors pin the
GPU prover to the restatement; the protocol is not in the reference, so no reference output exists.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import common  # noqa: E402
import multi_cases as MC  # noqa: E402
import multi_oracle as MO  # noqa: E402


def main():
    cases = []
    for mix, nbits in MC.FIXTURE_CASES:
        args = MC.arguments(mix, nbits)
        shapes = MC.shapes_of(args)
        coms, evs = MC.restated(mix, nbits)
        assert MO.verify_multi(shapes, (coms, evs), nbits, common.tau()), (mix, nbits)
        cases.append({"mix": mix, "nbits": nbits, "shapes": [list(s) for s in shapes], "inputs_sha256": MC.digest(args),
                      "commitments": [c.hex() for c in coms], "evaluations": [e.hex() for e in evs]})
        print(mix, nbits, "ok", file=sys.stderr)
    with open(MC.MULTI_JSON, "w") as fh:
        json.dump({"ptau": "synthetic power 11, tau = oracle.ptau.bench_tau()", "cases": cases}, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
