"""Shared references of test_kzg_coset_batch_refs.py (CPU) and test_gpu_kzg_coset_batch.py (GPU): the batch
verifier for coset openings (kgs_kzg_verify_cosets_batch) on integers, over an SRS s_k = tau^k G
with the known tau of common.tau(). Notation of kzg_coset_cases: n = 2^nbits, l = 2^lbits, m = n / l, w = Fr.w[nbits],
a_i = w^(i l). Opening k is (commit index c(k), coset index i_k, values y_k, proof scalar pi_k: the proof is pi_k G).

  seed, rho   Keccak over the batch, as include/kgs.h states it
  D           sum_k rho^k I_k with I_k from kzg_coset_cases.interpolant
  A, B        in the exponent: A = sum_k rho^k pi_k, B = sum_k rho^k (p_c(k)(tau) + a_{i_k} pi_k) - D(tau)

An opening that fails a structural check (a value >= r, an index >= m, a commit index >= ncommits, a point off the
curve) has weight 0 in all three.
"""
import struct

import common
import g1_ntt_cases as N
import kzg_coset_cases as C
import kzg_open_cases as Z
from oracle import bn254 as bn

R = N.R
TAG = b"kgs-verify-cosets-batch-v1"


def keccak(data):
    return common.load_pkg().keccak256(data)


def seed_of(tau_l_g2, nbits, lbits, commits, commit_of, index, ys_bytes, proofs_bytes):
    """the derived seed: commits / ys_bytes / proofs_bytes are the concatenated buffers the library is given"""
    msg = TAG + tau_l_g2 + struct.pack("<II", nbits, lbits) + struct.pack("<Q", len(commits) // 64) + commits
    msg += struct.pack("<Q", len(commit_of)) + b"".join(struct.pack("<I", c) for c in commit_of)
    msg += b"".join(struct.pack("<Q", i) for i in index) + ys_bytes + proofs_bytes
    return keccak(msg)


def rho_of(seed):
    rho = int.from_bytes(keccak(TAG + b"/rho" + seed), "little") % R
    return rho or 1


class Batch:
    """polys: coefficient lists (at most n each); openings: (commit index, coset index, values, proof scalar)"""

    def __init__(self, nbits, lbits, polys, openings):
        self.nbits, self.lbits = nbits, lbits
        self.n, self.l, self.m = C.sizes(nbits, lbits)
        self.polys = [list(c) for c in polys]
        self.pt = [Z.poly_eval(c, common.tau()) for c in self.polys]
        self.openings = [(ci, i, list(ys), pi % R) for ci, i, ys, pi in openings]

    # ---- what the library is given
    def commits(self):
        return [N.point(p) for p in self.pt]

    def tuples(self):
        """the `openings` argument of kzg_verify_cosets_batch"""
        return [(ci, i, b"".join(int(y).to_bytes(32, "little") if y >= R else Z.mont([y]) for y in ys), N.point(pi))
                for ci, i, ys, pi in self.openings]

    def tau_l_g2(self):
        return C.tau_l_g2(self.lbits)

    def srs(self):
        return C.srs_g1(self.lbits)

    # ---- the references
    def structurally_valid(self, k):
        ci, i, ys, _ = self.openings[k]
        return ci < len(self.polys) and i < self.m and all(y < R for y in ys)

    def equation_holds(self, k):
        ci, i, ys, pi = self.openings[k]
        return self.structurally_valid(k) and C.check_identity(self.polys[ci], self.nbits, self.lbits, i, ys, pi)

    def verdicts(self):
        return [self.equation_holds(k) for k in range(len(self.openings))]

    def seed(self):
        t = self.tuples()
        return seed_of(self.tau_l_g2(), self.nbits, self.lbits, b"".join(self.commits()), [x[0] for x in t],
                       [x[1] for x in t], b"".join(x[2] for x in t), b"".join(x[3] for x in t))

    def weights(self, rho):
        return [pow(rho, k, R) if self.structurally_valid(k) else 0 for k in range(len(self.openings))]

    def interp(self, rho):
        """D_j, j < l"""
        D = [0] * self.l
        for w, (ci, i, ys, pi) in zip(self.weights(rho), self.openings):
            if w:
                d = C.interpolant(ys, self.nbits, self.lbits, i)
                D = [(a + w * b) % R for a, b in zip(D, d)]
        return D

    def folded_scalars(self, rho):
        """(A, B) in the exponent"""
        A = B = 0
        for w, (ci, i, ys, pi) in zip(self.weights(rho), self.openings):
            if w:
                A += w * pi
                B += w * (self.pt[ci] + C.a_of(self.nbits, self.lbits, i) * pi)
        return A % R, (B - Z.poly_eval(self.interp(rho), common.tau())) % R

    def folded(self, rho):
        A, B = self.folded_scalars(rho)
        return N.point(A) + N.point(B)


def valid_batch(nbits, lbits, coef_lists, picks):
    """a Batch of valid openings: picks = (polynomial index, coset index) pairs, proofs from closed_scalars"""
    pis = [C.closed_scalars(c, nbits, lbits) for c in coef_lists]
    evs = [Z.evals(c, nbits) for c in coef_lists]
    return Batch(nbits, lbits, coef_lists,
                 [(ci, i, C.coset_values(evs[ci], nbits, lbits, i), pis[ci][i]) for ci, i in picks])


def check_bound(b, count):
    """1 + 2 b ceil(log2 count): the most pairing checks a batch of `count` with b invalid openings may take"""
    return 1 + 2 * b * max(count - 1, 0).bit_length()


def interp_fold_reference(nbits, lbits, index, rows, weights):
    """kgs_coset_interp_fold on integers: rows[k] the l values of row k"""
    l = 1 << lbits
    D = [0] * l
    for i, ys, w in zip(index, rows, weights):
        if w % R:
            d = C.interpolant(ys, nbits, lbits, i)
            D = [(a + w * b) % R for a, b in zip(D, d)]
    return D


def interp_fold_reference_grouped(nbits, lbits, index, rows, weights):
    """the same sum by linearity: the rows of one index are combined first (sum_k w_k y_k), then interpolated once.
    For many rows over few distinct indices; pinned to interp_fold_reference on the CPU."""
    l = 1 << lbits
    by_index = {}
    for i, ys, w in zip(index, rows, weights):
        w %= R
        if w:
            acc = by_index.setdefault(i, [0] * l)
            for j, y in enumerate(ys):
                acc[j] = (acc[j] + w * y) % R
    D = [0] * l
    for i, comb in by_index.items():
        D = [(a + b) % R for a, b in zip(D, C.interpolant(comb, nbits, lbits, i))]
    return D
