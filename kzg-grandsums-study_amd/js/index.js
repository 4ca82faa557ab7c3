// JavaScript host of the MI355X prover: the reference's module surface.
module.exports = {
    getCurveFromName: require("./src/curve").getCurveFromName,
    BigBuffer: require("./src/bigbuffer").BigBuffer,
    Scalar: require("./src/scalar").Scalar,
    Evaluations: require("./src/polynomial/evaluations").Evaluations,
    mset_eq_kzg_grandsum_prover: require("./src/grandsum/mset_eq_kzg_prover"),
    mset_eq_kzg_grandproduct_prover: require("./src/grandproduct/mset_eq_kzg_prover"),
    mset_eq_kzg_grandsum_verifier: require("./src/grandsum/mset_eq_kzg_verifier"),
    mset_eq_kzg_grandproduct_verifier: require("./src/grandproduct/mset_eq_kzg_verifier"),
    lookup_kzg_grandsum_prover: require("./src/lookup/lookup_kzg_prover"),
    lookup_kzg_grandsum_verifier: require("./src/lookup/lookup_kzg_verifier"),
    // the table's multiplicities from the witness and the table, and the prover that computes them itself
    lookup_multiplicities: require("./src/lookup/lookup_multiplicities"),
    lookup_kzg_grandsum_prover_from_table: require("./src/lookup/lookup_multiplicities").lookup_kzg_grandsum_prover_from_table,
    // commit_evals(pTauFilename, evals): the commitment to a column given as standard-form evaluations, over
    // the Lagrange-basis SRS built on the GPU (kgs_commit_evals)
    commit_evals: require("./src/backend").commitEvals,
    // kzg_open_all(pTauFilename, coefs) -> {proofs, evals}: the opening proofs of a polynomial (Montgomery
    // coefficients) at every point of its domain at once (kgs_kzg_open_all); one of them is checked with
    // curve.pairingEq(proof, [tau]_2, -(C - y G + z proof), [1]_2)
    kzg_open_all: require("./src/backend").kzgOpenAll,
    // kzg_open_cosets(pTauFilename, coefs, lBits) -> {proofs, evals}: one proof per coset of 2^lBits points of
    // the domain (kgs_kzg_open_cosets); kzg_verify_coset(commit, nBits, lBits, index, ysMont, proof, srsG1,
    // tauLG2) -> bool checks one of them on the host (kgs_kzg_verify_coset)
    kzg_open_cosets: require("./src/backend").kzgOpenCosets,
    kzg_verify_coset: require("./src/backend").kzgVerifyCoset,
    // kzg_open_cosets_many(pTauFilename, [coefs ..], lBits) -> {proofs: [..], evals: [..]}: kzg_open_cosets for many
    // polynomials over one domain and SRS in one call, every stage launched once (kgs_kzg_open_cosets_many)
    kzg_open_cosets_many: require("./src/backend").kzgOpenCosetsMany,
    // kzg_verify_cosets_batch(commits, nBits, lBits, openings, srsG1, tauLG2[, {host, seed}]) -> Promise<{valid, ..}>:
    // many coset openings {commit, index, ys, proof} against one SRS with one pairing check, folded on the GPU
    // (kgs_kzg_verify_cosets_batch)
    kzg_verify_cosets_batch: require("./src/backend").kzgVerifyCosetsBatch,
    // kzg_recover_cosets(nBits, lBits, cells, length) -> Promise<{ok, coefs, evals}>: the polynomial of `length`
    // coefficients through the cells {index, ys} it is given, rebuilt on the GPU (kgs_kzg_recover_cosets)
    kzg_recover_cosets: require("./src/backend").kzgRecoverCosets,
    // kzg_recover_cosets_many(nBits, lBits, cells, length, polys) -> Promise<{status, coefs, evals}>: `polys`
    // polynomials of `length` coefficients each through the cells {poly, index, ys} they are given, rebuilt on the GPU
    // in one call (kgs_kzg_recover_cosets_many); status holds 1 / 0 / 2 per polynomial
    kzg_recover_cosets_many: require("./src/backend").kzgRecoverCosetsMany,
    // one proof of several arguments of any kinds over one domain (kgs_prove_multi / kgs_verify_multi)
    mset_eq_kzg_multi_prover: require("./src/multi/mset_eq_kzg_multi_prover"),
    mset_eq_kzg_multi_verifier: require("./src/multi/mset_eq_kzg_multi_verifier"),
    // many proofs against one ptau, one pairing check (kgs_verify_batch)
    kzg_verifier_batch: require("./src/verifier_batch"),
    // the provers' log channel (the reference's logger.js lines): setLogger(logplease instance), setLogLevel
    logger: require("./src/logger"),
};
