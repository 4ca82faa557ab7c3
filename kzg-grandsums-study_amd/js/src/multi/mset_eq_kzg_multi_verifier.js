// Verifier of mset_eq_kzg_multi_prover's proofs, run natively by libkgs (kgs_verify_multi_ptau: transcript
// replay and ONE pairing check, host only).
//   shapes: the arguments the proof was made for, [{ kind: "grandsum" | "grandproduct" | "lookup" (or
//           the number), npols, selected }]; defaults to the `shapes` member the prover attaches
// A missing member of the proof throws, as in the single verifiers (a malformed proof object); a value of
// the wrong size just fails to verify.
const backend = require("../backend");
const logger = require("../logger");
const path = require("path");
const { proofNames, KIND } = require("./mset_eq_kzg_multi_prover");

module.exports = async function mset_eq_kzg_multi_verifier(pTauFilename, proof, nBits, shapes = undefined) {
    logger.info("> MULTI-ARGUMENT KZG VERIFIER STARTED");
    if (shapes === undefined || shapes === null) shapes = proof.shapes;
    if (!Array.isArray(shapes) || shapes.length < 1) throw new TypeError("the shapes of the proof's arguments are missing");
    shapes = shapes.map(s => ({ kind: typeof s.kind === "number" ? s.kind : KIND[s.kind], npols: s.npols, selected: !!s.selected }));
    const names = proofNames(shapes);
    for (const n of names.commitments)
        if (proof.commitments[n] === undefined || proof.commitments[n] === null)
            throw new TypeError(`proof.commitments.${n} is missing`);
    for (const n of names.evaluations)
        if (proof.evaluations[n] === undefined || proof.evaluations[n] === null)
            throw new TypeError(`proof.evaluations.${n} is missing`);
    const sized = (v, len) => v instanceof Uint8Array && v.length === len;
    if (!names.commitments.every(n => sized(proof.commitments[n], 64)) ||
        !names.evaluations.every(n => sized(proof.evaluations[n], 32))) {
        logger.warn("> MULTI-ARGUMENT KZG VERIFIER: a proof member has the wrong size");
        return false;
    }
    const com = Buffer.concat(names.commitments.map(n => Buffer.from(proof.commitments[n])));
    const ev = Buffer.concat(names.evaluations.map(n => Buffer.from(proof.evaluations[n])));
    const ok = backend.load().verifyMultiPtau(path.resolve(pTauFilename), nBits, shapes, com, ev);
    logger.info(`> MULTI-ARGUMENT KZG VERIFIER FINISHED: ${ok ? "valid" : "invalid"} proof`);
    return ok;
};
