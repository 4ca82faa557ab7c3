// Batch verifier (include/kgs.h kgs_verify_batch): many proofs against one ptau's [tau]_2 with ONE pairing
// check, the per-proof G1 linear combinations folded on the GPU of a pooled context.
//   kzg_verifier_batch(pTauFilename, [{kind, proof, nBits}, ...]) -> Promise<boolean[]>
// kind: "grandsum" | "grandproduct" | "lookup" (or the backend's 0 / 1 / 2); proof: the object the provers
// return. Each proof's shape is read from its keys as the single-proof verifiers do (nPols from /^F\d/,
// selectors from /^selF/). The verdicts are theirs, proof for proof; an item with a missing member, a value
// of the wrong length or a lookup without selectors is false without reaching the library.
// One INFO line summarises the call: count, invalid, pairing checks.
const backend = require("./backend");
const logger = require("./logger");

const KINDS = { grandsum: backend.GRANDSUM, grandproduct: backend.GRANDPRODUCT, lookup: backend.LOOKUP };

// -> {kind, nbits, npols, selected, commitments, evaluations} in the C-ABI order, or null
function layout(item) {
    const kind = typeof item.kind === "string" ? KINDS[item.kind] : item.kind;
    if (kind !== 0 && kind !== 1 && kind !== 2) throw new Error(`kzg_verifier_batch: unknown kind ${item.kind}`);
    const C = item.proof.commitments, E = item.proof.evaluations;
    const keys = Object.keys(C);
    const nFi = keys.filter(k => k.match(/^F\d/)).length;
    const nPols = nFi > 0 ? nFi : 1;
    const isVector = nPols > 1;
    const isSelected = keys.filter(k => k.match(/^selF/)).length === 1;
    if (kind === backend.LOOKUP && !isSelected) return null;
    const gs = kind !== backend.GRANDPRODUCT;
    const cNames = [], eNames = [];
    for (let i = 0; i < nPols; i++) {
        cNames.push(isVector ? `F${i}` : "F", isVector ? `T${i}` : "T");
        eNames.push(isVector ? `f${i}xi` : "fxi");
        if (gs) eNames.push(isVector ? `t${i}xi` : "txi");
    }
    if (isSelected) {
        cNames.push("selF", "selT");
        eNames.push("selFxi", "selTxi");
    }
    cNames.push(gs ? "S" : "Z", "Q", "Wxi", "Wxiw");
    eNames.push(gs ? "sxiw" : "zxiw");
    const com = new Uint8Array(64 * cNames.length), ev = new Uint8Array(32 * eNames.length);
    for (let i = 0; i < cNames.length; i++) {
        const v = C[cNames[i]];
        if (!(v instanceof Uint8Array) || v.length !== 64) return null;
        com.set(v, 64 * i);
    }
    for (let i = 0; i < eNames.length; i++) {
        const v = E[eNames[i]];
        if (!(v instanceof Uint8Array) || v.length !== 32) return null;
        ev.set(v, 32 * i);
    }
    return { kind, nbits: item.nBits, npols: nPols, selected: isSelected, commitments: com, evaluations: ev };
}

async function kzg_verifier_batch(pTauFilename, items) {
    const sent = [], refs = [];
    items.forEach((item, pos) => {
        const r = layout(item);
        if (r !== null) {
            sent.push(pos);
            refs.push(r);
        }
    });
    const verdicts = new Array(items.length).fill(false);
    let checks = 0;
    if (refs.length) {
        const ptau = require("path").resolve(pTauFilename);
        const res = await backend.withContext(slot => backend.load().verifyBatch(slot.ctx, ptau, refs));
        sent.forEach((pos, j) => { verdicts[pos] = res.valid[j] === 1; });
        checks = res.pairingChecks;
    }
    const invalid = verdicts.filter(v => !v).length;
    logger.info(`> KZG BATCH VERIFIER: ${items.length} proofs, ${invalid} invalid, ${checks} pairing checks`);
    return verdicts;
}

module.exports = kzg_verifier_batch;
module.exports.kzg_verifier_batch = kzg_verifier_batch;
