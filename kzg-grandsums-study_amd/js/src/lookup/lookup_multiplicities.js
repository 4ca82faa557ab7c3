// Multiplicities of a lookup table, computed on the GPU (include/kgs.h kgs_lookup_multiplicities):
//   lookup_multiplicities(evalsFs, evalsTs, evalsSelF = null) -> Promise<Evaluations>
// evalsFs / evalsTs: one Evaluations or an array of k (the columns of the witness and of the table), in
// STANDARD form as the provers take them; evalsSelF: the Montgomery zero / one selector of the witness
// rows (all rows when omitted). The result holds, for every table row, how many selected witness rows
// equal it (Montgomery): the evalsMulT of lookup_kzg_grandsum_prover. A table row that occurs several
// times gets all of its count at its first occurrence. The inputs are read, not modified: they are
// still standard form afterwards. A selected row that is in no table row rejects with
// "Row <i> of F is not in the table." (the lowest such row).
//   lookup_kzg_grandsum_prover_from_table(pTauFilename, evalsFs, evalsTs, evalsSelF = null)
// chains the two calls.
const backend = require("../backend");
const { contiguous } = require("../bigbuffer");
const { Evaluations } = require("../polynomial/evaluations");
const lookup_kzg_grandsum_prover = require("./lookup_kzg_prover");

async function lookup_multiplicities(evalsFs, evalsTs, evalsSelF = null) {
    // the provers' list and length checks, with their messages (prover_common.js)
    if (!Array.isArray(evalsFs)) evalsFs = [evalsFs];
    if (!Array.isArray(evalsTs)) evalsTs = [evalsTs];
    if (evalsFs.length !== evalsTs.length) throw new Error(`The lengths of the two vector multisets must be the same.`);
    const nPols = evalsFs.length;
    if (nPols === 0) throw new Error(`The number of multisets must be greater than 0.`);
    for (let i = 0; i < nPols; i++) {
        if (evalsFs[i].length() !== evalsTs[i].length()) {
            throw new Error(`The ${i}-th multiset buffers must have the same length.`);
        } else if (evalsFs[i].length() !== evalsFs[0].length()) {
            throw new Error("The multiset buffers must all have the same length.");
        }
    }
    const noSelF = evalsSelF === null || evalsSelF === undefined;
    if (!noSelF && evalsSelF.length() !== evalsFs[0].length()) {
        throw new Error("The selection buffers must have the same length as the multiset buffers.");
    }
    if (evalsFs[0].length() === 0) throw new Error("The multiset buffers must not be empty.");
    const F = evalsFs.map(e => contiguous(e.eval));
    const T = evalsTs.map(e => contiguous(e.eval));
    const selF = noSelF ? null : contiguous(evalsSelF.eval);
    const m = await backend.withContext(slot => backend.load().lookupMultiplicities(slot.ctx, F, T, selF));
    return new Evaluations(m, evalsFs[0].curve);
}

async function lookup_kzg_grandsum_prover_from_table(pTauFilename, evalsFs, evalsTs, evalsSelF = null) {
    const evalsMulT = await lookup_multiplicities(evalsFs, evalsTs, evalsSelF);
    return lookup_kzg_grandsum_prover(pTauFilename, evalsFs, evalsTs, evalsSelF, evalsMulT);
}

module.exports = lookup_multiplicities;
module.exports.lookup_multiplicities = lookup_multiplicities;
module.exports.lookup_kzg_grandsum_prover_from_table = lookup_kzg_grandsum_prover_from_table;
