// Multi-argument prover (include/kgs.h kgs_prove_multi; DESIGN.md §16): ONE proof of several arguments
// over one domain, which share their challenges, one quotient and one pair of opening proofs.
//   args: 1 .. 16 objects { kind: "grandsum" | "grandproduct" | "lookup", evalsFs, evalsTs,
//         evalsSelF = null, evalsSelT = null } with the Evaluations the single provers take (a lookup's
//         multiplicities in evalsSelT)
// Every argument passes the single provers' input checks (prover_common.js, same messages prefixed with
// "argument <j>: "). The inputs are left as they are (no Montgomery write-back). The proof object uses the
// single provers' names for one argument and, for more, the same names prefixed with "A<j>." (A0.F,
// A1.T2, A1.selF, A0.S, A1.Z, A0.fxi, A1.zxiw); Q, Wxi and Wxiw keep their names. Insertion order is the
// C-ABI order. The proof carries its shapes in the non-enumerable member `shapes` for the verifier.
const backend = require("../backend");
const logger = require("../logger");
const { checkInputs } = require("../prover_common");
const { getCurveFromName } = require("../curve");

const KIND = { grandsum: backend.GRANDSUM, grandproduct: backend.GRANDPRODUCT, lookup: backend.LOOKUP };
const MAX_ARGS = 16;

// key order of a proof of these shapes ([{kind (number), npols, selected}]): { commitments, evaluations }
function proofNames(shapes) {
    const one = s => {
        const vec = s.npols > 1, gs = s.kind !== backend.GRANDPRODUCT;
        const c = [], e = [];
        for (let i = 0; i < s.npols; i++) {
            c.push(vec ? `F${i}` : "F", vec ? `T${i}` : "T");
            e.push(vec ? `f${i}xi` : "fxi");
            if (gs) e.push(vec ? `t${i}xi` : "txi");
        }
        if (s.selected) {
            c.push("selF", "selT");
            e.push("selFxi", "selTxi");
        }
        return { c, e, S: gs ? "S" : "Z", sxiw: gs ? "sxiw" : "zxiw" };
    };
    if (shapes.length === 1) {
        const n = one(shapes[0]);
        return { commitments: n.c.concat([n.S, "Q", "Wxi", "Wxiw"]), evaluations: n.e.concat([n.sxiw]) };
    }
    const com = [], comS = [], ev = [], evS = [];
    shapes.forEach((s, j) => {
        const n = one(s);
        com.push(...n.c.map(x => `A${j}.${x}`));
        comS.push(`A${j}.${n.S}`);
        ev.push(...n.e.map(x => `A${j}.${x}`));
        evS.push(`A${j}.${n.sxiw}`);
    });
    return { commitments: com.concat(comS, ["Q", "Wxi", "Wxiw"]), evaluations: ev.concat(evS) };
}

async function mset_eq_kzg_multi_prover(pTauFilename, args) {
    logger.info("> MULTI-ARGUMENT KZG PROVER STARTED");
    const nBitsPTau = backend.ptauPower(pTauFilename);
    const curve = await getCurveFromName("bn128");
    if (!Array.isArray(args) || args.length < 1 || args.length > MAX_ARGS) {
        throw new Error(`The number of arguments must be in 1 .. ${MAX_ARGS}.`);
    }
    const native = [], shapes = [];
    let nBits = null;
    args.forEach((a, j) => {
        const kind = typeof a.kind === "number" ? a.kind : KIND[a.kind];
        if (kind !== backend.GRANDSUM && kind !== backend.GRANDPRODUCT && kind !== backend.LOOKUP) {
            throw new Error(`argument ${j}: unknown argument kind`);
        }
        let c;
        try {
            c = checkInputs(kind, nBitsPTau, curve, a.evalsFs, a.evalsTs, a.evalsSelF, a.evalsSelT);
        } catch (e) {
            throw new Error(`argument ${j}: ${e.message}`);
        }
        if (nBits !== null && c.nBits !== nBits) throw new Error(`argument ${j}: every argument must have the domain of argument 0.`);
        nBits = c.nBits;
        native.push({ kind, F: c.evalsFs.map(e => e.eval), T: c.evalsTs.map(e => e.eval),
                      selF: c.isSelected ? c.evalsSelF.eval : null, selT: c.isSelected ? c.evalsSelT.eval : null });
        shapes.push({ kind, npols: c.nPols, selected: c.isSelected });
    });
    const res = await backend.proveMulti(pTauFilename, nBits, native);
    const names = proofNames(shapes);
    const proof = { evaluations: {}, commitments: {} };
    names.commitments.forEach((n, i) => { proof.commitments[n] = res.commitments[i]; });
    names.evaluations.forEach((n, i) => { proof.evaluations[n] = res.evaluations[i]; });
    Object.defineProperty(proof, "shapes", { value: shapes, enumerable: false });
    logger.info("> MULTI-ARGUMENT KZG PROVER FINISHED");
    return proof;
}

module.exports = mset_eq_kzg_multi_prover;
module.exports.proofNames = proofNames;
module.exports.KIND = KIND;
