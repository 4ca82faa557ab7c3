// Test driver used by tests/test_gpu_verify_batch.py: read {ptau, cases:[{kind, nbits, commitments:{k:hex},
// evaluations:{k:hex}}]} from argv[2], run kzg_verifier_batch once on all of them, print {verdicts:[bool]}.
const fs = require("fs");
const { kzg_verifier_batch } = require("../index");

(async () => {
    const spec = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const u8 = h => new Uint8Array(Buffer.from(h, "hex"));
    const items = spec.cases.map(c => {
        const proof = { commitments: {}, evaluations: {} };
        for (const k of Object.keys(c.commitments)) proof.commitments[k] = u8(c.commitments[k]);
        for (const k of Object.keys(c.evaluations)) proof.evaluations[k] = u8(c.evaluations[k]);
        return { kind: c.kind, proof, nBits: c.nbits };
    });
    const verdicts = await kzg_verifier_batch(spec.ptau, items);
    console.log(JSON.stringify({ verdicts }));
})().catch(e => { console.error(e); process.exit(1); });
