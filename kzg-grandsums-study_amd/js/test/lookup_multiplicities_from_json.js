// Test driver used by tests/test_lookup_multiplicities.py: read
// {ptau, cases:[{op: "mul" | "prove", F:[hex], T:[hex], selF: hex | null}]} from argv[2] and print
// {results:[...]}: "mul" runs lookup_multiplicities -> {m: hex, F:[hex] (the inputs afterwards)},
// "prove" runs lookup_kzg_grandsum_prover_from_table -> {commitments, evaluations}; a rejection gives
// {error, kgsCode}.
const fs = require("fs");
const { getCurveFromName, Evaluations, lookup_multiplicities, lookup_kzg_grandsum_prover_from_table } = require("../index");

(async () => {
    const spec = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const curve = await getCurveFromName("bn128");
    const hex = b => Buffer.from(b).toString("hex");
    const ev = h => new Evaluations(new Uint8Array(Buffer.from(h, "hex")), curve);
    const results = [];
    for (const c of spec.cases) {
        const F = c.F.map(ev), T = c.T.map(ev);
        const selF = c.selF ? ev(c.selF) : null;
        try {
            if (c.op === "mul") {
                const m = await lookup_multiplicities(F.length === 1 ? F[0] : F, T.length === 1 ? T[0] : T, selF);
                results.push({ m: hex(m.eval), F: F.map(e => hex(e.eval)), T: T.map(e => hex(e.eval)) });
            } else {
                const proof = await lookup_kzg_grandsum_prover_from_table(spec.ptau, F.length === 1 ? F[0] : F,
                    T.length === 1 ? T[0] : T, selF);
                const o = { commitments: {}, evaluations: {} };
                for (const k of Object.keys(proof.commitments)) o.commitments[k] = hex(proof.commitments[k]);
                for (const k of Object.keys(proof.evaluations)) o.evaluations[k] = hex(proof.evaluations[k]);
                results.push(o);
            }
        } catch (e) {
            results.push({ error: e.message, kgsCode: e.kgsCode === undefined ? null : e.kgsCode });
        }
    }
    console.log(JSON.stringify({ results }));
})().catch(e => { console.error(e); process.exit(1); });
