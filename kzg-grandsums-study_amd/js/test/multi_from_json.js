// Test driver used by tests/test_gpu_multi.py: read {ptau, nbits, cases:[{op: "prove", args:[{kind, F:[hex],
// T:[hex], selF, selT}]} | {op: "verify", shapes:[{kind, npols, selected}], commitments:{k:hex},
// evaluations:{k:hex}}]} from argv[2]; print {results:[{commitments:{k:hex}, evaluations:{k:hex}, verified,
// F0} | {verdict} | {error}]}.
const fs = require("fs");
const { getCurveFromName, Evaluations, mset_eq_kzg_multi_prover, mset_eq_kzg_multi_verifier } = require("../index");

(async () => {
    const spec = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const curve = await getCurveFromName("bn128");
    const hex = b => Buffer.from(b).toString("hex");
    const u8 = h => new Uint8Array(Buffer.from(h, "hex"));
    const ev = h => new Evaluations(u8(h), curve);
    const out = [];
    for (const c of spec.cases) {
        try {
            if (c.op === "verify") {
                const proof = { commitments: {}, evaluations: {} };
                for (const k of Object.keys(c.commitments)) proof.commitments[k] = u8(c.commitments[k]);
                for (const k of Object.keys(c.evaluations)) proof.evaluations[k] = u8(c.evaluations[k]);
                out.push({ verdict: await mset_eq_kzg_multi_verifier(spec.ptau, proof, spec.nbits, c.shapes) });
                continue;
            }
            const args = c.args.map(a => {
                const F = a.F.map(ev), T = a.T.map(ev);
                return { kind: a.kind, evalsFs: F.length === 1 ? F[0] : F, evalsTs: T.length === 1 ? T[0] : T,
                         evalsSelF: a.selF ? ev(a.selF) : null, evalsSelT: a.selT ? ev(a.selT) : null };
            });
            const proof = await mset_eq_kzg_multi_prover(spec.ptau, args);
            const o = { commitments: {}, evaluations: {} };
            for (const k of Object.keys(proof.commitments)) o.commitments[k] = hex(proof.commitments[k]);
            for (const k of Object.keys(proof.evaluations)) o.evaluations[k] = hex(proof.evaluations[k]);
            o.verified = await mset_eq_kzg_multi_verifier(spec.ptau, proof, spec.nbits);
            const first = Array.isArray(args[0].evalsFs) ? args[0].evalsFs[0] : args[0].evalsFs;
            o.F0 = hex(first.eval);  // still the caller's standard form
            out.push(o);
        } catch (e) {
            out.push({ error: e.message, kgsCode: e.kgsCode === undefined ? null : e.kgsCode });
        }
    }
    console.log(JSON.stringify({ results: out }));
})().catch(e => { console.error(e); process.exit(1); });
