// Device backend: a pool of libkgs contexts spread over the visible HIP devices.
//
// The reference prover is an independent async function per call
// (src/grandsum/mset_eq_kzg_prover.js:12): `Promise.all([prover(a), prover(b)])` runs both. Here
// every call takes a context slot for its whole duration (SRS load + prove), so a context is never
// used by two calls at once, and independent calls run concurrently on different contexts (each
// with its own HIP stream and buffers, on the same GPU or on another one). libkgs additionally
// serialises calls per context with a mutex, and shares the read-only SRS / NTT tables between the
// contexts of a device, so a pool of several contexts costs one set of tables per GPU.
//
// Knobs: KGS_JS_CONTEXTS = contexts per device (default 8: with 16 concurrent calls, 8 contexts
// reach 82 proofs/s at n = 2^20 against 78.5 with 4, profiles/r02/js_adaptive_lanes.txt), KGS_DEVICES = comma-separated device list (default: every visible device),
// KGS_JS_SHARD_RANKS / KGS_JS_SHARD_MIN_NBITS = one large proof over several GPUs (below).
const fs = require("fs");
const path = require("path");
const { contiguous } = require("./bigbuffer");

// N-API async work runs on the libuv thread pool (4 threads by default): one thread per context of
// an 8-GPU pool needs more. Effective only if set before the process first uses the pool.
if (!process.env.UV_THREADPOOL_SIZE) process.env.UV_THREADPOOL_SIZE = "64";

let addon = null;
function load() {
    if (!addon) {
        const p = process.env.KGS_ADDON || path.join(__dirname, "..", "build", "kgs_addon.node");
        addon = require(p);  // no CPU fallback: the HIP library is the only path
    }
    return addon;
}

function devices() {
    const env = process.env.KGS_DEVICES;
    if (env && env.trim() !== "") return env.split(",").map(x => parseInt(x, 10)).filter(x => x >= 0);
    const n = load().deviceCount();
    if (n < 1) throw new Error("no HIP device visible");
    return Array.from({ length: n }, (_, i) => i);
}

function perDevice() {
    const v = parseInt(process.env.KGS_JS_CONTEXTS || "8", 10);
    return Number.isFinite(v) && v >= 1 ? v : 8;
}

const pool = { slots: [], idle: [], waiters: [], devs: null, cap: 0 };
const diag = { execMs: null, timing: null, waitMs: null, callMs: null };

function newSlot() {
    if (!pool.devs) {
        pool.devs = devices();
        pool.cap = pool.devs.length * perDevice();
    }
    // round-robin over devices: slot i lives on device devs[i % ndev]
    const device = pool.devs[pool.slots.length % pool.devs.length];
    const slot = { device, ctx: load().ctxCreate(device), index: pool.slots.length, busy: false, lanes: 2 };
    pool.slots.push(slot);
    return slot;
}

function acquire() {
    if (pool.idle.length) return Promise.resolve(pool.idle.pop());
    if (!pool.devs || pool.slots.length < pool.cap) return Promise.resolve(newSlot());
    return new Promise(resolve => pool.waiters.push(resolve));
}

function release(slot) {
    const w = pool.waiters.shift();
    if (w) w(slot);
    else pool.idle.push(slot);
}

// run fn(slot) with exclusive use of one context
async function withContext(fn) {
    const slot = await acquire();
    slot.busy = true;
    try {
        return await fn(slot);
    } finally {
        slot.busy = false;
        release(slot);
    }
}

// Eager collection beside a lone proof: OPT-IN (KGS_JS_EAGER_GC=1, or =<ms> for the delay), and only
// in an application that itself started Node with --expose-gc (the library never changes V8 flags).
// Why it exists: every proof leaves the caller's previous input buffers (the reference replaces
// Evaluations.eval by the Montgomery copy, prover.js:147-148) as 64 MiB of garbage at n = 2^20; V8
// then finalises a ~6 ms mark-sweep as a main-thread task, which, scheduled while the GPU works, tended
// to run just as the proof completed: the Promise resolved 0.1-5 ms after the result was ready
// (profiles/r04/js/). With the opt-in, a proof alone on its device runs one full collection
// GC_DELAY_MS after it is queued, beside its ~15 ms of GPU work (not at once: freeing the garbage's
// pages while round 1 copies the next inputs into pinned staging stretched that round from 3.4 to
// 9-15 ms in a third of the samples, profiles/r04/js/run5); with other proofs in flight V8's own
// schedule is kept. A blocking full collection on the host application's main thread is its call to
// make, which is why this is off by default.
const GC_DELAY_MS = (() => {
    const v = parseInt(process.env.KGS_JS_EAGER_GC || "", 10);
    return Number.isFinite(v) && v > 1 ? v : 5;
})();
function eagerGcEnabled() {
    const v = process.env.KGS_JS_EAGER_GC;
    return v !== undefined && v !== "" && v !== "0" && typeof global.gc === "function";
}
// Only proofs whose inputs are large enough for their garbage to matter (>= 16 MiB of F / T, e.g.
// n >= 2^18 for one pair) schedule it, and at most one collection is pending at a time: small proofs
// take less than the collection itself.
const GC_MIN_BYTES = 16 << 20;
let gcPending = false;
function scheduleCollect(inputBytes) {
    if (!eagerGcEnabled() || gcPending || inputBytes < GC_MIN_BYTES) return;
    gcPending = true;
    setTimeout(() => {
        gcPending = false;
        global.gc();
    }, GC_DELAY_MS);
}

// MSM lanes of a proof about to start: two (single-proof latency mode, kgs_ctx_set_msm_lanes) when it
// is alone on its device, one when other proofs are in flight there or waiting for a context — the
// GPU is then already full, and the two-lane accumulation's register reservation would keep the
// other contexts' kernels from co-residing (DESIGN.md §3 register budget)
function setLanes(slot) {
    const others = pool.slots.some(s => s !== slot && s.busy && s.device === slot.device);
    const lanes = others || pool.waiters.length > 0 ? 1 : 2;
    if (slot.lanes !== lanes) {
        load().ctxSetMsmLanes(slot.ctx, lanes);
        slot.lanes = lanes;
    }
}

// ptau header power, read without a context (readPTauHeader, src/ptau_utils.js:3-24)
function ptauPower(pTauFilename) {
    return load().ptauPower(path.resolve(pTauFilename));
}

// The SRS of `key` for domains up to 2^nBits on the slot's context. The load is an async job (a libuv
// thread round trip) even when libkgs finds its tables already resident; it is skipped when this context
// loaded the same file (same real path, size and mtime — the identity libkgs checks, so a rewritten ptau
// is still re-read) for >= nBits (a file that cannot be stat'ed goes to libkgs, which reports it as the
// drop-in always has)
async function ensureSrs(slot, key, nBits) {
    let id = null;
    try {
        const st = fs.statSync(key, { bigint: true });
        id = `${fs.realpathSync(key)}#${st.size}#${st.mtimeNs}`;
    } catch (e) {
        id = null;
    }
    if (id === null || slot.srsId !== id || slot.srsBits < nBits) {
        slot.srsId = null;
        await load().srsLoadPtau(slot.ctx, key, nBits);
        slot.srsId = id;
        slot.srsBits = nBits;
    }
}

// SRS load (only 2^(nBits+1) points, as prover.js:83-85 reads; grow-only device cache in libkgs)
// and prove on the same held context: nothing can swap the SRS between the two
async function prove(kind, pTauFilename, nBits, evalsF, evalsT, selF, selT) {
    const key = path.resolve(pTauFilename);
    // evaluations held in a BigBuffer (Evaluations.fromPolynomial, src/polynomial/evaluations.js:12-21)
    // go to the native side as one contiguous copy
    evalsF = evalsF.map(contiguous);
    evalsT = evalsT.map(contiguous);
    if (selF) selF = contiguous(selF);
    if (selT) selT = contiguous(selT);
    if (shardRanks() >= 2 && nBits >= shardMinBits()) return proveSharded(kind, key, nBits, evalsF, evalsT, selF, selT);
    return withContext(async slot => {
        await ensureSrs(slot, key, nBits);
        setLanes(slot);
        const t0 = process.hrtime.bigint();
        const pending = load().prove(slot.ctx, kind, nBits, evalsF, evalsT, selF, selT);
        if (slot.lanes === 2) {  // alone on its device: see scheduleCollect (opt-in)
            scheduleCollect(evalsF.concat(evalsT).reduce((a, e) => a + e.length, 0));
        }
        const res = await pending;
        // diagnostics of the last call: the native call's wall time, its [queue -> worker, worker ->
        // completion] waits, time inside libkgs, kgs_last_timing rounds / copy / prover / write-back
        diag.callMs = Number(process.hrtime.bigint() - t0) / 1e6;
        diag.waitMs = res.waitMs;
        diag.execMs = res.execMs;
        diag.timing = load().lastTiming(slot.ctx);
        return res;
    });
}

// One proof of several arguments (kgs_prove_multi) on one held context; args: [{kind, F: [..], T: [..],
// selF|null, selT|null}]. No Montgomery write-back, always one GPU (rank groups do not take it).
async function proveMulti(pTauFilename, nBits, args) {
    const key = path.resolve(pTauFilename);
    args = args.map(a => ({ kind: a.kind, F: a.F.map(contiguous), T: a.T.map(contiguous),
                            selF: a.selF ? contiguous(a.selF) : null, selT: a.selT ? contiguous(a.selT) : null }));
    return withContext(async slot => {
        await ensureSrs(slot, key, nBits);
        setLanes(slot);
        return load().proveMulti(slot.ctx, nBits, args);
    });
}

// The commitment to the polynomial with the 2^k standard-form evaluations `evals` (an Evaluations, a
// Uint8Array or a BigBuffer), over the SRS of pTauFilename (kgs_commit_evals: the Lagrange bases are
// built on the GPU on first use and cached on the device) -> Promise<64 B affine LEM>
async function commitEvals(pTauFilename, evals) {
    const key = path.resolve(pTauFilename);
    const e = contiguous(evals && evals.eval !== undefined ? evals.eval : evals);
    const n = e.byteLength / 32;
    if (!Number.isInteger(n) || n < 1 || (n & (n - 1)) !== 0) {
        throw new Error("commit_evals: the evaluations must be a power of two of 32-byte elements");
    }
    const nBits = Math.round(Math.log2(n));
    return withContext(async slot => {
        await ensureSrs(slot, key, nBits);
        return load().commitEvals(slot.ctx, e);
    });
}

// Every opening of the polynomial with the Montgomery coefficients `coefs` (a Uint8Array or a BigBuffer of
// 32-byte elements) on the smallest domain 2^k that holds them, over the SRS of pTauFilename
// (kgs_kzg_open_all, FK20: O(n log n) group operations; the SRS side is cached on the device)
// -> Promise<{proofs: 2^k x 64 B affine LEM, evals: 2^k x 32 B Montgomery}>, entry i for Fr.w[k]^i
async function kzgOpenAll(pTauFilename, coefs) {
    const key = path.resolve(pTauFilename);
    const c = contiguous(coefs);
    const n = c.byteLength / 32;
    if (!Number.isInteger(n) || n > (1 << 23)) {
        throw new Error("kzg_open_all: the coefficients must be at most 2^23 32-byte elements");
    }
    const nBits = n > 1 ? Math.ceil(Math.log2(n)) : 0;
    return withContext(async slot => {
        await ensureSrs(slot, key, nBits);
        return load().kzgOpenAll(slot.ctx, c);
    });
}

// Every coset opening of the polynomial with the Montgomery coefficients `coefs` (a Uint8Array or a BigBuffer
// of 32-byte elements): the domain is the smallest 2^k that holds them (and at least 2^lBits points), a coset
// has 2^lBits points, over the SRS of pTauFilename (kgs_kzg_open_cosets; the SRS side is cached on the device)
// -> Promise<{proofs: 2^(k - lBits) x 64 B affine LEM, evals: 2^k x 32 B Montgomery}>; proof i covers the
// values evals[i + 2^(k - lBits) j], j < 2^lBits
async function kzgOpenCosets(pTauFilename, coefs, lBits) {
    const key = path.resolve(pTauFilename);
    const c = contiguous(coefs);
    const n = c.byteLength / 32;
    if (!Number.isInteger(n) || n > (1 << 23) || !Number.isInteger(lBits) || lBits < 0 || lBits > 23) {
        throw new Error("kzg_open_cosets: the coefficients must be at most 2^23 32-byte elements, lBits in 0 .. 23");
    }
    const nBits = Math.max(n > 1 ? Math.ceil(Math.log2(n)) : 0, lBits);
    return withContext(async slot => {
        await ensureSrs(slot, key, nBits);
        return load().kzgOpenCosets(slot.ctx, c, nBits, lBits);
    });
}

// kzgOpenCosets for many polynomials in one call (kgs_kzg_open_cosets_many: every stage runs once for the whole
// set, so small polynomials share the latency one call pays alone). coefsList: an array of Uint8Arrays / BigBuffers
// of Montgomery coefficients; the domain is the smallest 2^k that holds the longest (and at least 2^lBits points),
// shorter ones are zero-padded, which changes no proof; coefsList.length * 2^k <= 2^24
// -> Promise<{proofs: [2^(k - lBits) x 64 B ..], evals: [2^k x 32 B ..]}>, entry b what kzgOpenCosets gives for
// polynomial b on that domain
async function kzgOpenCosetsMany(pTauFilename, coefsList, lBits) {
    const key = path.resolve(pTauFilename);
    if (!Array.isArray(coefsList) || !Number.isInteger(lBits) || lBits < 0 || lBits > 23) {
        throw new Error("kzg_open_cosets_many: expected an array of coefficient buffers and lBits in 0 .. 23");
    }
    if (coefsList.length === 0) return { proofs: [], evals: [] };
    const cs = coefsList.map(c => contiguous(c));
    const n =cs.reduce((a, c) => Math.max(a, c.byteLength / 32), 0);
    if (cs.some(c => c.byteLength % 32 !== 0) || n > (1 << 23)) {
        throw new Error("kzg_open_cosets_many: the coefficients must be at most 2^23 32-byte elements");
    }
    const nBits = Math.max(n > 1 ? Math.ceil(Math.log2(n)) : 0, lBits);
    if (cs.length * 2 ** nBits > 2 ** 24) {
        throw new Error("kzg_open_cosets_many: polys * 2^nBits must be at most 2^24");
    }
    const packed = new Uint8Array(32 * n * cs.length);
    cs.forEach((c, b) => packed.set(c, 32 * n * b));
    return withContext(async slot => {
        await ensureSrs(slot, key, nBits);
        const r = await load().kzgOpenCosetsMany(slot.ctx, packed, cs.length, nBits, lBits);
        const ps = 64 * 2 ** (nBits - lBits), es = 32 * 2 ** nBits;
        return {
            proofs: cs.map((_, b) => r.proofs.subarray(ps * b, ps * (b + 1))),
            evals: cs.map((_, b) => r.evals.subarray(es * b, es * (b + 1))),
        };
    });
}

// The check of one coset opening on the host (kgs_kzg_verify_coset) -> bool. commit / proof: 64 B affine LEM;
// ysMont: the coset's 2^lBits values, 32 B Montgomery each; srsG1: the first 2^lBits points [tau^k]_1, 64 B
// affine LEM each; tauLG2: [tau^(2^lBits)]_2, 128 B LEM
function kzgVerifyCoset(commit, nBits, lBits, index, ysMont, proof, srsG1, tauLG2) {
    return load().kzgVerifyCoset(contiguous(commit), nBits, lBits, index, contiguous(ysMont), contiguous(proof),
        contiguous(srsG1), contiguous(tauLG2));
}

// Many coset openings against one SRS with one pairing check (kgs_kzg_verify_cosets_batch)
// -> Promise<{valid: [bool ..], pairingChecks, onGpu, hashMs, foldMs, pairingMs}>. commits: an array of 64 B affine
// LEM commitments; openings: an array of {commit (an index into commits), index (the coset), ys (2^lBits x 32 B
// Montgomery), proof (64 B affine LEM)}; srsG1: the first 2^lBits points [tau^k]_1; tauLG2: [tau^(2^lBits)]_2,
// 128 B LEM. opts.host computes on the host (no GPU), else the folds run on a pooled context's GPU; opts.seed:
// 32 bytes that replace the hash of the batch as the source of the weights (they must be unpredictable to
// whoever made the proofs). An opening with ys or proof of the wrong length is false without reaching the library.
async function kzgVerifyCosetsBatch(commits, nBits, lBits, openings, srsG1, tauLG2, opts) {
    opts = opts || {};
    const cm = Buffer.concat(commits.map(c => Buffer.from(contiguous(c))));
    const sent = [];
    openings.forEach((o, k) => {
        if (contiguous(o.ys).byteLength === 32 * 2 ** lBits && contiguous(o.proof).byteLength === 64) sent.push(k);
    });
    const ys = Buffer.concat(sent.map(k => Buffer.from(contiguous(openings[k].ys))));
    const proofs = Buffer.concat(sent.map(k => Buffer.from(contiguous(openings[k].proof))));
    const args = [nBits, lBits, new Uint8Array(cm), sent.map(k => openings[k].commit), sent.map(k => openings[k].index),
        new Uint8Array(ys), new Uint8Array(proofs), contiguous(srsG1), contiguous(tauLG2),
        opts.seed ? contiguous(opts.seed) : null];
    const res = opts.host ? await load().kzgVerifyCosetsBatch(null, ...args)
        : await withContext(slot => load().kzgVerifyCosetsBatch(slot.ctx, ...args));
    const valid = openings.map(() => false);
    sent.forEach((k, j) => { valid[k] = res.valid[j] === 1; });
    return Object.assign(res, { valid });
}

// A polynomial of `length` coefficients back from a subset of its cosets (kgs_kzg_recover_cosets; needs no SRS)
// -> Promise<{ok, coefs: length x 32 B Montgomery, evals: 2^nBits x 32 B Montgomery}>. cells: an array of {index (the
// coset, < 2^(nBits - lBits), each at most once), ys (its 2^lBits values p(w^(index + 2^(nBits - lBits) j)), 32 B
// Montgomery each)}, in any order, with cells.length * 2^lBits >= length. ok is false when the values lie on no
// polynomial of degree < length; coefs and evals mean nothing then.
async function kzgRecoverCosets(nBits, lBits, cells, length) {
    const ys = Buffer.concat(cells.map(c => Buffer.from(contiguous(c.ys))));
    return withContext(slot => load().kzgRecoverCosets(slot.ctx, nBits, lBits, cells.map(c => c.index),
        new Uint8Array(ys), length));
}

// `polys` polynomials of `length` coefficients each back from their cells in one call (kgs_kzg_recover_cosets_many;
// needs no SRS) -> Promise<{status: polys bytes (1 recovered, 0 the cells lie on no polynomial of degree < length,
// 2 fewer than ceil(length / 2^lBits) cells), coefs: polys x length x 32 B Montgomery, evals: polys x 2^nBits x 32 B
// Montgomery}>. cells: an array of {poly (< polys), index (the coset, each at most once per polynomial), ys (its
// 2^lBits values)}, in any order: the batch verifier's openings with `commit` as `poly`. The bytes of a polynomial
// whose status is not 1 mean nothing.
async function kzgRecoverCosetsMany(nBits, lBits, cells, length, polys) {
    const ys = Buffer.concat(cells.map(c => Buffer.from(contiguous(c.ys))));
    return withContext(slot => load().kzgRecoverCosetsMany(slot.ctx, nBits, lBits, cells.map(c => c.poly),
        cells.map(c => c.index), new Uint8Array(ys), length, polys));
}

// Large proofs over several GPUs from this one Node process: with KGS_JS_SHARD_RANKS = W >= 2, a
// proof of at least 2^KGS_JS_SHARD_MIN_NBITS elements (default 22) runs on W contexts (rank r on
// device r mod #devices) joined by an in-process rank group (kgs_group_create_local +
// kgs_ctx_set_group): every vector of the proof sharded, NTTs as rank-local transforms plus one
// all-to-all, every MSM over the rank's slice of the SRS, which is all a rank loads
// (kgs_srs_load_ptau_slice; DESIGN.md §6). The W ranks run as ONE async job that starts one native
// thread per rank (addon proveGroup), so they never wait for libuv pool threads held by other work;
// rank 0 returns the proof and the Montgomery write-back. One sharded proof at a time (the group's
// barriers join the ranks of one proof); the same inputs and the same Promise result as the
// single-GPU path.
const shard = { ctxs: null, group: null, busy: Promise.resolve() };
function shardRanks() {
    const v = parseInt(process.env.KGS_JS_SHARD_RANKS || "0", 10);
    return Number.isFinite(v) ? v : 0;
}
function shardMinBits() {
    const v = parseInt(process.env.KGS_JS_SHARD_MIN_NBITS || "22", 10);
    return Number.isFinite(v) ? v : 22;
}
function proveSharded(kind, key, nBits, evalsF, evalsT, selF, selT) {
    const a = load();
    const W = shardRanks();
    const run = async () => {
        if (!shard.ctxs || shard.ctxs.length !== W) {
            const devs = devices();
            shard.ctxs = Array.from({ length: W }, (_, r) => a.ctxCreate(devs[r % devs.length]));
            shard.group = null;
        }
        if (!shard.group) {
            shard.group = a.groupCreateLocal(W);
            shard.ctxs.forEach((c, r) => a.ctxSetGroup(c, shard.group, r));
        }
        try {
            return await a.proveGroup(shard.ctxs, key, kind, nBits, evalsF, evalsT, selF, selT);
        } catch (e) {
            // a rank failed: the group may be spent (the others were released with an error); make a
            // fresh one for the next proof
            shard.ctxs.forEach(c => a.ctxSetGroup(c, null, 0));
            shard.group = null;
            throw e;
        }
    };
    const p = shard.busy.then(run, run);
    shard.busy = p.catch(() => {});
    return p;
}

function poolInfo() {
    return { contexts: pool.slots.length, capacity: pool.cap, devices: pool.devs ? pool.devs.slice() : null,
             idle: pool.idle.length, waiting: pool.waiters.length };
}

module.exports = { load, ptauPower, prove, proveMulti, commitEvals, kzgOpenAll, kzgOpenCosets, kzgOpenCosetsMany, kzgVerifyCoset, kzgVerifyCosetsBatch, kzgRecoverCosets, kzgRecoverCosetsMany, withContext, poolInfo, diag, GRANDSUM: 0, GRANDPRODUCT: 1, LOOKUP: 2 };
