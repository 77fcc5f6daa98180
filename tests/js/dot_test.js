'use strict';
// Ciphertext inner product of the FHEEngine surface on the GPU: dotProduct
// (one fused dotAsync launch, fhe_ct_dot_ptrs) and the lazily relinearised
// tallyWeightedVotes(..., { relinearize: 'once' }).
//   node tests/js/dot_test.js
const assert = require('assert');
const path = require('path');

const ROOT = path.join(__dirname, '..', '..');
const fhe = require(path.join(ROOT, 'node-fhe-accelerate_amd', 'lib'));

let passed = 0;
async function test(name, fn) {
  await fn();
  passed += 1;
  console.log('ok -', name);
}
async function rejects(p, code, re) {
  let err;
  try { await p; } catch (e) { err = e; }
  assert.ok(err, `expected a rejection (${code})`);
  assert.ok(err instanceof fhe.FHEError, `FHEError expected, got ${err && err.constructor && err.constructor.name}: ${err}`);
  assert.strictEqual(err.code, code, err.message);
  if (re) assert.ok(re.test(err.message), err.message);
}
const wordsOf = async (eng, ct) => {
  const s = await eng.serializeCiphertext(ct);
  const b = Buffer.from(s.data);
  return b.slice(52 + b.readUInt32LE(48)).toString('hex');
};

// The weighted tally's parameters (tests/js/tally_test.js): the reference's
// multiply is the plain tensor product, which decodes to the plaintext
// product for q = j t^2 + t + 1, noise-free encryption and relinearisation
// digits that cover all of c2.
const T = 2048n, Q = 2305843009276610561n;
async function weightedEngine() {
  const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [Q], securityLevel: 128, plaintextModulus: T,
    decompBaseLog: 16, decompLevel: 4 }, { seed: 9n, mode: 'negacyclic' });
  const sk = await eng.generateSecretKey(), pk = await eng.generatePublicKey(sk);
  const ek = await eng.generateEvalKey(sk);
  return { eng, sk, pk, ek };
}

async function main() {
  await test('the addon and the engine export the dot surface', async () => {
    for (const m of ['dot', 'dotAsync']) assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    assert.strictEqual(typeof fhe.FHEEngineImpl.prototype.dotProduct, 'function');
  });

  await test('dotProduct over 5 pairs (one repeated, one square): words of the multiply/add chain, budget, progress', async () => {
    const { eng, sk, pk, ek } = await weightedEngine();
    const xs = [1n, 0n, 1n, 2n], ys = [3n, 5n, 7n, 11n];
    const a = [], b = [];
    for (const x of xs) a.push(await eng.encryptValue(x, pk));
    for (const y of ys) b.push(await eng.encryptValue(y, pk));
    const A = [a[0], a[1], a[2], a[1], a[3]], B = [b[0], b[1], b[2], b[1], a[3]];
    const seen = [];
    const d = await eng.dotProduct(A, B, (p) => seen.push([p.stage, p.current, p.total]));
    assert.deepStrictEqual(seen, [1, 2, 3, 4, 5].map((k) => ['dot_product', k, 5]));
    assert.strictEqual(d.degree, 2);
    assert.strictEqual(d.isNtt, false);
    assert.strictEqual(d.keyId, sk.keyId);
    let chain = await eng.multiply(A[0], B[0]);
    const first = chain.noiseBudget;
    for (let i = 1; i < A.length; i++) chain = await eng.add(chain, await eng.multiply(A[i], B[i]));
    assert.strictEqual(await wordsOf(eng, d), await wordsOf(eng, chain));
    // multiply's rule per pair (min - (log2 n + 5)), then the tree ((0 1)(2 3)) 4: -1 per level
    assert.strictEqual(first, a[0].noiseBudget - 15);
    assert.strictEqual(d.noiseBudget, first - 3);
    const got = await eng.decrypt(await eng.relinearize(d, ek), sk);
    assert.strictEqual(got.success, true);
    assert.strictEqual(got.plaintext.values[0], (1n * 3n + 0n * 5n + 1n * 7n + 0n * 5n + 2n * 2n) % T);
    // one pair: the product
    const one = await eng.dotProduct([a[3]], [b[3]]);
    assert.strictEqual(await wordsOf(eng, one), await wordsOf(eng, await eng.multiply(a[3], b[3])));
    assert.strictEqual(one.noiseBudget, first);
  });

  await test("tallyWeightedVotes { relinearize: 'once' } decrypts to sum w_i b_i; default words unchanged", async () => {
    const { eng, sk, pk, ek } = await weightedEngine();
    const bs = [1n, 0n, 1n], ws = [3n, 5n, 7n];
    const ballots = [], weights = [];
    for (const x of bs) ballots.push(await eng.encryptValue(x, pk));
    for (const x of ws) weights.push(await eng.encryptValue(x, pk));
    const want = bs.reduce((acc, x, i) => acc + x * ws[i], 0n) % T;
    const seenOnce = [], seenEach = [];
    const once = await eng.tallyWeightedVotes(ballots, weights, ek, (p) => seenOnce.push([p.stage, p.current, p.total]),
      { relinearize: 'once' });
    const each = await eng.tallyWeightedVotes(ballots, weights, ek, (p) => seenEach.push([p.stage, p.current, p.total]));
    assert.deepStrictEqual(seenOnce, seenEach);
    assert.deepStrictEqual(seenEach.map((s) => s.slice(1)), [[4, 5], [5, 5]]);
    assert.strictEqual(once.degree, 1);
    const d = await eng.decrypt(once, sk);
    assert.strictEqual(d.success, true);
    assert.strictEqual(d.plaintext.values[0], want);
    const dot = await eng.dotProduct(ballots, weights);
    assert.strictEqual(once.noiseBudget, dot.noiseBudget - 1);
    assert.strictEqual(await wordsOf(eng, once), await wordsOf(eng, await eng.relinearize(dot, ek)));
    // the default: op for op the reference's fold, with or without an options object
    const parts = [];
    for (let i = 0; i < 3; i++) parts.push(await eng.relinearize(await eng.multiply(ballots[i], weights[i]), ek));
    const ref = await eng.add(await eng.add(parts[0], parts[1]), parts[2]);
    assert.strictEqual(await wordsOf(eng, each), await wordsOf(eng, ref));
    assert.strictEqual(each.noiseBudget, Math.min(Math.min(parts[0].noiseBudget, parts[1].noiseBudget) - 1, parts[2].noiseBudget) - 1);
    for (const o of [{}, { relinearize: 'each' }]) {
      const r = await eng.tallyWeightedVotes(ballots, weights, ek, undefined, o);
      assert.strictEqual(await wordsOf(eng, r), await wordsOf(eng, ref));
      assert.strictEqual(r.noiseBudget, each.noiseBudget);
    }
    assert.strictEqual((await eng.decrypt(each, sk)).plaintext.values[0], want);
    await rejects(eng.tallyWeightedVotes(ballots, weights, ek, undefined, { relinearize: 'never' }), 'INVALID_PARAMETERS', /relinearize/);
  });

  await test('argument errors', async () => {
    const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [132120577n], securityLevel: 128, plaintextModulus: 16n },
      { seed: 7n });
    const skA = await eng.generateSecretKey(), skB = await eng.generateSecretKey();
    const pkA = await eng.generatePublicKey(skA), pkB = await eng.generatePublicKey(skB);
    const a = await eng.encryptValue(5n, pkA), a2 = await eng.encryptValue(1n, pkA), b = await eng.encryptValue(6n, pkB);
    await rejects(eng.dotProduct([a, a2], [a]), 'INVALID_PARAMETERS', /Ballots and weights must have the same size/);
    await rejects(eng.dotProduct([], []), 'INVALID_PARAMETERS', /Cannot tally empty ballot list/);
    await rejects(eng.dotProduct([a], [b]), 'KEY_MISMATCH', /Cannot multiply ciphertexts encrypted with different keys/);
    await rejects(eng.dotProduct([a, b], [a2, b]), 'KEY_MISMATCH', /Cannot add ciphertexts encrypted with different keys/);
    await rejects(eng.dotProduct([a, { __brand: 'Ciphertext' }], [a2, a]), 'INVALID_PARAMETERS', /handle/);
    const d2 = await eng.multiply(a, a2);
    await rejects(eng.dotProduct([a, d2], [a2, a]), 'INVALID_PARAMETERS', /degree-1/);
    for (const o of [undefined, { relinearize: 'once' }]) {
      await rejects(eng.tallyWeightedVotes([a, a2], [a], null, undefined, o), 'INVALID_PARAMETERS', /Ballots and weights must have the same size/);
      await rejects(eng.tallyWeightedVotes([], [], null, undefined, o), 'INVALID_PARAMETERS', /Cannot tally empty ballot list/);
    }
    // the addon's own argument checks
    const ctx = eng.context, buf = eng.deviceBuffer(a), buf2 = eng.deviceBuffer(a2), out = new fhe.DeviceBuffer(ctx, 3072);
    assert.throws(() => ctx.dot([], [], out), /Cannot tally empty ballot list/);
    assert.throws(() => ctx.dot([buf, buf2], [buf], out), /Ballots and weights must have the same size/);
    assert.throws(() => ctx.dot([buf], [buf2], new fhe.DeviceBuffer(ctx, 2048)), /degree-2/);
    assert.throws(() => ctx.dot([buf], [new fhe.DeviceBuffer(ctx, 3072)], out), /2 n words/);
    assert.throws(() => ctx.dot([buf], [buf2], new BigUint64Array(3072)), /DeviceBuffers of this context/);
    const prod = ctx.ctMultiply(buf, buf2, new fhe.DeviceBuffer(ctx, 3072));
    const sq = ctx.ctMultiply(buf, buf, new fhe.DeviceBuffer(ctx, 3072));
    assert.deepStrictEqual(ctx.dot([buf, buf], [buf2, buf], out).download(), ctx.add(prod, sq, new fhe.DeviceBuffer(ctx, 3072)).download());
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
