'use strict';
// Public-weight tallies of the FHEEngine surface on the GPU:
// tallyScalarWeightedVotes (one sumScaledAsync launch, fhe_ct_sum_scaled_ptrs),
// dotPlain (one fused dotPlainAsync launch, fhe_ct_dot_plain_ptrs) and
// multiplyPlain on a degree-1 ciphertext, which takes the plain dot with one
// pair.
//   node tests/js/weighted_test.js
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

// The weighted tally's parameters (tests/js/tally_test.js): q = j t^2 + t + 1
// and noise-free encryption, for which the product with an encoded plaintext
// (delta^2 m w) still decodes to m w.
const T = 2048n, Q = 2305843009276610561n;
async function weightedEngine() {
  const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [Q], securityLevel: 128, plaintextModulus: T,
    decompBaseLog: 16, decompLevel: 4 }, { seed: 9n, mode: 'negacyclic' });
  const sk = await eng.generateSecretKey(), pk = await eng.generatePublicKey(sk);
  return { eng, sk, pk };
}

async function main() {
  await test('the addon and the engine export the public-weight surface', async () => {
    for (const m of ['sumScaled', 'sumScaledAsync', 'dotPlain', 'dotPlainAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    for (const m of ['tallyScalarWeightedVotes', 'dotPlain']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('tallyScalarWeightedVotes: words of the multiplyScalar/add chain, budget, progress, decryption', async () => {
    const { eng, sk, pk } = await weightedEngine();
    const bs = [1n, 0n, 1n, 2n], ws = [3n, 5n, 7n, 11n];
    const b = [];
    for (const x of bs) b.push(await eng.encryptValue(x, pk));
    const B = [b[0], b[1], b[2], b[1], b[3]], W = [ws[0], ws[1], ws[2], 9n, ws[3]];  // one ballot twice, two weights
    const seen = [];
    const t = await eng.tallyScalarWeightedVotes(B, W, (p) => seen.push([p.stage, p.current, p.total]));
    assert.deepStrictEqual(seen, [1, 2, 3, 4].map((k) => ['tally_scalar_weighted_votes', k, 4]));
    assert.strictEqual(t.degree, 1);
    assert.strictEqual(t.keyId, sk.keyId);
    let chain = await eng.multiplyScalar(B[0], W[0]);
    const first = chain.noiseBudget;
    for (let i = 1; i < B.length; i++) chain = await eng.add(chain, await eng.multiplyScalar(B[i], W[i]));
    assert.strictEqual(await wordsOf(eng, t), await wordsOf(eng, chain));
    // multiplyScalar's - 1 per ballot, then the tree ((0 1)(2 3)) 4: -1 per level
    assert.strictEqual(first, b[0].noiseBudget - 1);
    assert.strictEqual(t.noiseBudget, first - 3);
    const got = await eng.decrypt(t, sk);
    assert.strictEqual(got.success, true);
    assert.strictEqual(got.plaintext.values[0], (1n * 3n + 0n * 5n + 1n * 7n + 0n * 9n + 2n * 11n) % T);
    // ballots (1, 0, 1) under the weights (3, 5, 7)
    const small = await eng.tallyScalarWeightedVotes(b.slice(0, 3), ws.slice(0, 3));
    assert.strictEqual((await eng.decrypt(small, sk)).plaintext.values[0], 10n);
    // one ballot: the scaled ballot
    const one = await eng.tallyScalarWeightedVotes([b[3]], [ws[3]]);
    assert.strictEqual(await wordsOf(eng, one), await wordsOf(eng, await eng.multiplyScalar(b[3], ws[3])));
    assert.strictEqual(one.noiseBudget, first);
  });

  await test('dotPlain: words of the multiplyPlain/add chain, budget, progress, decryption; X^k moves the slot', async () => {
    const { eng, sk, pk } = await weightedEngine();
    const bs = [1n, 0n, 1n], ws = [3n, 5n, 7n];
    const b = [], p = [];
    for (const x of bs) b.push(await eng.encryptValue(x, pk));
    for (const w of ws) p.push(eng.createPlaintext(w));
    const B = [b[0], b[1], b[2], b[0]], P = [p[0], p[1], p[2], p[1]];  // a ballot twice, a plaintext shared
    const seen = [];
    const d = await eng.dotPlain(B, P, (q) => seen.push([q.stage, q.current, q.total]));
    assert.deepStrictEqual(seen, [1, 2, 3, 4].map((k) => ['dot_plain', k, 4]));
    assert.strictEqual(d.degree, 1);
    assert.strictEqual(d.isNtt, false);
    assert.strictEqual(d.keyId, sk.keyId);
    let chain = await eng.multiplyPlain(B[0], P[0]);
    const first = chain.noiseBudget;
    for (let i = 1; i < B.length; i++) chain = await eng.add(chain, await eng.multiplyPlain(B[i], P[i]));
    assert.strictEqual(await wordsOf(eng, d), await wordsOf(eng, chain));
    // multiplyPlain's - 2 per ballot, then the tree (0 1)(2 3): -1 per level
    assert.strictEqual(first, b[0].noiseBudget - 2);
    assert.strictEqual(d.noiseBudget, first - 2);
    const got = await eng.decrypt(d, sk);
    assert.strictEqual(got.success, true);
    assert.strictEqual(got.plaintext.values[0], (1n * 3n + 0n * 5n + 1n * 7n + 1n * 5n) % T);
    const small = await eng.dotPlain(b, p);
    assert.strictEqual((await eng.decrypt(small, sk)).plaintext.values[0], 10n);
    // pts = X^k: the tally of the ballots moves from slot 0 to slot k
    const k = 5, mono = new Array(k + 1).fill(0n);
    mono[k] = 1n;
    const xk = eng.createPackedPlaintext(mono);
    const moved = await eng.decryptPacked(await eng.dotPlain(b, [xk, xk, xk]), sk, k + 1);
    assert.strictEqual(moved[k], 2n);
    assert.strictEqual(moved[0], 0n);
  });

  await test('multiplyPlain on a degree-1 ciphertext keeps the words of the polymul path', async () => {
    const { eng, pk } = await weightedEngine();
    const n = 1024, ctx = eng.context;
    const ct = await eng.encryptValue(3n, pk);
    for (const pt of [eng.createPlaintext(7n), eng.createPackedPlaintext([1n, 2n, 3n, 2047n])]) {
      const enc = eng._encoded(pt);
      const rep = new fhe.DeviceBuffer(ctx, 2 * n);
      rep.upload(enc, 0);
      rep.upload(enc, n);
      const want = ctx.polymul(eng.deviceBuffer(ct), rep, new fhe.DeviceBuffer(ctx, 2 * n)).download();
      const got = await eng.multiplyPlain(ct, pt);
      assert.strictEqual(got.degree, 1);
      assert.strictEqual(got.noiseBudget, ct.noiseBudget - 2);
      assert.deepStrictEqual(eng.deviceBuffer(got).download(), want);
    }
  });

  await test('argument errors', async () => {
    const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [132120577n], securityLevel: 128, plaintextModulus: 16n },
      { seed: 7n });
    const skA = await eng.generateSecretKey(), skB = await eng.generateSecretKey();
    const pkA = await eng.generatePublicKey(skA), pkB = await eng.generatePublicKey(skB);
    const a = await eng.encryptValue(5n, pkA), a2 = await eng.encryptValue(1n, pkA), b = await eng.encryptValue(6n, pkB);
    const pt = eng.createPlaintext(3n);
    await rejects(eng.tallyScalarWeightedVotes([a, a2], [1n]), 'INVALID_PARAMETERS', /Ballots and weights must have the same size/);
    await rejects(eng.tallyScalarWeightedVotes([], []), 'INVALID_PARAMETERS', /Cannot add empty vector of ciphertexts/);
    await rejects(eng.tallyScalarWeightedVotes([a, b], [1n, 2n]), 'KEY_MISMATCH', /Cannot add ciphertexts encrypted with different keys/);
    await rejects(eng.dotPlain([a, a2], [pt]), 'INVALID_PARAMETERS', /Ballots and weights must have the same size/);
    await rejects(eng.dotPlain([], []), 'INVALID_PARAMETERS', /Cannot tally empty ballot list/);
    await rejects(eng.dotPlain([a, b], [pt, pt]), 'KEY_MISMATCH', /Cannot add ciphertexts encrypted with different keys/);
    await rejects(eng.dotPlain([a], [{ values: [1n] }]), 'INVALID_PARAMETERS', /Plaintext/);
    const d2 = await eng.multiply(a, a2);
    await rejects(eng.dotPlain([a, d2], [pt, pt]), 'INVALID_PARAMETERS', /degree-1/);
    // the addon's own argument checks
    const ctx = eng.context, buf = eng.deviceBuffer(a), buf2 = eng.deviceBuffer(a2);
    const out = new fhe.DeviceBuffer(ctx, 2048), pbuf = new fhe.DeviceBuffer(ctx, 1024).upload(eng._encoded(pt));
    assert.throws(() => ctx.sumScaled([], new BigUint64Array(0), out), /Cannot add empty vector of ciphertexts/);
    assert.throws(() => ctx.sumScaled([buf, buf2], new BigUint64Array(1), out), /Ballots and weights must have the same size/);
    assert.throws(() => ctx.sumScaled([buf], [1n], out), /BigUint64Array/);
    assert.throws(() => ctx.sumScaled([buf], new BigUint64Array(1), new BigUint64Array(2048)), /DeviceBuffers of this context/);
    assert.throws(() => ctx.dotPlain([], [], out), /Cannot tally empty ballot list/);
    assert.throws(() => ctx.dotPlain([buf, buf2], [pbuf], out), /Ballots and weights must have the same size/);
    assert.throws(() => ctx.dotPlain([buf], [pbuf], new fhe.DeviceBuffer(ctx, 3072)), /degree-1/);
    assert.throws(() => ctx.dotPlain([buf], [buf2], out), /n words/);
    const s1 = ctx.mulScalar(buf, 3n, new fhe.DeviceBuffer(ctx, 2048)), s2 = ctx.mulScalar(buf2, 5n, new fhe.DeviceBuffer(ctx, 2048));
    assert.deepStrictEqual(ctx.sumScaled([buf, buf2], BigUint64Array.from([3n, 5n]), out).download(),
      ctx.add(s1, s2, new fhe.DeviceBuffer(ctx, 2048)).download());
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
