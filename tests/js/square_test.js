'use strict';
// Squaring and the anomaly score of the FHEEngine surface on the GPU: square /
// squareRelin over the addon's ctSquareAsync / ctSquareRelinPreparedAsync
// (fhe_ct_square_batch, fhe_ct_square_relin_batch) keep the words and metadata
// of multiply(ct, ct), and computeAnomalyScore those of
// relinearize(multiply(subtract(a, b), subtract(a, b))).
//   node tests/js/square_test.js
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
const meta = (c) => ({ keyId: c.keyId, noiseBudget: c.noiseBudget, degree: c.degree, isNtt: c.isNtt });

async function engines() {
  const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [132120577n], securityLevel: 128, plaintextModulus: 16n,
    decompBaseLog: 4, decompLevel: 7 }, { seed: 7n });
  const sk = await eng.generateSecretKey(), pk = await eng.generatePublicKey(sk);
  const ek = await eng.generateEvalKey(sk);
  return { eng, sk, pk, ek };
}

async function main() {
  await test('the addon, the ring wrapper and the engine export the squaring surface', async () => {
    for (const m of ['ctSquare', 'ctSquareAsync', 'ctSquareRelinPrepared', 'ctSquareRelinPreparedAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    assert.strictEqual(typeof fhe.PolynomialEngine.prototype.ctSquare, 'function');
    for (const m of ['square', 'squareRelin', 'computeAnomalyScore']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('square / squareRelin: words and metadata of multiply(ct, ct)', async () => {
    const { eng, pk, ek } = await engines();
    const ct = await eng.encryptPacked([3n, 1n, 4n, 1n, 5n], pk);
    const sq = await eng.square(ct), mul = await eng.multiply(ct, ct);
    assert.deepStrictEqual(eng.deviceBuffer(sq).download(), eng.deviceBuffer(mul).download());
    assert.deepStrictEqual(meta(sq), meta(mul));
    assert.strictEqual(sq.degree, 2);
    const sr = await eng.squareRelin(ct, ek), mr = await eng.relinearize(mul, ek);
    assert.deepStrictEqual(eng.deviceBuffer(sr).download(), eng.deviceBuffer(mr).download());
    assert.deepStrictEqual(meta(sr), meta(mr));
    await rejects(eng.square(mul), 'INVALID_PARAMETERS', /degree-1/);
  });

  await test('computeAnomalyScore: words and metadata of relinearize(multiply(d, d)), d = subtract(a, b)', async () => {
    const { eng, sk, pk, ek } = await engines();
    const a = await eng.encryptPacked([3n, 0n, 1n], pk), b = await eng.encryptPacked([1n, 1n, 1n], pk);
    const score = await eng.computeAnomalyScore(a, b, ek);
    const d = await eng.subtract(a, b);
    const chain = await eng.relinearize(await eng.multiply(d, d), ek);
    assert.deepStrictEqual(eng.deviceBuffer(score).download(), eng.deviceBuffer(chain).download());
    assert.deepStrictEqual(meta(score), meta(chain));
    assert.strictEqual(score.degree, 1);
    assert.strictEqual(score.keyId, sk.keyId);
    // a ballot equal to the expectation: the score is the square of the zero difference
    const zero = await eng.computeAnomalyScore(a, a, ek);
    const dz = await eng.subtract(a, a);
    assert.deepStrictEqual(eng.deviceBuffer(zero).download(),
      eng.deviceBuffer(await eng.relinearize(await eng.multiply(dz, dz), ek)).download());
    // key checks of subtract and relinearize
    const sk2 = await eng.generateSecretKey(), pk2 = await eng.generatePublicKey(sk2), ek2 = await eng.generateEvalKey(sk2);
    const other = await eng.encryptValue(2n, pk2);
    await rejects(eng.computeAnomalyScore(a, other, ek), 'KEY_MISMATCH', /Cannot subtract ciphertexts encrypted with different keys/);
    await rejects(eng.computeAnomalyScore(a, b, ek2), 'KEY_MISMATCH', /Evaluation key does not match ciphertext key/);
    await rejects(eng.computeAnomalyScore(a, await eng.multiply(a, b), ek), 'INVALID_PARAMETERS', /degrees differ/);
  });

  await test('the addon: shared and per-ciphertext ref on host arrays, argument errors', async () => {
    const n = 1024, q = 132120577n;
    const ring = new fhe.PolynomialEngine(n, q);
    const ct = new BigUint64Array(3 * 2 * n), ref = new BigUint64Array(3 * 2 * n);
    let s = 12345n;
    for (let i = 0; i < ct.length; i++) {
      s = (s * 6364136223846793005n + 1442695040888963407n) & 0xffffffffffffffffn;
      ct[i] = s;
      ref[i] = (s >> 7n) * 31n & 0xffffffffffffffffn;
    }
    const one = ref.slice(0, 2 * n);
    const rep = new BigUint64Array(ct.length);
    for (let i = 0; i < 3; i++) rep.set(one, i * 2 * n);
    const d1 = ring.subtract(ct, rep), dn = ring.subtract(ct, ref);
    assert.deepStrictEqual(ring.ctSquare(ct), ring.ctMultiply(ct, ct));
    assert.deepStrictEqual(ring.ctSquare(ct, one), ring.ctMultiply(d1, d1));
    assert.deepStrictEqual(ring.ctSquare(ct, ref), ring.ctMultiply(dn, dn));
    assert.deepStrictEqual(ring.ctSquare(ct, ref, { isNtt: true }), ring.ctMultiply(dn, dn, { isNtt: true }));
    assert.deepStrictEqual(await ring.ctx.ctSquareAsync(ct, one, new BigUint64Array(9 * n), 0), ring.ctMultiply(d1, d1));
    assert.throws(() => ring.ctx.ctSquare(ct, ref.slice(0, 4 * n), new BigUint64Array(9 * n)), /ref must be/);
    assert.throws(() => ring.ctx.ctSquare(ct, null, new BigUint64Array(6 * n)), /out \[batch\]\[3\]\[n\]/);
    assert.throws(() => ring.ctx.ctSquare(ct, 5, new BigUint64Array(9 * n)), /ctSquare\(ct, ref \| null, out, isNtt\?\)/);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
