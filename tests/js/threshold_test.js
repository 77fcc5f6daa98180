'use strict';
// Threshold decryption of the FHEEngine surface on the GPU: generateThresholdKeys
// over the addon's shamirSharesAsync, partialDecrypt / partialDecryptBatch over
// prepareKeySharesAsync + partialDecryptPreparedAsync (fhe_partial_decrypt_batch),
// combinePartialDecryptions / combinePartialDecryptionsBatch over
// combinePartialsAsync (fhe_combine_partials_batch).
//   node tests/js/threshold_test.js
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

const N = 1024, Q = 132120577n, T = 16n;
const engine = () => fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T }, { seed: 11n, mode: 'negacyclic' });  // the mode whose product is the ring's: slots decrypt
const slots = (k) => Array.from({ length: N }, (_, i) => BigInt((i * 7 + k * 3) % 16));

async function main() {
  await test('the addon, the ring wrapper and the engine export the threshold surface', async () => {
    for (const m of ['shamirShares', 'prepareKeyShares', 'partialDecryptPrepared', 'combinePartials']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
      assert.strictEqual(typeof fhe.NttContext.prototype[m + 'Async'], 'function', m);
    }
    for (const m of ['partialDecrypt', 'combinePartials']) assert.strictEqual(typeof fhe.PolynomialEngine.prototype[m], 'function', m);
    for (const m of ['partialDecryptBatch', 'combinePartialDecryptionsBatch']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('partialDecryptBatch: partialDecrypt per ciphertext, and polymul(c1, share)', async () => {
    const eng = await engine();
    const tk = await eng.generateThresholdKeys({ threshold: 2, totalShares: 3 });
    const cts = [];
    for (let k = 0; k < 3; k++) cts.push(await eng.encryptPacked(slots(k), tk.publicKey));
    const share = tk.shares[1];
    const batch = await eng.partialDecryptBatch(cts, share);
    assert.strictEqual(batch.length, 3);
    const ring = new fhe.PolynomialEngine(N, Q);
    const sw = eng.deviceBuffer(share).download();
    for (let k = 0; k < 3; k++) {
      const one = await eng.partialDecrypt(cts[k], share);
      assert.strictEqual(batch[k].shareId, 2);
      assert.deepStrictEqual(batch[k], one);
      const c1 = eng.deviceBuffer(cts[k]).download().slice(N, 2 * N);
      const ctBuf = eng.deviceBuffer(cts[k]), prod = new fhe.DeviceBuffer(eng._ctx, N);
      eng._ctx.polymul(ctBuf.view(N, N), eng.deviceBuffer(share), prod);
      assert.deepStrictEqual(BigUint64Array.from(one.partialResult), prod.download());
      // the ring wrapper: prepared and multiplied in one call
      assert.deepStrictEqual(ring.partialDecrypt(eng.deviceBuffer(cts[k]).download(), sw), ring.multiply(c1, sw));
    }
    assert.deepStrictEqual(await eng.partialDecryptBatch([], share), []);
  });

  await test('combinePartialDecryptionsBatch: two 2-of-3 subsets open the encrypted slots', async () => {
    const eng = await engine();
    const tk = await eng.generateThresholdKeys({ threshold: 2, totalShares: 3 });
    const cts = [];
    for (let k = 0; k < 4; k++) cts.push(await eng.encryptPacked(slots(k), tk.publicKey));
    for (const subset of [[0, 2], [2, 1]]) {
      const partials = [];
      for (const i of subset) partials.push(await eng.partialDecryptBatch(cts, tk.shares[i]));
      const res = await eng.combinePartialDecryptionsBatch(cts, partials, 2);
      assert.strictEqual(res.length, 4);
      for (let k = 0; k < 4; k++) {
        assert.strictEqual(res[k].success, true);
        assert.deepStrictEqual(res[k].plaintext.values, slots(k));
        assert.ok(Number.isFinite(res[k].remainingNoiseBudget) && res[k].remainingNoiseBudget >= 0, String(res[k].remainingNoiseBudget));
        // the single form: same values, the initial budget as before
        const single = await eng.combinePartialDecryptions(cts[k], partials.map((l) => l[k]), 2);
        assert.deepStrictEqual(single.plaintext.values, res[k].plaintext.values);
        assert.strictEqual(single.remainingNoiseBudget, eng._initialBudget);
      }
    }
  });

  await test('the same seed gives the same shares and commitments', async () => {
    const a = await (await engine()).generateThresholdKeys({ threshold: 3, totalShares: 5 });
    const e2 = await engine();
    const b = await e2.generateThresholdKeys({ threshold: 3, totalShares: 5 });
    assert.strictEqual(a.shares.length, 5);
    for (let i = 0; i < 5; i++) {
      assert.strictEqual(a.shares[i].shareId, i + 1);
      assert.deepStrictEqual(a.shares[i].commitment, b.shares[i].commitment);
      assert.strictEqual(a.shares[i].commitment.length, 32);
    }
    assert.notDeepStrictEqual(a.shares[0].commitment, a.shares[1].commitment);
    // the commitment is the SHA-256 of the share's words
    const words = e2.deviceBuffer(b.shares[4]).download();
    const h = require('crypto').createHash('sha256').update(Buffer.from(words.buffer, words.byteOffset, words.byteLength)).digest();
    assert.deepStrictEqual(b.shares[4].commitment, new Uint8Array(h));
  });

  await test('error codes: THRESHOLD_NOT_MET and KEY_MISMATCH', async () => {
    const eng = await engine();
    const tk = await eng.generateThresholdKeys({ threshold: 2, totalShares: 3 });
    const other = await eng.generateThresholdKeys({ threshold: 2, totalShares: 3 });
    const cts = [await eng.encryptPacked(slots(0), tk.publicKey), await eng.encryptPacked(slots(1), tk.publicKey)];
    const p0 = await eng.partialDecryptBatch(cts, tk.shares[0]);
    await rejects(eng.combinePartialDecryptionsBatch(cts, [p0], 2), 'THRESHOLD_NOT_MET');
    await rejects(eng.combinePartialDecryptions(cts[0], [p0[0]], 2), 'THRESHOLD_NOT_MET');
    await rejects(eng.partialDecryptBatch(cts, other.shares[0]), 'KEY_MISMATCH', /Key share does not match/);
    await rejects(eng.partialDecrypt(cts[0], other.shares[0]), 'KEY_MISMATCH', /Key share does not match/);
    const foreign = await eng.encryptPacked(slots(2), other.publicKey);
    await rejects(eng.partialDecryptBatch([cts[0], foreign], tk.shares[0]), 'KEY_MISMATCH');
    await rejects(eng.combinePartialDecryptionsBatch(cts, [p0, p0.slice(0, 1)], 2), 'INVALID_PARAMETERS');
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
