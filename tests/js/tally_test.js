'use strict';
// Ballot aggregation of the FHEEngine surface on the GPU: batchAdd,
// tallyVotes, tallyMultiCandidate, updateTally and tallyWeightedVotes
// (EncryptionEngine::batch_add / batch_add_tree / tally_*,
// encryption.cpp:1061-1168, 1327-1460), each sum one sumAsync launch.
//   node tests/js/tally_test.js
const assert = require('assert');
const path = require('path');

const ROOT = path.join(__dirname, '..', '..');
const fhe = require(path.join(ROOT, 'node-fhe-accelerate_amd', 'lib'));
const M64 = (1n << 64n) - 1n;

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
// splitmix64(seed ^ i) % q (oracle_splitmix_fill)
const splitmix = (seed, q, count) => {
  const out = new Array(count);
  for (let i = 0; i < count; i++) {
    let x = (BigInt(seed) ^ BigInt(i)) & M64;
    x = (x + 0x9E3779B97F4A7C15n) & M64;
    x = ((x ^ (x >> 30n)) * 0xBF58476D1CE4E5B9n) & M64;
    x = ((x ^ (x >> 27n)) * 0x94D049BB133111EBn) & M64;
    x ^= x >> 31n;
    out[i] = x % BigInt(q);
  }
  return out;
};
const wordsOf = async (eng, ct) => {
  const s = await eng.serializeCiphertext(ct);
  const b = Buffer.from(s.data);
  return b.slice(52 + b.readUInt32LE(48)).toString('hex');
};

async function main() {
  await test('the addon and the engine export the tally surface', async () => {
    for (const m of ['sum', 'sumAsync']) assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    for (const m of ['tallyVotes', 'tallyMultiCandidate', 'updateTally', 'tallyWeightedVotes']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('batchAdd and tallyVotes over 5 ciphertexts, one repeated: slots, progress, noise budgets', async () => {
    const eng = await fhe.createEngine('bfv-128-simd', { seed: 21n, mode: 'negacyclic' });
    const t = 65537n, n = eng.getSlotCount();
    const sk = await eng.generateSecretKey(), pk = await eng.generatePublicKey(sk);
    const v = [201, 202, 203, 204].map((s) => splitmix(s, t, n));
    const c = [];
    for (const x of v) c.push(await eng.encryptPacked(x, pk));
    const list = [c[0], c[1], c[2], c[1], c[3]];
    const want = (i) => (v[0][i] + 2n * v[1][i] + v[2][i] + v[3][i]) % t;
    const check = async (ct, what) => {
      const got = await eng.decryptPacked(ct, sk, n);
      for (let i = 0; i < n; i += 97) assert.strictEqual(got[i], want(i), `${what} slot ${i}`);
    };
    const b0 = c[0].noiseBudget;
    const seenB = [], seenT = [];
    const sb = await eng.batchAdd(list, (p) => seenB.push([p.stage, p.current, p.total]));
    await check(sb, 'batchAdd');
    assert.deepStrictEqual(seenB, [2, 3, 4, 5].map((k) => ['batch_add', k, 5]));
    assert.strictEqual(sb.noiseBudget, b0 - 4);           // min - 1 per input, as the chain of add()
    assert.strictEqual(sb.degree, 1);
    assert.strictEqual(sb.isNtt, false);
    assert.strictEqual(sb.keyId, sk.keyId);
    const st = await eng.tallyVotes(list, (p) => seenT.push([p.current, p.total]));
    await check(st, 'tallyVotes');
    assert.deepStrictEqual(seenT, [1, 2, 3, 4].map((k) => [k, 4]));
    // batch_add_tree: ((0 1)(2 3)) 4 -> -1 per level, the odd element carried up: min(b - 2, b) - 1
    assert.strictEqual(st.noiseBudget, b0 - 3);
    assert.strictEqual(await wordsOf(eng, st), await wordsOf(eng, sb));
    // the chain of add() gives the same words
    let chain = list[0];
    for (let i = 1; i < list.length; i++) chain = await eng.add(chain, list[i]);
    assert.strictEqual(await wordsOf(eng, chain), await wordsOf(eng, sb));
    assert.strictEqual(chain.noiseBudget, sb.noiseBudget);
    // one ciphertext: batchAdd hands it back, tallyVotes returns a copy
    assert.strictEqual(await eng.batchAdd([c[2]]), c[2]);
    const one = await eng.tallyVotes([c[2]]);
    assert.notStrictEqual(one, c[2]);
    assert.strictEqual(one.noiseBudget, c[2].noiseBudget);
    assert.strictEqual(await wordsOf(eng, one), await wordsOf(eng, c[2]));
    // tallyMultiCandidate: the slots are the candidates; updateTally is add
    await check(await eng.tallyMultiCandidate(list, n), 'tallyMultiCandidate');
    await rejects(eng.tallyMultiCandidate(list, n + 1), 'INVALID_PARAMETERS', /Number of candidates exceeds polynomial degree/);
    const up = await eng.updateTally(await eng.tallyVotes(list.slice(0, 4)), list[4]);
    await check(up, 'updateTally');
    await rejects(eng.tallyVotes([]), 'INVALID_PARAMETERS', /Cannot add empty vector of ciphertexts/);
    await rejects(eng.batchAdd([]), 'INVALID_PARAMETERS', /Empty/);
    // the packed flag is the inputs'
    assert.strictEqual((await eng.decrypt(sb, sk)).plaintext.isPacked, true);
    const s1 = await eng.batchAdd([await eng.encryptValue(3n, pk), await eng.encryptValue(4n, pk)]);
    const d1 = await eng.decrypt(s1, sk);
    assert.strictEqual(d1.plaintext.isPacked, false);
    assert.strictEqual(d1.plaintext.values[0], 7n);
  });

  await test('mismatched keys, mixed representations and degrees are rejected', async () => {
    const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [132120577n], securityLevel: 128, plaintextModulus: 16n },
      { seed: 7n });
    const skA = await eng.generateSecretKey(), skB = await eng.generateSecretKey();
    const pkA = await eng.generatePublicKey(skA), pkB = await eng.generatePublicKey(skB);
    const a = await eng.encryptValue(5n, pkA), a2 = await eng.encryptValue(1n, pkA), b = await eng.encryptValue(6n, pkB);
    for (const f of ['batchAdd', 'tallyVotes']) {
      await rejects(eng[f]([a, a2, b]), 'KEY_MISMATCH', /different keys/);
      await rejects(eng[f]([b, a]), 'KEY_MISMATCH');
      await rejects(eng[f]([a, { __brand: 'Ciphertext' }]), 'INVALID_PARAMETERS', /handle/);
    }
    // an NTT-form ciphertext arrives through deserialisation
    const s = await eng.serializeCiphertext(a2, { format: 'json' });
    const j = JSON.parse(Buffer.from(s.data).toString());
    j.meta = JSON.stringify(Object.assign(JSON.parse(j.meta), { isNtt: true }));
    const ntt = await eng.deserializeCiphertext({ data: new Uint8Array(Buffer.from(JSON.stringify(j))), format: 'json' });
    assert.strictEqual(ntt.isNtt, true);
    for (const f of ['batchAdd', 'tallyVotes']) {
      await rejects(eng[f]([a, ntt]), 'INVALID_PARAMETERS', /different representations/);
      await rejects(eng[f]([a, a2, ntt]), 'INVALID_PARAMETERS', /different representations/);
    }
    const d2 = await eng.multiply(a, a2);
    await rejects(eng.batchAdd([a, d2]), 'INVALID_PARAMETERS', /degrees differ/);
    await rejects(eng.tallyWeightedVotes([a, a2], [a], null), 'INVALID_PARAMETERS', /Ballots and weights must have the same size/);
    await rejects(eng.tallyWeightedVotes([], [], null), 'INVALID_PARAMETERS', /Cannot tally empty ballot list/);
    // the addon's own argument checks
    const ctx = eng.context, buf = eng.deviceBuffer(a), out = new fhe.DeviceBuffer(ctx, 2048);
    assert.throws(() => ctx.sum([], out), /Cannot add empty vector of ciphertexts/);
    assert.throws(() => ctx.sum([buf, new fhe.DeviceBuffer(ctx, 1024)], out), /DeviceBuffer of out's size/);
    assert.throws(() => ctx.sum([buf, out], out), /none of them out/);
    assert.throws(() => ctx.sum([buf], new BigUint64Array(2048)), /DeviceBuffers of this context/);
    assert.deepStrictEqual(ctx.sum([buf, buf], out).download(), ctx.add(buf, buf, new fhe.DeviceBuffer(ctx, 2048)).download());
  });

  await test('tallyWeightedVotes with 3 ballots decrypts to sum w_i b_i mod t', async () => {
    // The reference's multiply is the plain tensor product (no t / q rescale),
    // so its decryption is the plaintext product only for parameters where
    // delta^2 m decodes to m: no encryption noise (custom parameter sets carry
    // lweNoiseStd = 3.2e-11, every sampled error rounds to 0), delta = 1 mod t
    // and q = 1 mod t, i.e. q = j t^2 + t + 1, here with t = 2N = 2048, and
    // relinearisation digits that cover all of c2 (4 x 16 bits).
    const t = 2048n, q = 2305843009276610561n;  // 549755813903 t^2 + t + 1, prime, 1 mod 2N
    assert.strictEqual((q / t) % t, 1n);
    assert.strictEqual(q % t, 1n);
    const eng = await fhe.createEngine({ polyDegree: 1024, moduli: [q], securityLevel: 128, plaintextModulus: t,
      decompBaseLog: 16, decompLevel: 4 }, { seed: 9n, mode: 'negacyclic' });
    const sk = await eng.generateSecretKey(), pk = await eng.generatePublicKey(sk);
    const ek = await eng.generateEvalKey(sk);
    assert.strictEqual(ek.decompLevel, 4);
    const bs = [1n, 0n, 1n], ws = [3n, 5n, 7n];
    const ballots = [], weights = [];
    for (const x of bs) ballots.push(await eng.encryptValue(x, pk));
    for (const x of ws) weights.push(await eng.encryptValue(x, pk));
    const seen = [];
    const tally = await eng.tallyWeightedVotes(ballots, weights, ek, (p) => seen.push([p.current, p.total]));
    assert.deepStrictEqual(seen, [[4, 5], [5, 5]]);  // total + completed of total + (count - 1)
    assert.strictEqual(tally.degree, 1);
    const d = await eng.decrypt(tally, sk);
    assert.strictEqual(d.success, true);
    assert.strictEqual(d.plaintext.values[0], bs.reduce((acc, x, i) => acc + x * ws[i], 0n) % t);
    // op for op (encryption.cpp:1069-1110): multiply + relinearize per ballot, then the tree sum
    const parts = [];
    for (let i = 0; i < 3; i++) parts.push(await eng.relinearize(await eng.multiply(ballots[i], weights[i]), ek));
    const ref = await eng.add(await eng.add(parts[0], parts[1]), parts[2]);
    assert.strictEqual(await wordsOf(eng, tally), await wordsOf(eng, ref));
    assert.strictEqual(tally.noiseBudget, Math.min(Math.min(parts[0].noiseBudget, parts[1].noiseBudget) - 1, parts[2].noiseBudget) - 1);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
