'use strict';
// SIMD batching of the FHEEngine surface on the GPU: encodeSimd / decodeSimd
// round trip (and simdEncode / simdDecode of the context), one row rotation
// against the model's permutation, and the encrypted inner product.
//   node tests/js/simd_test.js
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

// w[r][i] = v[r xor swap][(i + steps) mod n/2]
function rotate(v, steps, swap) {
  const n = v.length, half = n / 2;
  return v.map((_, s) => v[((Math.floor(s / half) ^ (swap ? 1 : 0)) * half) + (((s % half) + steps) % half + half) % half]);
}

async function main() {
  // n = 64, the 62-bit prime, t = 257 = 1 mod 128, key-switch base 2^16 x 4 (tests/test_simd_abi.py
  // shows the margins of this parameter set in exact integers)
  const N = 64, Q = 4611686018326724609n, T = 257n;
  const eng = await fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T },
    { seed: 31n, mode: 'negacyclic' });
  const sk = await eng.generateSecretKey();
  const pk = await eng.generatePublicKey(sk);
  const v = Array.from({ length: N }, (_, i) => BigInt((i * 7 + 3) % 257));
  const w = Array.from({ length: N }, (_, i) => BigInt((i * i + 11) % 257));

  await test('encodeSimd / decodeSimd round trip, on the engine and on the context', async () => {
    for (const m of ['simdEncode', 'simdEncodeAsync', 'simdDecode', 'simdDecodeAsync', 'ctGaloisChain', 'ctGaloisChainAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    for (const m of ['generateRotationKeys', 'encodeSimd', 'decodeSimd', 'rotateRows', 'rotateColumns', 'sumSlots', 'innerProductScaled']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
    const pt = await eng.encodeSimd(v);
    assert.strictEqual(pt.values.length, N);
    assert.ok(pt.values.every((c) => c < T));
    assert.deepStrictEqual(await eng.decodeSimd(pt), v);
    // raw words are read mod t, a short vector is zero-padded
    assert.deepStrictEqual((await eng.encodeSimd(v.map((x) => x + 3n * T))).values, pt.values);
    assert.deepStrictEqual(await eng.decodeSimd(await eng.encodeSimd([5n, 6n])), [5n, 6n].concat(new Array(N - 2).fill(0n)));
    // the centred lift mod q
    const lifted = await eng.encodeSimd(v, { lift: true });
    pt.values.forEach((c, i) => assert.strictEqual(lifted.values[i], c <= (T - 1n) / 2n ? c : c + (Q - T)));
    // the context: host arrays, and an encryption decrypts to the slots
    const ctx = new fhe.NttContext(N, Q, 1, 0);
    const words = ctx.simdEncode(T, BigUint64Array.from(v), 0, new BigUint64Array(N));
    assert.deepStrictEqual(Array.from(words), pt.values);
    assert.deepStrictEqual(Array.from(await ctx.simdDecodeAsync(T, words, new BigUint64Array(N))), v);
    assert.throws(() => ctx.simdEncode(T, words, 0, words), /overlap/);
    assert.throws(() => ctx.simdEncode(259n, words, 0, new BigUint64Array(N)), /NTT-friendly/);
    const ct = (await eng.encrypt(pt, pk)).ciphertext;
    assert.deepStrictEqual(await eng.decodeSimd(await eng.decryptPacked(ct, sk, N)), v);
  });

  const keys = await eng.generateRotationKeys(sk, { decompBaseLog: 16, decompLevel: 4 });
  const cv = (await eng.encrypt(await eng.encodeSimd(v), pk)).ciphertext;
  const cw = (await eng.encrypt(await eng.encodeSimd(w), pk)).ciphertext;
  const open = async (ct) => eng.decodeSimd(await eng.decryptPacked(ct, sk, N));

  await test('rotateRows and rotateColumns permute the slots', async () => {
    assert.strictEqual(keys.__brand, 'RotationKeys');
    assert.strictEqual(keys.steps, 6);
    assert.deepStrictEqual(await open(await eng.rotateRows(cv, 5, keys)), rotate(v, 5, false));
    assert.deepStrictEqual(await open(await eng.rotateRows(cv, -1, keys)), rotate(v, -1, false));
    assert.deepStrictEqual(await open(await eng.rotateRows(cv, N / 2, keys)), v);
    assert.deepStrictEqual(await open(await eng.rotateColumns(cv, keys)), rotate(v, 0, true));
    const other = await eng.generateSecretKey();
    await assert.rejects(async () => eng.rotateRows(cv, 1, await eng.generateRotationKeys(other)), /do not match/);
  });

  await test('sumSlots and innerProductScaled', async () => {
    const total = v.reduce((a, b) => a + b, 0n) % T;
    assert.deepStrictEqual(await open(await eng.sumSlots(cv, keys)), new Array(N).fill(total));
    const rows = await open(await eng.sumSlots(cv, keys, { rowsOnly: true }));
    const top = v.slice(0, N / 2).reduce((a, b) => a + b, 0n) % T, bottom = v.slice(N / 2).reduce((a, b) => a + b, 0n) % T;
    assert.deepStrictEqual(rows, new Array(N / 2).fill(top).concat(new Array(N / 2).fill(bottom)));
    const ek = await eng.generateEvalKey(sk, { decompBaseLog: 16, decompLevel: 4 });  // must recompose every word of c2
    const ip = v.reduce((a, x, i) => a + x * w[i], 0n) % T;
    assert.deepStrictEqual(await open(await eng.innerProductScaled(cv, cw, ek, keys)), new Array(N).fill(ip));
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
