'use strict';
// Hoisted rotations of the FHEEngine surface on the GPU: rotateMany against the
// model's permutation (from a ciphertext and from a hoisted one), the context's
// ctHoist / ctHoistedGalois words against ctGalois at g = 1, and linearTransform
// against the slot-wise sum of diagonal products.
//   node tests/js/hoist_test.js
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

// w[r][i] = v[r][(i + steps) mod n/2]
function rotate(v, steps) {
  const n = v.length, half = n / 2;
  return v.map((_, s) => v[Math.floor(s / half) * half + (((s % half) + steps) % half + half) % half]);
}

async function main() {
  // n = 64, the 62-bit prime, t = 257, key-switch base 2^16 x 4 (tests/test_hoist_abi.py bounds the noise)
  const N = 64, Q = 4611686018326724609n, T = 257n;
  const eng = await fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T },
    { seed: 37n, mode: 'negacyclic' });
  const sk = await eng.generateSecretKey();
  const pk = await eng.generatePublicKey(sk);
  const v = Array.from({ length: N }, (_, i) => BigInt((i * 7 + 3) % 257));
  const steps = [1, 2, 3, 5];
  const keys = await eng.generateRotationKeysFor(sk, steps, { decompBaseLog: 16, decompLevel: 4 });
  const cv = (await eng.encrypt(await eng.encodeSimd(v), pk)).ciphertext;
  const open = async (ct) => eng.decodeSimd(await eng.decryptPacked(ct, sk, N));

  await test('rotateMany from a ciphertext and from a hoisted ciphertext', async () => {
    for (const m of ['ctHoist', 'ctHoistAsync', 'ctHoistedGalois', 'ctHoistedGaloisAsync', 'ctHoistedLinear', 'ctHoistedLinearAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    for (const m of ['hoist', 'rotateMany', 'linearTransform', 'generateRotationKeysFor']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
    assert.strictEqual(keys.__brand, 'RotationKeys');
    assert.strictEqual(keys.steps, steps.length);
    const rots = await eng.rotateMany(cv, [5, 1, -61], keys);
    assert.strictEqual(rots.length, 3);
    assert.deepStrictEqual(await open(rots[0]), rotate(v, 5));
    assert.deepStrictEqual(await open(rots[1]), rotate(v, 1));
    assert.deepStrictEqual(await open(rots[2]), rotate(v, 3));  // -61 = 3 mod n/2
    const h = await eng.hoist(cv, keys);
    assert.strictEqual(h.__brand, 'HoistedCiphertext');
    assert.deepStrictEqual(await open((await eng.rotateMany(h, [2], keys))[0]), rotate(v, 2));
    await assert.rejects(async () => eng.rotateMany(cv, [4], keys), /no key/);
    await assert.rejects(async () => eng.rotateRows(cv, 1, keys), /explicit steps/);
    const other = await eng.generateSecretKey();
    await assert.rejects(async () => eng.rotateMany(cv, [1], await eng.generateRotationKeysFor(other, [1])), /do not match/);
  });

  await test('the context: hoisted words at g = 1 are ctGalois words', async () => {
    const ctx = new fhe.NttContext(N, Q, 1, 0);
    const bl = 16, lv = 4;
    const ct = BigUint64Array.from({ length: 2 * N }, (_, i) => (BigInt(i) * 0x9E3779B97F4A7C15n) & 0xFFFFFFFFFFFFFFFFn);
    const raw = BigUint64Array.from({ length: lv * 2 * N }, (_, i) => (BigInt(i + 5) * 0xD1B54A32D192ED03n) % Q);
    const prep = ctx.prepareRelinKey(raw, new BigUint64Array(raw.length));
    const hoisted = ctx.ctHoist(bl, lv, ct, new BigUint64Array((1 + lv) * N));
    const one = BigUint64Array.from([1n]), zero = BigUint64Array.from([0n]);
    const got = ctx.ctHoistedGalois(lv, one, zero, prep, hoisted, new BigUint64Array(2 * N));
    const want = ctx.ctGalois(bl, 1, prep, ct, 0, new BigUint64Array(2 * N));
    assert.deepStrictEqual(Array.from(got), Array.from(want));
    assert.deepStrictEqual(Array.from(await ctx.ctHoistedGaloisAsync(lv, one, zero, prep, hoisted, new BigUint64Array(2 * N))), Array.from(want));
    assert.throws(() => ctx.ctHoistedGalois(lv, BigUint64Array.from([2n]), zero, prep, hoisted, new BigUint64Array(2 * N)), /odd/);
    assert.throws(() => ctx.ctHoistedGalois(lv, one, one, prep, hoisted, new BigUint64Array(2 * N)), /out of range/);
  });

  await test('linearTransform sums diagonal products slot by slot', async () => {
    const d = [0, 1, 3].map((st, k) => [st, Array.from({ length: N }, (_, i) => BigInt((i * (k + 2) + 5 * k + 1) % 257))]);
    const want = v.map((_, i) => d.reduce((a, [st, diag]) => a + diag[i] * rotate(v, st)[i], 0n) % T);
    assert.deepStrictEqual(await open(await eng.linearTransform(cv, d, keys)), want);
    // without the unrotated diagonal, from a hoisted ciphertext and a Map
    const h = await eng.hoist(cv, keys);
    const want2 = v.map((_, i) => d.slice(1).reduce((a, [st, diag]) => a + diag[i] * rotate(v, st)[i], 0n) % T);
    assert.deepStrictEqual(await open(await eng.linearTransform(h, new Map(d.slice(1)), keys)), want2);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
