'use strict';
// Galois automorphisms, re-keying and the trace of the FHEEngine surface on the
// GPU: polyGalois (fhe_poly_galois_batch) against sigma_g in BigInt arithmetic,
// ctGaloisAsync / ctTraceAsync (fhe_ct_galois_batch, fhe_ct_trace_batch) against
// their chains of older calls, and generateSwitchKey / generateGaloisKeys /
// applyGalois / reKey / isolateSlot on encrypted values.
//   node tests/js/galois_test.js
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

const M64 = (1n << 64n) - 1n;
function splitmix(seed) {
  let x = BigInt(seed);
  return () => {
    x = (x + 0x9E3779B97F4A7C15n) & M64;
    let z = x;
    z = ((z ^ (z >> 30n)) * 0xBF58476D1CE4E5B9n) & M64;
    z = ((z ^ (z >> 27n)) * 0x94D049BB133111EBn) & M64;
    return z ^ (z >> 31n);
  };
}

// out[j g mod 2n] = +-in[j]: the definition, one row
function sigma(row, g, q) {
  const n = row.length, out = new BigUint64Array(n);
  for (let j = 0; j < n; j++) {
    const k = (j * g) % (2 * n);
    if (k < n) out[k] = row[j] % q;
    else out[k - n] = (q - row[j] % q) % q;
  }
  return out;
}

async function main() {
  await test('the addon and the engine export the Galois surface', async () => {
    for (const m of ['polyGalois', 'switchKeyGenerate', 'ctGalois', 'ctGaloisAsync', 'ctTrace', 'ctTraceAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    for (const m of ['generateSwitchKey', 'generateGaloisKeys', 'applyGalois', 'reKey', 'isolateSlot']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('polyGalois, ctGaloisAsync and ctTraceAsync: sigma_g and the chains at (256, 7681)', async () => {
    const n = 256, q = 7681n, batch = 3, bl = 5, lv = 3;
    const ctx = new fhe.NttContext(n, q, 1, 0);
    const rnd = splitmix(29);
    const ct = new BigUint64Array(batch * 2 * n), raw = new BigUint64Array(2 * lv * 2 * n);
    for (let i = 0; i < ct.length; i++) ct[i] = rnd();
    [0n, q - 1n, q, M64].forEach((v, i) => { ct[i] = v; ct[ct.length - 1 - i] = v; });
    for (let i = 0; i < raw.length; i++) raw[i] = rnd() % q;
    const keys = ctx.prepareRelinKey(raw, new BigUint64Array(raw.length));
    const key = keys.subarray(0, lv * 2 * n);
    for (const g of [1, 3, n / 2 + 1, n + 1, 2 * n - 1, (5 ** 7) % (2 * n)]) {
      const s = ctx.polyGalois(ct, g, new BigUint64Array(ct.length));
      for (let r = 0; r < 2 * batch; r++) {
        assert.deepStrictEqual(s.subarray(r * n, (r + 1) * n), sigma(ct.subarray(r * n, (r + 1) * n), g, q), `sigma ${g}`);
      }
      for (const add of [0, 1]) {
        // ct3 = (sigma(c0) [+ c0], [c1 mod q | 0], sigma(c1))
        const ct3 = new BigUint64Array(batch * 3 * n);
        for (let c = 0; c < batch; c++) {
          for (let j = 0; j < n; j++) {
            const s0 = s[(2 * c) * n + j], c0 = ct[(2 * c) * n + j] % q, c1 = ct[(2 * c + 1) * n + j] % q;
            ct3[(3 * c) * n + j] = add ? (s0 + c0) % q : s0;
            ct3[(3 * c + 1) * n + j] = add ? c1 : 0n;
            ct3[(3 * c + 2) * n + j] = s[(2 * c + 1) * n + j];
          }
        }
        const want = ctx.relinearizePrepared(ct3, key, bl, new BigUint64Array(ct.length));
        const got = await ctx.ctGaloisAsync(bl, g, key, ct, add, new BigUint64Array(ct.length));
        assert.deepStrictEqual(got, want, `g ${g} add ${add}`);
      }
    }
    // two trace steps = the scalar (2^2)^-1 and two key switches with add_input
    const inv4 = ((q + 1n) / 2n) ** 2n % q;
    let x = ctx.mulScalar(ct, inv4, new BigUint64Array(ct.length));
    x = ctx.ctGalois(bl, n + 1, keys.subarray(0, lv * 2 * n), x, 1, new BigUint64Array(ct.length));
    x = ctx.ctGalois(bl, n / 2 + 1, keys.subarray(lv * 2 * n), x, 1, new BigUint64Array(ct.length));
    assert.deepStrictEqual(await ctx.ctTraceAsync(bl, 2, keys, ct, new BigUint64Array(ct.length)), x);
    assert.throws(() => ctx.polyGalois(ct, 2, new BigUint64Array(ct.length)), /Galois element must be odd/);
    assert.throws(() => ctx.ctGalois(bl, 2 * n + 1, key, ct, 0, new BigUint64Array(ct.length)), /out of range/);
    assert.throws(() => ctx.ctTrace(bl, 9, keys, ct, new BigUint64Array(ct.length)), /steps/);
  });

  await test('reKey, applyGalois and isolateSlot on encrypted values', async () => {
    // worst case of the full trace: (2^10 - 1) * level 8 * n 2^10 * 255 * 28 < 2^36, against q / (2 t) > 2^52
    const N = 1024, Q = 4611686018326724609n, T = 257n;
    const eng = await fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T },
      { seed: 23n, mode: 'negacyclic' });
    const skA = await eng.generateSecretKey(), skB = await eng.generateSecretKey();
    const pk = await eng.generatePublicKey(skA);
    const values = Array.from({ length: N }, (_, i) => BigInt((i * 7 + 3) % 257));
    const ct = await eng.encryptPacked(values, pk);
    // re-keying: the same values under the second key, no longer under the first
    const rk = await eng.generateSwitchKey(skB, skA);
    assert.strictEqual(rk.__brand, 'SwitchKey');
    assert.strictEqual(rk.galoisElement, 1);
    assert.ok(rk.decompBaseLog * rk.decompLevel >= 62);
    const moved = await eng.reKey(ct, rk);
    assert.strictEqual(moved.keyId, skB.keyId);
    assert.deepStrictEqual(Array.from(await eng.decryptPacked(moved, skB, N)), values);
    await assert.rejects(() => eng.reKey(moved, rk), /does not match/);
    // sigma_3 of the values, negated modulo t where X^n = -1 was crossed
    const gk = await eng.generateSwitchKey(skA, skA, { galoisElement: 3 });
    const turned = await eng.applyGalois(ct, 3, gk);
    const want = Array.from(sigma(BigUint64Array.from(values), 3, T));
    assert.deepStrictEqual(Array.from(await eng.decryptPacked(turned, skA, N)), want);
    await assert.rejects(() => eng.reKey(ct, gk), /Galois element 1/);
    await assert.rejects(() => eng.applyGalois(ct, 5, gk), /Galois element 3/);
    // one slot and nothing else
    const keys = await eng.generateGaloisKeys(skA);
    assert.strictEqual(keys.__brand, 'GaloisKeys');
    assert.strictEqual(keys.steps, 10);
    for (const slot of [0, 5, N - 1]) {
      const one = await eng.isolateSlot(ct, slot, keys);
      const only = new Array(N).fill(0n);
      only[slot] = values[slot];
      assert.deepStrictEqual(Array.from(await eng.decryptPacked(one, skA, N)), only, `slot ${slot}`);
    }
    await assert.rejects(() => eng.isolateSlot(ct, N, keys), /slot index out of range/);
    await assert.rejects(async () => eng.isolateSlot(ct, 0, await eng.generateGaloisKeys(skA, 3)), /full trace/);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
