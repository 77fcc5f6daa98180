'use strict';
// LWE-to-RLWE packing of the FHEEngine surface on the GPU: generatePackKey and
// packBits over packKeyGenerateAsync (fhe_pack_key_generate) and lwePackAsync
// (fhe_lwe_pack_batch), and the words of lwePackAsync against the formula of
// include/fhe_gpu.h in BigInt arithmetic.
//   node tests/js/pack_test.js
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

async function main() {
  await test('the addon and the engine export the packing surface', async () => {
    for (const m of ['lwePack', 'lwePackAsync', 'packKeyGenerate', 'packKeyGenerateAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    for (const m of ['generatePackKey', 'packBits']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('lwePackAsync: the words of the formula at (256, 7681)', async () => {
    const n = 256, q = 7681n, batch = 2, bl = 4, lv = 4, dim = 3, entries = dim * lv;
    const ctx = new fhe.NttContext(n, q, 0, 0);
    const rnd = splitmix(13);
    const slots = [0, n - 1, n / 2, n / 2, 5], S = slots.length;
    const key = new BigUint64Array(entries * 2 * n), la = new BigUint64Array(batch * S * dim);
    const lb = new BigUint64Array(batch * S), prev = new BigUint64Array(batch * 2 * n);
    for (const w of [key, la, lb, prev]) {
      for (let i = 0; i < w.length; i++) w[i] = rnd();
      [0n, q - 1n, q, M64].forEach((v, i) => { w[i] = v; w[w.length - 1 - i] = v; });
    }
    for (let i = 0; i < dim; i++) { la[1 * dim + i] = 0n; la[2 * dim + i] = M64; }  // all digits zero / all ones
    const mask = (1n << BigInt(bl)) - 1n;
    const W = (c, s, p, j) => {
      let sum = 0n;
      for (let e = 0; e < entries; e++) {
        const i = Math.floor(e / lv), l = e % lv;
        const d = (la[(c * S + s) * dim + i] >> BigInt((lv - 1 - l) * bl)) & mask;
        sum += ((d * key[(e * 2 + p) * n + j]) & M64) % q;
      }
      return ((-sum + (p === 0 && j === 0 ? lb[c * S + s] % q : 0n)) % q + q) % q;
    };
    const want = (acc) => {
      const out = new BigUint64Array(batch * 2 * n);
      for (let c = 0; c < batch; c++) {
        for (let p = 0; p < 2; p++) {
          for (let j = 0; j < n; j++) {
            let v = acc ? prev[(c * 2 + p) * n + j] % q : 0n;
            slots.forEach((h, s) => { v += j >= h ? W(c, s, p, j - h) : (q - W(c, s, p, n + j - h)) % q; });
            out[(c * 2 + p) * n + j] = v % q;
          }
        }
      }
      return out;
    };
    const slotWords = BigUint64Array.from(slots, BigInt);
    const out = new BigUint64Array(batch * 2 * n);
    await ctx.lwePackAsync(bl, lv, key, la, lb, slotWords, 0, out);
    assert.deepStrictEqual(out, want(false));
    const acc = prev.slice();
    ctx.lwePack(bl, lv, key, la, lb, slotWords, 1, acc);
    assert.deepStrictEqual(acc, want(true));
    assert.throws(() => ctx.lwePack(bl, lv, key, la, lb, BigUint64Array.from([0n, 1n, 2n, 3n, BigInt(n)]), 0, out), /slot index out of range/);
  });

  await test('comparison bits packed into one ciphertext decrypt at their slots', async () => {
    const N = 1024, Q = 132120577n, T = 16n, DELTA = Q / T;
    const eng = await fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T,
      lweDimension: 8, decompBaseLog: 4, decompLevel: 3 }, { seed: 5n, mode: 'negacyclic' });
    const sk = await eng.generateSecretKey();
    const pk = await eng.generatePublicKey(sk);
    const bk = await eng.generateBootstrapKey(sk);
    const packKey = await eng.generatePackKey(sk, bk);
    assert.strictEqual(packKey.__brand, 'PackKey');
    assert.strictEqual(packKey.lweDimension, 8);
    assert.ok(packKey.decompBaseLog * packKey.decompLevel >= 27);
    // all-zero bootstrapping and key switching keys: the sign bootstrap then acts on the body alone
    for (const part of [undefined, 'kskA', 'kskB']) {
      const buf = eng.deviceBuffer(bk, part);
      buf.upload(new BigUint64Array(buf.words));
    }
    const rnd = splitmix(17);
    const plain = async (values) => {
      const ct = await eng.encryptPacked(values, pk);
      const w = new BigUint64Array(2 * N);
      values.forEach((v, i) => { w[i] = ((v * DELTA) & M64) % Q; });
      for (let i = N; i < 2 * N; i++) w[i] = rnd() % Q;
      eng.deviceBuffer(ct).upload(w);
      return ct;
    };
    const tally = [5n, 0n, 7n, 3n, 2n, 6n], thresholds = [5n, 1n, 0n, 4n, 2n, 7n];
    const ct = await plain(tally.concat(new Array(N - tally.length).fill(0n)));
    const alerts = await eng.checkThresholds(ct, thresholds, bk);
    const slots = [9, 0, 1023, 512, 4, 77];
    const packed = await eng.packBits(alerts, slots, packKey);
    assert.strictEqual(packed.__brand, 'Ciphertext');
    const got = await eng.decryptPacked(packed, sk, N);
    const want = new Array(N).fill(0n);
    slots.forEach((h, j) => { want[h] = tally[j] >= thresholds[j] ? 1n : 0n; });
    assert.deepStrictEqual(Array.from(got), want);
    // the packed bits are an ordinary BFV ciphertext: doubling it doubles every bit
    const twice = await eng.add(packed, packed);
    assert.deepStrictEqual(Array.from(await eng.decryptPacked(twice, sk, N)), want.map((v) => 2n * v));
    // repeated slots add their bits: the number of candidates at or above their threshold
    const count = await eng.packBits(alerts, alerts.map(() => 2), packKey);
    assert.strictEqual((await eng.decryptPacked(count, sk, 3))[2], BigInt(want.reduce((a, v) => a + Number(v), 0)));
    await assert.rejects(() => eng.packBits(alerts, [0, 1], packKey), /one slot each/);
    await assert.rejects(() => eng.packBits([ct], [0], packKey), /LWE/);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
