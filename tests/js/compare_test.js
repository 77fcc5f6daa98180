'use strict';
// Encrypted comparisons of the FHEEngine surface on the GPU: compareGreaterThan,
// compareEqual and checkThresholds over slotExtractAsync (fhe_slot_extract_batch),
// keySwitchAsync, bootstrapPreparedAsync and lweSumAsync (fhe_lwe_sum_batch), and
// the words of slotExtractAsync against the formula in BigInt arithmetic.
//   node tests/js/compare_test.js
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
  await test('the addon and the engine export the comparison surface', async () => {
    for (const m of ['slotExtract', 'lweSum']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
      assert.strictEqual(typeof fhe.NttContext.prototype[m + 'Async'], 'function', m);
    }
    for (const m of ['compareGreaterThan', 'compareLessThan', 'compareEqual', 'checkThreshold', 'checkThresholds',
      'checkRange', 'detectDuplicate']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('slotExtractAsync: the words of the formula at (256, 7681)', async () => {
    const n = 256, q = 7681n, batch = 3;
    const ctx = new fhe.NttContext(n, q, 0, 0);
    const rnd = splitmix(7);
    const ct = new BigUint64Array(batch * 2 * n), ref = new BigUint64Array(batch * 2 * n);
    for (let i = 0; i < ct.length; i++) { ct[i] = rnd(); ref[i] = rnd(); }
    for (const w of [ct, ref]) {
      for (let c = 0; c < batch; c++) {
        for (let p = 0; p < 2; p++) {
          const o = (c * 2 + p) * n;
          [0n, q - 1n, q, M64].forEach((v, i) => { w[o + i] = v; w[o + n - 1 - i] = v; });
        }
      }
    }
    const slots = [0, n - 1, n / 2, n / 2, 5];
    const offs = [0n, q, M64, 1234n, q - 1n];
    for (const useRef of [false, true]) {
      for (const negate of [0, 1]) {
        const a = new BigUint64Array(batch * slots.length * n), b = new BigUint64Array(batch * slots.length);
        await ctx.slotExtractAsync(ct, useRef ? ref : null, negate, BigUint64Array.from(slots, BigInt), BigUint64Array.from(offs), a, b);
        for (let c = 0; c < batch; c++) {
          const d = (p, i) => {
            let x = ct[(c * 2 + p) * n + i] % q, y = useRef ? ref[(c * 2 + p) * n + i] % q : 0n;
            if (negate) [x, y] = [y, x];
            return (x - y + q) % q;
          };
          slots.forEach((h, s) => {
            for (let j = 0; j < n; j++) {
              const want = j <= h ? d(1, h - j) : (q - d(1, n + h - j)) % q;
              assert.strictEqual(a[(c * slots.length + s) * n + j], want, `a c=${c} s=${s} j=${j} ref=${useRef} neg=${negate}`);
            }
            assert.strictEqual(b[c * slots.length + s], (d(0, h) + offs[s] % q) % q, `b c=${c} s=${s}`);
          });
        }
      }
    }
    // lweSumAsync: two terms and a body offset
    const la = BigUint64Array.from([1n, q - 1n, q, M64, 5n, 6n, 7n, 8n]), lb = BigUint64Array.from([q - 1n, 3n, 4n, M64]);
    const oa = new BigUint64Array(4), ob = new BigUint64Array(2);
    await ctx.lweSumAsync(la, lb, 2, M64, oa, ob);
    for (let x = 0; x < 4; x++) assert.strictEqual(oa[x], (la[x] % q + la[4 + x] % q) % q);
    for (let c = 0; c < 2; c++) assert.strictEqual(ob[c], (lb[c] % q + lb[2 + c] % q + M64 % q) % q);
  });

  await test('zero-key truth tables: compareGreaterThan, compareEqual, checkThresholds', async () => {
    const N = 1024, Q = 132120577n, T = 16n, DELTA = Q / T;
    const eng = await fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T,
      lweDimension: 8, decompBaseLog: 4, decompLevel: 3 }, { seed: 5n, mode: 'negacyclic' });
    const sk = await eng.generateSecretKey();
    const pk = await eng.generatePublicKey(sk);
    const bk = await eng.generateBootstrapKey(sk);
    // all-zero bootstrapping and key switching keys: the sign bootstrap then acts on the body alone
    for (const part of [undefined, 'kskA', 'kskB']) {
      const buf = eng.deviceBuffer(bk, part);
      assert.ok(buf, String(part));
      buf.upload(new BigUint64Array(buf.words));
    }
    const rnd = splitmix(11);
    // c0 = encode(values), c1 random: under zero keys the phase of an extracted LWE is c0[slot]
    const plain = async (values) => {
      const ct = await eng.encryptPacked(values, pk);
      const w = new BigUint64Array(2 * N);
      values.forEach((v, i) => { w[i] = ((v * DELTA) & M64) % Q; });
      for (let i = N; i < 2 * N; i++) w[i] = rnd() % Q;
      eng.deviceBuffer(ct).upload(w);
      return ct;
    };
    const half = Number(T / 2n), slot = 3;
    const cts = [];
    for (let v = 0; v < half; v++) {
      const vals = new Array(N).fill(0n);
      vals[slot] = BigInt(v);
      vals[0] = BigInt((v + 3) % half);
      cts.push(await plain(vals));
    }
    for (let a = 0; a < half; a++) {
      for (let b = 0; b < half; b++) {
        const gt = await eng.compareGreaterThan(cts[a], cts[b], bk, { slot });
        const eq = await eng.compareEqual(cts[a], cts[b], bk, { slot });
        assert.strictEqual(await eng.decryptValue(gt, sk), a > b ? 1n : 0n, `gt ${a} ${b}`);
        assert.strictEqual(await eng.decryptValue(eq, sk), a === b ? 1n : 0n, `eq ${a} ${b}`);
      }
    }
    // slot 0 by default
    const gt0 = await eng.compareGreaterThan(cts[1], cts[2], bk);
    assert.strictEqual(await eng.decryptValue(gt0, sk), 4 > 5 ? 1n : 0n);
    // per-candidate thresholds: tally[j] >= thresholds[j]
    const tally = [5n, 0n, 7n, 3n, 2n, 6n];
    const thresholds = [5n, 1n, 0n, 4n, 2n, 7n];
    const ct = await plain(tally.concat(new Array(N - tally.length).fill(0n)));
    const alerts = await eng.checkThresholds(ct, thresholds, bk);
    assert.strictEqual(alerts.length, thresholds.length);
    for (let j = 0; j < thresholds.length; j++) {
      assert.strictEqual(alerts[j].__brand, 'Ciphertext');
      assert.strictEqual(await eng.decryptValue(alerts[j], sk), tally[j] >= thresholds[j] ? 1n : 0n, `threshold ${j}`);
    }
    const one = await eng.checkThreshold(ct, 6n, bk, { slot: 2 });
    assert.strictEqual(await eng.decryptValue(one, sk), 1n);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
