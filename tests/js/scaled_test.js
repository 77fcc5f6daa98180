'use strict';
// The scale-invariant BFV products of the FHEEngine surface on the GPU:
// ctMultiplyScaled / ctDotScaled / ctSquareScaled (fhe_ct_multiply_scaled_batch,
// fhe_ct_dot_scaled_batch, fhe_ct_square_scaled_batch) against the definition in
// BigInt arithmetic, and multiplyScaled / squareScaled / dotProductScaled /
// tallyWeightedVotes(..., { scaled: true }) on values encrypted with real keys.
//   node tests/js/scaled_test.js
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

// the definition of include/fhe_gpu.h in BigInt arithmetic
const lift = (x, q) => { const r = x % q; return r <= (q - 1n) / 2n ? r : r - q; };
const mod = (x, q) => ((x % q) + q) % q;
function rnd(y, q) { return (y - lift(mod(y, q), q)) / q; }
function nega(a, b) {
  const n = a.length, out = new Array(n).fill(0n);
  for (let i = 0; i < n; i++) for (let j = 0; j < n; j++) {
    if (i + j < n) out[i + j] += a[i] * b[j]; else out[i + j - n] -= a[i] * b[j];
  }
  return out;
}
function tensor(x, y, n, q) {  // one pair [2][n] each -> [X0, X1, X2] over the integers
  const row = (v, r) => Array.from(v.subarray(r * n, (r + 1) * n), (w) => lift(w, q));
  const a0 = row(x, 0), a1 = row(x, 1), b0 = row(y, 0), b1 = row(y, 1);
  const p = nega(a0, b1), r = nega(a1, b0);
  return [nega(a0, b0), p.map((v, i) => v + r[i]), nega(a1, b1)];
}
function scaleRows(X, q, t) {
  const out = [];
  for (const row of X) for (const v of row) out.push(mod(rnd(t * v, q), q));
  return BigUint64Array.from(out);
}

async function main() {
  await test('the addon and the engine export the scaled surface', async () => {
    for (const m of ['ctMultiplyScaled', 'ctMultiplyScaledAsync', 'ctDotScaled', 'ctDotScaledAsync', 'ctSquareScaled', 'ctSquareScaledAsync']) {
      assert.strictEqual(typeof fhe.NttContext.prototype[m], 'function', m);
    }
    for (const m of ['multiplyScaled', 'dotProductScaled', 'squareScaled']) {
      assert.strictEqual(typeof fhe.FHEEngineImpl.prototype[m], 'function', m);
    }
  });

  await test('ctMultiplyScaled, ctDotScaled and ctSquareScaled against the definition at (16, 132120577)', async () => {
    const n = 16, q = 132120577n, t = 4n, batch = 3, w = 2 * n;
    const ctx = new fhe.NttContext(n, q, 1, 0);
    const rng = splitmix(31);
    const x = new BigUint64Array(batch * w), y = new BigUint64Array(batch * w);
    for (let i = 0; i < x.length; i++) { x[i] = rng(); y[i] = rng(); }
    [0n, q - 1n, q, M64, (q - 1n) / 2n, (q + 1n) / 2n].forEach((v, i) => { x[i] = v; y[y.length - 1 - i] = v; });
    const got = ctx.ctMultiplyScaled(t, x, y, new BigUint64Array(batch * 3 * n));
    const sum = [0, 1, 2].map(() => new Array(n).fill(0n));
    for (let c = 0; c < batch; c++) {
      const X = tensor(x.subarray(c * w, (c + 1) * w), y.subarray(c * w, (c + 1) * w), n, q);
      assert.deepStrictEqual(got.subarray(c * 3 * n, (c + 1) * 3 * n), scaleRows(X, q, t), `pair ${c}`);
      X.forEach((row, r) => row.forEach((v, i) => { sum[r][i] += v; }));
    }
    // count 1 in `batch` groups is the multiply; one group of `batch` pairs rescales the sum once
    assert.deepStrictEqual(ctx.ctDotScaled(t, x, y, 1, new BigUint64Array(batch * 3 * n)), got);
    assert.deepStrictEqual(await ctx.ctDotScaledAsync(t, x, y, batch, new BigUint64Array(3 * n)), scaleRows(sum, q, t));
    // squares, with the reference subtracted
    const ref = y.subarray(0, w), d = new BigUint64Array(x.length);
    for (let i = 0; i < x.length; i++) d[i] = mod(x[i] % q - ref[i % w] % q, q);
    assert.deepStrictEqual(await ctx.ctSquareScaledAsync(t, x, ref, new BigUint64Array(batch * 3 * n)),
      ctx.ctMultiplyScaled(t, d, d, new BigUint64Array(batch * 3 * n)));
    assert.deepStrictEqual(ctx.ctSquareScaled(t, x, null, new BigUint64Array(batch * 3 * n)),
      ctx.ctMultiplyScaled(t, x, x, new BigUint64Array(batch * 3 * n)));
    assert.throws(() => ctx.ctMultiplyScaled(q, x, y, new BigUint64Array(batch * 3 * n)), /2 <= t < q/);
    const compat = new fhe.NttContext(n, q, 0, 0);
    assert.throws(() => compat.ctMultiplyScaled(t, x, y, new BigUint64Array(batch * 3 * n)), /FHE_MODE_NEGACYCLIC/);
  });

  await test('multiplyScaled, squareScaled and the scaled weighted tally open with real keys', async () => {
    const N = 1024, Q = 4611686018326724609n, T = 257n;
    const eng = await fhe.createEngine({ polyDegree: N, moduli: [Q], securityLevel: 128, plaintextModulus: T },
      { seed: 29n, mode: 'negacyclic' });
    const sk = await eng.generateSecretKey(), pk = await eng.generatePublicKey(sk);
    // the digits must recompose every word of c2 (the default 3 x 2^4 covers 12 bits of it)
    const ek = await eng.generateEvalKey(sk, { decompBaseLog: 16, decompLevel: 4 });
    assert.ok(ek.decompBaseLog * ek.decompLevel >= 62);
    const m1 = Array.from({ length: N }, (_, i) => BigInt((i * 5 + 2) % 257));
    const m2 = new Array(N).fill(0n);
    m2[0] = 2n; m2[1] = 1n;  // (2 + X) m1
    const want = m1.map((v, k) => mod(2n * v + (k > 0 ? m1[k - 1] : -m1[N - 1]), T));
    const c1 = await eng.encryptPacked(m1, pk), c2 = await eng.encryptPacked(m2, pk);
    const prod = await eng.relinearize(await eng.multiplyScaled(c1, c2), ek);
    assert.deepStrictEqual(Array.from(await eng.decryptPacked(prod, sk, N)), want);
    // the reference's multiply at the same parameters does not open to it
    const plain = await eng.relinearize(await eng.multiply(c1, c2), ek);
    assert.notDeepStrictEqual(Array.from(await eng.decryptPacked(plain, sk, N)), want);
    const sq = await eng.relinearize(await eng.squareScaled(c2), ek);
    const four = new Array(N).fill(0n);
    four[0] = 4n; four[1] = 4n; four[2] = 1n;  // (2 + X)^2
    assert.deepStrictEqual(Array.from(await eng.decryptPacked(sq, sk, N)), four);
    // three ballots under encrypted constant weights
    const ballots = [0, 1, 2].map((b) => Array.from({ length: N }, (_, i) => BigInt((i + b) % 2)));
    const weights = [3n, 5n, 7n];
    const cb = [], cw = [];
    for (let i = 0; i < 3; i++) {
      cb.push(await eng.encryptPacked(ballots[i], pk));
      cw.push(await eng.encryptValue(weights[i], pk));
    }
    const tally = await eng.tallyWeightedVotes(cb, cw, ek, undefined, { scaled: true });
    const sum = ballots[0].map((_, k) => mod(ballots.reduce((s, b, i) => s + b[k] * weights[i], 0n), T));
    assert.deepStrictEqual(Array.from(await eng.decryptPacked(tally, sk, N)), sum);
    const dot = await eng.dotProductScaled(cb, cw);
    assert.strictEqual(dot.degree, 2);
    await assert.rejects(() => eng.dotProductScaled(cb, cw.slice(1)), /same size/);
  });
}

main().then(() => console.log(`${passed} passed`)).catch((e) => {
  console.error(e);
  process.exit(1);
});
