'use strict';
/**
 * The TypeScript FHEEngine surface (src/api/fhe-engine.ts:33-78,
 * src/api/types.ts:18-166) on the MI355X backend.
 *
 * Every key and ciphertext is a branded, frozen handle object of the
 * reference's shape -- Ciphertext {__brand, handle, keyId, noiseBudget, isNtt,
 * degree}, SecretKey / PublicKey {__brand, handle, keyId}, EvaluationKey
 * {..., decompBaseLog, decompLevel}, BootstrapKey {..., lweDimension} --
 * whose `handle` is the HBM address of its native DeviceBuffer.  The words
 * stay on the GPU between operations: encrypt draws u / e1 / e2 on the
 * device (seeded ChaCha20, fhe_encrypt_sampled_batch), every homomorphic
 * operation is a device-to-device kernel call, and only decrypt /
 * serialisation bring words back.  Device memory is released when the
 * handle object is collected (N-API finalizer, stream-ordered free).
 *
 * Semantics follow the reference C++ engines the TS surface fronts:
 * EncryptionEngine (encryption.cpp: encode/decode, encrypt_internal,
 * decrypt + compute_noise_budget, add/subtract/negate/add_plain/add_scalar,
 * multiply/multiply_plain/multiply_scalar/relinearize and their noise-budget
 * bookkeeping), KeyManager (key_manager.cpp: generate_secret_key /
 * public / eval / threshold keys, partial decryption, Lagrange combination)
 * and BootstrapEngine (bootstrap_engine.cpp: generate_bootstrap_key,
 * bootstrap_with_test_poly, create_lookup_table, the identity test
 * polynomial).  Parameter sets are parameters/index.ts's presets.
 *
 * Randomness: SecureRandom's draws come from a ChaCha20 stream keyed by a
 * 256-bit seed (crypto.randomBytes unless createEngine's options.seed fixes
 * it: then every key and ciphertext is reproducible, which the parity tests
 * use), each key / encryption taking fresh stream ids.
 */
const crypto = require('crypto');
const zlib = require('zlib');

const M64 = (1n << 64n) - 1n;

// ---------------------------------------------------------------- errors (types.ts:140-166)
const FHEErrorCode = Object.freeze({
  NOISE_BUDGET_EXHAUSTED: 'NOISE_BUDGET_EXHAUSTED',
  INVALID_PARAMETERS: 'INVALID_PARAMETERS',
  KEY_MISMATCH: 'KEY_MISMATCH',
  HARDWARE_UNAVAILABLE: 'HARDWARE_UNAVAILABLE',
  SERIALIZATION_ERROR: 'SERIALIZATION_ERROR',
  PROOF_VERIFICATION_FAILED: 'PROOF_VERIFICATION_FAILED',
  THRESHOLD_NOT_MET: 'THRESHOLD_NOT_MET',
  INVALID_BALLOT: 'INVALID_BALLOT',
  DUPLICATE_VOTE: 'DUPLICATE_VOTE',
  NATIVE_ERROR: 'NATIVE_ERROR',
});

class FHEError extends Error {
  constructor(message, code, details) {
    super(message);
    this.name = 'FHEError';
    this.code = code;
    this.details = details;
    Object.setPrototypeOf(this, FHEError.prototype);
  }
}

/** Native errors carry a FHEErrorCode name in `code` (fhe_napi.c code_name). */
function toFHEError(e) {
  if (e instanceof FHEError) return e;
  const code = e && FHEErrorCode[e.code] ? e.code : FHEErrorCode.NATIVE_ERROR;
  return new FHEError(e && e.message ? e.message : String(e), code,
    e && e.status !== undefined ? { status: e.status } : undefined);
}
async function guard(fn) {
  try {
    return await fn();
  } catch (e) {
    throw toFHEError(e);
  }
}

// ---------------------------------------------------------------- parameter sets (parameters/index.ts)
const NTT_PRIMES = Object.freeze({
  Q_60_1: 1152921504606584833n, Q_60_2: 1152921504598720513n, Q_60_3: 1152921504597016577n,
  Q_50_1: 1125899906826241n, Q_50_2: 1125899906793473n,
  Q_40_1: 1099511627777n, Q_40_2: 1099511562241n,
  Q_30_1: 1073479681n, Q_30_2: 1073217537n,
});

/** calculateDerivedParameters (parameters/index.ts:91-124) */
function calculateDerivedParameters(p) {
  let logQ = 0;
  for (const q of p.moduli || []) logQ += Math.log2(Number(q));
  const logT = Math.log2(Number(p.plaintextModulus || 1n));
  let noiseBudget;
  if (p.scheme === 'TFHE') {
    noiseBudget = logQ - Math.log2((p.lweNoiseStd || 1) * Math.sqrt(p.lweDimension || 1)) - 10;
  } else {
    noiseBudget = logQ - logT - 20;
  }
  noiseBudget = Math.max(0, noiseBudget);
  let maxMultDepth = Math.floor(noiseBudget / 10);
  if (p.scheme === 'TFHE' && (p.decompLevel || 0) > 0) maxMultDepth = 1000;
  return { noiseBudget, maxMultDepth };
}
function preset(scheme, security, polyDegree, moduli, lweDimension, lweNoiseStd, decompBaseLog, decompLevel,
  plaintextModulus) {
  const p = {
    scheme, security, polyDegree, moduli, lweDimension, lweNoiseStd, glweDimension: 1, decompBaseLog,
    decompLevel, plaintextModulus, noiseBudget: 0, maxMultDepth: 0,
  };
  Object.assign(p, calculateDerivedParameters(p));
  return p;
}
const Q = NTT_PRIMES;
const PRESET_FACTORIES = {
  'tfhe-128-fast': () => preset('TFHE', 128, 1024, [Q.Q_40_1], 742, 3.2e-11, 23, 1, 4n),
  'tfhe-128-balanced': () => preset('TFHE', 128, 2048, [Q.Q_50_1], 830, 2.9e-11, 15, 2, 8n),
  'tfhe-256-secure': () => preset('TFHE', 256, 4096, [Q.Q_60_1], 1024, 2.0e-12, 10, 3, 16n),
  'bfv-128-simd': () => preset('BFV', 128, 8192, [Q.Q_60_1, Q.Q_60_2, Q.Q_60_3], 0, 3.2, 60, 3, 65537n),
  'ckks-128-ml': () => preset('CKKS', 128, 16384, [Q.Q_60_1, Q.Q_50_1, Q.Q_50_2, Q.Q_40_1, Q.Q_40_2], 0, 3.2, 40, 5,
    1n << 40n),
  'tfhe-128-voting': () => preset('TFHE', 128, 1024, [Q.Q_40_1], 742, 3.2e-11, 23, 1, 16n),
};
/** createParameterSet / createCustomParameterSet (parameters/index.ts:296-347) */
function createParameterSet(params) {
  if (typeof params === 'string') {
    const f = PRESET_FACTORIES[params];
    if (!f) throw new FHEError(`Unknown parameter preset: ${params}`, FHEErrorCode.INVALID_PARAMETERS);
    return f();
  }
  if (!params || typeof params !== 'object' || !params.polyDegree || !params.moduli || !params.moduli.length) {
    throw new FHEError('Custom parameters need polyDegree and moduli', FHEErrorCode.INVALID_PARAMETERS);
  }
  const p = {
    scheme: params.scheme || (params.lweDimension ? 'TFHE' : 'BFV'),
    security: params.securityLevel || params.security || 128,
    polyDegree: params.polyDegree,
    moduli: params.moduli.map((m) => BigInt(m)),
    lweDimension: params.lweDimension || 0,
    lweNoiseStd: params.lweNoiseStd || 3.2e-11,
    glweDimension: params.glweDimension || 1,
    decompBaseLog: params.decompBaseLog || 23,
    decompLevel: params.decompLevel || 1,
    // createCustomParameterSet fixes t = 4; an explicit plaintextModulus is kept
    plaintextModulus: params.plaintextModulus !== undefined ? BigInt(params.plaintextModulus) : 4n,
    noiseBudget: 0,
    maxMultDepth: 0,
  };
  Object.assign(p, calculateDerivedParameters(p));
  return p;
}
function getAvailablePresets() {
  return ['tfhe-128-fast', 'tfhe-128-balanced', 'tfhe-256-secure', 'bfv-128-simd', 'ckks-128-ml'];
}

// ---------------------------------------------------------------- helpers
const SAMPLE = { UNIFORM: 0, TERNARY: 1, GAUSSIAN: 2, BINARY: 3, RAW: 4 };
const DIST = { TERNARY: SAMPLE.TERNARY, GAUSSIAN: SAMPLE.GAUSSIAN, BINARY: SAMPLE.BINARY, UNIFORM: SAMPLE.UNIFORM };
const SERIAL_MAGIC = 0x4d454846; // 'FHEM'
const KINDS = ['ciphertext', 'secret', 'public', 'evaluation', 'bootstrap'];

function u64(v) { return BigInt.asUintN(64, BigInt(v)); }
function modPow(b, e, m) {
  let r = 1n;
  b %= m;
  while (e > 0n) {
    if (e & 1n) r = (r * b) % m;
    b = (b * b) % m;
    e >>= 1n;
  }
  return r;
}
function toBigIntArray(words, count) {
  const out = new Array(count);
  for (let i = 0; i < count; i++) out[i] = words[i];
  return out;
}

/**
 * createEngine(params, options?) -> Promise<FHEEngine>
 * options: { mode: 'compat' | 'negacyclic', device, seed (Uint8Array(32) | bigint) }
 */
function makeEngineClass(native) {
  const { NttContext, DeviceBuffer } = native;
  // native state of every handle object (spread copies are not handles)
  const state = new WeakMap();

  class FHEEngineImpl {
    constructor(params, options) {
      const o = options || {};
      this._params = params;
      this._n = params.polyDegree;
      this._q = BigInt(params.moduli[0]);
      this._t = params.plaintextModulus ? BigInt(params.plaintextModulus) : 4n;
      this._tEff = this._t === 0n ? 4n : this._t;
      this._delta = this._q / this._tEff;
      // the C++ engines' error std (encryption.cpp:52-56: lwe_noise_std or 3.2)
      this._std = params.lweNoiseStd > 0 ? params.lweNoiseStd : 3.2;
      this._initialBudget = Math.log2(Number(this._q)) - Math.log2(2 * this._std * Math.sqrt(this._n));
      let env;
      try {
        env = envDefaults(o);
      } catch (err) {
        throw new FHEError(err.message, FHEErrorCode.INVALID_PARAMETERS);
      }
      const mode = env.mode === 'negacyclic' ? 1 : env.mode === 'compat' ? 0 : -1;
      if (mode < 0) throw new FHEError(`unknown mode ${env.mode}`, FHEErrorCode.INVALID_PARAMETERS);
      this._mode = mode;
      this._ctx = new NttContext(this._n, this._q, mode, env.devices || env.device);
      let seed = o.seed;
      if (seed === undefined) seed = crypto.randomBytes(32);
      if (typeof seed === 'bigint' || typeof seed === 'number') {
        const s = new BigUint64Array(4);
        let v = BigInt(seed);
        for (let i = 0; i < 4; i++) { s[i] = v & M64; v >>= 64n; }
        this._seed = s;
      } else {
        const b = Buffer.alloc(32);
        Buffer.from(seed).copy(b);
        this._seed = new BigUint64Array(b.buffer.slice(b.byteOffset, b.byteOffset + 32));
      }
      this._stream = 1n;
      this._nextKey = BigInt(Date.now()) * 1000n;
      this._disposed = false;
    }

    // ---- plumbing
    _check() {
      if (this._disposed) throw new FHEError('Engine disposed', FHEErrorCode.NATIVE_ERROR);
    }
    _streams(k) { const s = this._stream; this._stream += BigInt(k); return s; }
    _keyId() { this._nextKey += 1n; return this._nextKey; }
    _buf(words) { return new DeviceBuffer(this._ctx, words); }
    _upload(words) { return this._buf(words.length).upload(words); }
    _st(h, brand) {
      const s = h && typeof h === 'object' ? state.get(h) : undefined;
      if (!s || h.__brand !== brand || s.engine !== this) {
        throw new FHEError(`not a ${brand} handle of this engine`, FHEErrorCode.INVALID_PARAMETERS);
      }
      return s;
    }
    _handle(brand, fields, st) {
      const h = Object.assign({ __brand: brand, handle: st.buf ? st.buf.handle : 0n }, fields);
      st.engine = this;
      Object.freeze(h);
      state.set(h, st);
      return h;
    }
    _ct(buf, keyId, noiseBudget, degree, extra) {
      return this._handle('Ciphertext', { keyId, noiseBudget, isNtt: false, degree },
        Object.assign({ buf, kind: 'rlwe', comps: degree + 1, packed: false }, extra || {}));
    }
    _sameKey(a, b, what) {
      if (a.keyId !== b.keyId) throw new FHEError(`Cannot ${what} ciphertexts encrypted with different keys`, FHEErrorCode.KEY_MISMATCH);
    }
    _rlwe(ct) {
      const s = this._st(ct, 'Ciphertext');
      if (s.kind !== 'rlwe') throw new FHEError('operation needs an RLWE ciphertext (not a bootstrapped LWE one)', FHEErrorCode.INVALID_PARAMETERS);
      return s;
    }
    /** encode_plaintext / encode_packed slots (encryption.cpp:107-131): the raw
     *  slot values, n per ciphertext; the kernels scale by delta */
    _slots(pt) {
      if (!pt || pt.__brand !== 'Plaintext' || !Array.isArray(pt.values)) {
        throw new FHEError('expected a Plaintext', FHEErrorCode.INVALID_PARAMETERS);
      }
      const s = new BigUint64Array(this._n);
      if (pt.isPacked && pt.values.length > 1) {
        const m = Math.min(pt.values.length, this._n);
        for (let i = 0; i < m; i++) s[i] = u64(pt.values[i]);
      } else {
        s[0] = u64(pt.values.length ? pt.values[0] : 0n);
      }
      return s;
    }
    /** the encoded polynomial (v * delta mod 2^64) mod q of encode_* */
    _encoded(pt) {
      const s = this._slots(pt);
      for (let i = 0; i < s.length; i++) if (s[i]) s[i] = ((s[i] * this._delta) & M64) % this._q;
      return s;
    }
    _budgetOf(maxNoise) {
      const m = Math.max(Number(maxNoise), 1);
      return Math.log2(Number(this._q) / (2 * m));
    }

    // ---- keys (key_manager.cpp)
    async generateSecretKey(options) {
      this._check();
      return guard(async () => {
        const dist = options && options.distribution ? DIST[options.distribution] : SAMPLE.TERNARY;
        if (dist === undefined) throw new FHEError(`unknown distribution ${options.distribution}`, FHEErrorCode.INVALID_PARAMETERS);
        const sk = this._buf(this._n);
        await this._ctx.sampleAsync(dist, this._seed, this._streams(1), this._std, sk);
        const prep = this._buf(2 * this._n);
        await this._ctx.prepareSecretKeyAsync(sk, prep);
        return this._handle('SecretKey', { keyId: this._keyId() }, { buf: sk, prep });
      });
    }
    async generatePublicKey(sk) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        const pk = this._buf(2 * this._n);
        await this._ctx.publicKeyGenerateAsync(s.buf, this._seed, this._streams(2), this._std, pk);
        const prep = this._buf(2 * this._n);
        await this._ctx.preparePublicKeyAsync(pk, prep);
        return this._handle('PublicKey', { keyId: sk.keyId }, { buf: pk, prep });
      });
    }
    /** generate_eval_key (:252-333); levels limited to (level - 1) * baseLog < 64
     *  (relinearize's digit shift) */
    async generateEvalKey(sk, options) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        const o = typeof options === 'number' ? { decompBaseLog: options } : (options || {});
        const bl = o.decompBaseLog || this._params.decompBaseLog || 4;
        const lv = Math.min(o.decompLevel || this._params.decompLevel || 3, Math.floor(63 / bl) + 1);
        if (bl < 1 || bl > 63) throw new FHEError('decompBaseLog must be in [1, 63]', FHEErrorCode.INVALID_PARAMETERS);
        const rlk = this._buf(lv * 2 * this._n);
        await this._ctx.evalKeyGenerateAsync(s.buf, bl, lv, this._seed, this._streams(2 * lv), this._std, rlk);
        const prep = this._buf(lv * 2 * this._n);
        await this._ctx.prepareRelinKeyAsync(rlk, prep);
        return this._handle('EvaluationKey', { keyId: sk.keyId, decompBaseLog: bl, decompLevel: lv },
          { buf: rlk, prep, baseLog: bl, level: lv });
      });
    }
    /** BootstrapEngine::generate_bootstrap_key (bootstrap_engine.cpp:308-360)
     *  with a fresh binary LWE key of the parameter set's lweDimension:
     *  GGSW encryptions of its bits (encrypt_ggsw :268-306) and the key
     *  switching key back to it (:367-420).  The LWE key stays with the
     *  secret key's native state (decrypt of bootstrapped ciphertexts). */
    async generateBootstrapKey(sk) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        const dim = this._params.lweDimension | 0;
        const k = this._params.glweDimension || 1;
        if (dim <= 0) throw new FHEError('parameter set has no LWE dimension (not a TFHE set)', FHEErrorCode.INVALID_PARAMETERS);
        if (k !== 1) throw new FHEError('bootstrapping keys implemented for GLWE dimension 1', FHEErrorCode.INVALID_PARAMETERS);
        const bl = this._params.decompBaseLog > 0 ? this._params.decompBaseLog : 4;
        const lv = this._params.decompLevel > 0 ? this._params.decompLevel : 3;
        const lweDev = this._buf(dim);
        await this._ctx.sampleAsync(SAMPLE.BINARY, this._seed, this._streams(1), 0, lweDev);
        const lweSk = new BigInt64Array(lweDev.download().buffer);
        const n = this._n;
        const bsk = this._buf(dim * 2 * lv * 2 * n);
        await this._ctx.ggswEncryptAsync(lweDev, s.buf, 1, bl, lv, this._seed, this._streams(2), this._std, bsk);
        const bskPrep = this._buf(dim * 2 * lv * 2 * n);
        await this._ctx.prepareGgswAsync(bsk, 1, lv, bskPrep);
        bsk.free();
        const kskA = this._buf(n * lv * dim), kskB = this._buf(n * lv);
        await this._ctx.kskGenerateAsync(s.buf, lweDev, bl, lv, this._seed, this._streams(2), this._std, kskA, kskB);
        s.lweSk = lweSk;
        s.lweDev = lweDev;
        const tp = this._upload(this._identityTestPoly());
        return this._handle('BootstrapKey', { keyId: sk.keyId, lweDimension: dim },
          { buf: bskPrep, bskPrep, kskA, kskB, baseLog: bl, level: lv, ksBaseLog: bl, ksLevel: lv, dim, testPoly: tp });
      });
    }
    /** init_default_test_poly (bootstrap_engine.cpp:57-77) */
    _identityTestPoly() {
      const n = BigInt(this._n), c = new BigUint64Array(this._n);
      for (let i = 0n; i < n; i++) c[Number(i)] = ((((i * this._tEff) / (2n * n)) * this._delta) & M64) % this._q;
      return c;
    }
    /** create_lookup_table (:725-758) over a table f[v], v < lut.length */
    _lutPoly(lut) {
      const n = BigInt(this._n), inMod = BigInt(lut.length), outMod = this._tEff, dOut = this._q / outMod;
      const c = new BigUint64Array(this._n);
      for (let i = 0n; i < n; i++) {
        const v = ((i * inMod + n) / (2n * n)) % inMod;
        c[Number(i)] = (((BigInt(lut[Number(v)]) % outMod) * dOut) & M64) % this._q;
      }
      return c;
    }

    /** KeyManager::generate_threshold_keys (key_manager.cpp:479-560): Shamir
     *  shares s_i = sum_j coeff_j i^j of a fresh ternary master key
     *  (coefficients j >= 1 uniform), all shares in one launch. */
    async generateThresholdKeys(config) {
      this._check();
      return guard(async () => {
        const t = config && config.threshold | 0, total = config && config.totalShares | 0;
        if (t <= 0 || t > total) throw new FHEError('Invalid threshold parameters', FHEErrorCode.INVALID_PARAMETERS);
        const n = this._n;
        const master = await this.generateSecretKey();
        const coeffs = this._buf(t * n);
        coeffs.view(0, n).copyFrom(state.get(master).buf);
        for (let j = 1; j < t; j++) {
          await this._ctx.sampleAsync(SAMPLE.UNIFORM, this._seed, this._streams(1), 0, coeffs.view(j * n, n));
        }
        const all = this._buf(total * n);
        await this._ctx.shamirSharesAsync(coeffs, total, all);
        coeffs.free();
        const words = all.download();
        const shares = [];
        for (let i = 1; i <= total; i++) {
          const buf = all.view((i - 1) * n, n);
          const bytes = Buffer.from(words.buffer, words.byteOffset + (i - 1) * n * 8, n * 8);
          const commitment = new Uint8Array(crypto.createHash('sha256').update(bytes).digest());
          const h = Object.freeze({ shareId: i, handle: buf.handle, commitment, keyId: master.keyId });
          state.set(h, { engine: this, buf });
          shares.push(h);
        }
        const publicKey = await this.generatePublicKey(master);
        return { shares, publicKey, threshold: t, totalShares: total };
      });
    }
    /** the share's state, its NTT-domain form prepared on first use and kept */
    async _share(share) {
      const s = share && state.get(share);
      if (!s || s.engine !== this || share.shareId === undefined) {
        throw new FHEError('not a key share of this engine', FHEErrorCode.INVALID_PARAMETERS);
      }
      if (!s.prep) {
        const prep = this._buf(this._n);
        await this._ctx.prepareKeySharesAsync(s.buf, prep);
        s.prep = prep;
      }
      return s;
    }
    /** partial decryptions of cts with one share: one launch over the batch */
    async _partials(cts, share) {
      const n = this._n, B = cts.length;
      const cs = cts.map((ct) => this._rlwe(ct));
      const s = await this._share(share);
      for (const ct of cts) {
        if (share.keyId !== ct.keyId) throw new FHEError('Key share does not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
      }
      let all = cs[0].buf;
      if (B > 1 || cs[0].comps !== 2) {
        all = this._buf(B * 2 * n);
        cs.forEach((c, i) => all.view(i * 2 * n, 2 * n).copyFrom(c.comps === 2 ? c.buf : c.buf.view(0, 2 * n)));
      }
      const p = this._buf(B * n);
      await this._ctx.partialDecryptPreparedAsync(s.prep, all, p);
      const w = p.download();
      if (all !== cs[0].buf) all.free();
      p.free();
      return cts.map((_, i) => ({ shareId: share.shareId, partialResult: toBigIntArray(w.subarray(i * n, (i + 1) * n), n) }));
    }
    /** KeyManager::partial_decrypt (:584-601): c1 (*) share */
    async partialDecrypt(ct, share) {
      this._check();
      return guard(async () => (await this._partials([ct], share))[0]);
    }
    /** partialDecrypt of every ciphertext with one share, one launch */
    async partialDecryptBatch(cts, share) {
      this._check();
      return guard(async () => {
        if (!Array.isArray(cts)) throw new FHEError('expected an array of ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
        return cts.length ? this._partials(cts, share) : [];
      });
    }
    /** lagrange_coefficient (:566-582) for the first t of the partials' ids, over all of them */
    _lambdas(ids, t) {
      const q = this._q, out = new BigUint64Array(t);
      for (let i = 0; i < t; i++) {
        let num = 1n, den = 1n;
        for (const j of ids) {
          if (j === ids[i]) continue;
          num = (num * j) % q;
          den = (den * (((j - ids[i]) % q + q) % q)) % q;
        }
        out[i] = (num * modPow(den, q - 2n, q)) % q;
      }
      return out;
    }
    /** combine (:604-632) + c0 - sum + decode of cts, partials[i][b] trustee i's
     *  partial of ciphertext b: one upload, one launch, no host decode */
    async _combine(cts, partials, t) {
      const n = this._n, B = cts.length;
      const cs = cts.map((ct) => this._rlwe(ct));
      if (!Array.isArray(partials) || partials.length < t || t < 1) {
        throw new FHEError(`Need ${t} partials, got ${partials ? partials.length : 0}`, FHEErrorCode.THRESHOLD_NOT_MET);
      }
      for (const list of partials) {
        if (!Array.isArray(list) || list.length !== B) {
          throw new FHEError('every trustee needs one partial decryption per ciphertext', FHEErrorCode.INVALID_PARAMETERS);
        }
        if (list.some((p) => p.shareId !== list[0].shareId)) {
          throw new FHEError('the partial decryptions of one trustee carry one share id', FHEErrorCode.INVALID_PARAMETERS);
        }
      }
      const lam = this._lambdas(partials.map((list) => BigInt(list[0].shareId)), t);
      const host = new BigUint64Array(t * B * n);
      for (let i = 0; i < t; i++) {
        for (let b = 0; b < B; b++) {
          const r = partials[i][b].partialResult, o = (i * B + b) * n;
          for (let k = 0; k < n; k++) host[o + k] = u64(r[k]);
        }
      }
      const pb = this._upload(host);
      let all = cs[0].buf;
      if (B > 1 || cs[0].comps !== 2) {
        all = this._buf(B * 2 * n);
        cs.forEach((c, i) => all.view(i * 2 * n, 2 * n).copyFrom(c.comps === 2 ? c.buf : c.buf.view(0, 2 * n)));
      }
      const vals = this._buf(B * n), mx = this._buf(B);
      await this._ctx.combinePartialsAsync(this._t, all, pb, lam, vals, mx);
      const v = vals.download(), m = mx.download();
      if (all !== cs[0].buf) all.free();
      pb.free(); vals.free(); mx.free();
      return cs.map((c, b) => ({ vals: v.slice(b * n, (b + 1) * n), maxNoise: m[b], packed: c.packed }));
    }
    /** combine_partial_decryptions (:604-632) with lagrange_coefficient
     *  (:566-582), then c0 - sum and decode (decode_packed :150-163) */
    async combinePartialDecryptions(ct, partials, t) {
      this._check();
      return guard(async () => {
        const lists = Array.isArray(partials) ? partials.map((p) => [p]) : partials;
        const r = (await this._combine([ct], lists, t))[0];
        return this._decryptionResult(r.vals, null, r.packed);
      });
    }
    /** combinePartialDecryptions of every ciphertext, partials[i] trustee i's
     *  list index-aligned with cts: one launch; the budget is the measured one */
    async combinePartialDecryptionsBatch(cts, partials, t) {
      this._check();
      return guard(async () => {
        if (!Array.isArray(cts)) throw new FHEError('expected an array of ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
        if (!cts.length) return [];
        return (await this._combine(cts, partials, t)).map((r) => this._decryptionResult(r.vals, r.maxNoise, r.packed));
      });
    }

    // ---- encrypt / decrypt (encryption.cpp:171-348)
    async encrypt(plaintext, pk) {
      this._check();
      return guard(async () => {
        const p = this._st(pk, 'PublicKey');
        const slots = this._slots(plaintext);
        const ct = this._buf(2 * this._n);
        await this._ctx.encryptSampledAsync(this._t, p.prep, this._upload(slots), this._seed, this._streams(3), this._std, ct);
        return { ciphertext: this._ct(ct, pk.keyId, this._initialBudget, 1, { packed: !!(plaintext.isPacked && plaintext.values.length > 1) }) };
      });
    }
    async encryptValue(value, pk) { return (await this.encrypt(this.createPlaintext(value), pk)).ciphertext; }
    async encryptPacked(values, pk) { return (await this.encrypt(this.createPackedPlaintext(values), pk)).ciphertext; }
    async getZeroCiphertext(pk) { return this.encryptValue(0n, pk); }
    /** batch_encrypt (encryption.cpp:460-540): one device launch for the whole batch */
    async batchEncrypt(pts, pk, opts) {
      this._check();
      return guard(async () => {
        const p = this._st(pk, 'PublicKey');
        const start = Date.now(), n = this._n, B = pts.length;
        if (B === 0) return { ciphertexts: [], elapsedMs: 0, throughputPerSecond: 0 };
        const slots = new BigUint64Array(B * n);
        pts.forEach((pt, i) => slots.set(this._slots(pt), i * n));
        const all = this._buf(2 * n * B);
        await this._ctx.encryptSampledAsync(this._t, p.prep, this._upload(slots), this._seed, this._streams(3), this._std, all);
        const ciphertexts = pts.map((pt, i) => this._ct(all.view(2 * n * i, 2 * n), pk.keyId, this._initialBudget, 1,
          { packed: !!(pt.isPacked && pt.values.length > 1) }));
        const ms = Date.now() - start;
        return { ciphertexts, elapsedMs: ms, throughputPerSecond: ms > 0 ? (B * 1000) / ms : 0 };
      });
    }
    _decryptionResult(vals, maxNoise, packed) {
      const budget = maxNoise === null ? this._initialBudget : this._budgetOf(maxNoise);
      const values = packed ? toBigIntArray(vals, this._n) : [vals[0]];
      const r = {
        plaintext: Object.freeze({ __brand: 'Plaintext', values, plaintextModulus: this._tEff, isPacked: !!packed }),
        remainingNoiseBudget: budget,
        success: budget >= 0,
      };
      if (!r.success) r.errorMessage = 'Noise budget exhausted - decryption may be incorrect';
      r._slots = vals;
      return r;
    }
    async _decryptRaw(ct, sk) {
      const c = this._st(ct, 'Ciphertext'), s = this._st(sk, 'SecretKey');
      if (ct.keyId !== sk.keyId) return { mismatch: true };
      if (c.kind === 'lwe') {
        if (!s.lweSk) throw new FHEError('no LWE key: generateBootstrapKey(sk) was not called', FHEErrorCode.INVALID_PARAMETERS);
        const v = this._buf(1), ph = this._buf(1);
        await this._ctx.lweDecryptAsync(this._t, s.lweDev, c.buf.view(0, c.dim), c.buf.view(c.dim, 1), v, ph);
        const phase = ph.download()[0];
        // the LWE noise: distance of the phase to round(p t / q) delta (compute_noise_budget's measure)
        const r = ((phase * this._tEff + this._q / 2n) / this._q);
        const exp = ((r * this._delta) & M64) % this._q;
        let d = phase >= exp ? phase - exp : exp - phase;
        if (d > this._q / 2n) d = this._q - d;
        const vals = new BigUint64Array(this._n);
        vals[0] = v.download()[0];
        return { vals, maxNoise: d, packed: false };
      }
      const vals = this._buf(this._n), mx = this._buf(1);
      await this._ctx.decryptAsync(this._t, s.prep, c.buf, c.comps, ct.isNtt ? 1 : 0, vals, mx);
      return { vals: vals.download(), maxNoise: mx.download()[0], packed: c.packed };
    }
    async decrypt(ct, sk) {
      this._check();
      return guard(async () => {
        const r = await this._decryptRaw(ct, sk);
        if (r.mismatch) {
          return { plaintext: Object.freeze({ __brand: 'Plaintext', values: [], plaintextModulus: this._tEff, isPacked: false }),
            remainingNoiseBudget: 0, success: false,
            errorMessage: 'Key ID mismatch: ciphertext was encrypted with different key' };
        }
        return this._decryptionResult(r.vals, r.maxNoise, r.packed);
      });
    }
    async decryptValue(ct, sk) {
      const r = await this.decrypt(ct, sk);
      if (!r.success) throw new FHEError(r.errorMessage || 'Decryption failed', FHEErrorCode.NOISE_BUDGET_EXHAUSTED);
      return r.plaintext.values.length ? r.plaintext.values[0] : 0n;
    }
    async decryptPacked(ct, sk, numValues) {
      const r = await this.decrypt(ct, sk);
      if (!r.success) throw new FHEError(r.errorMessage || 'Decryption failed', FHEErrorCode.NOISE_BUDGET_EXHAUSTED);
      return toBigIntArray(r._slots, Math.min(numValues, this._n));
    }
    async getNoiseBudget(ct, sk) {
      this._check();
      return guard(async () => {
        const r = await this._decryptRaw(ct, sk);
        if (r.mismatch) throw new FHEError('Key ID mismatch', FHEErrorCode.KEY_MISMATCH);
        return this._budgetOf(r.maxNoise);
      });
    }
    /** estimate_noise_budget (:446-450): the tracked estimate */
    estimateNoiseBudget(ct) {
      this._check();
      this._st(ct, 'Ciphertext');
      return ct.noiseBudget;
    }

    // ---- additive operations (encryption.cpp:594-735)
    async _addsub(ct1, ct2, sub) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct1), b = this._rlwe(ct2);
        this._sameKey(ct1, ct2, sub ? 'subtract' : 'add');
        if (ct1.isNtt !== ct2.isNtt) throw new FHEError('Cannot combine ciphertexts in different representations (NTT vs coefficient)', FHEErrorCode.INVALID_PARAMETERS);
        if (a.comps !== b.comps) throw new FHEError('ciphertext degrees differ', FHEErrorCode.INVALID_PARAMETERS);
        const out = this._buf(a.comps * this._n);
        await (sub ? this._ctx.subAsync(a.buf, b.buf, out) : this._ctx.addAsync(a.buf, b.buf, out));
        return this._ct(out, ct1.keyId, Math.min(ct1.noiseBudget, ct2.noiseBudget) - 1, ct1.degree,
          { packed: a.packed || b.packed });
      });
    }
    async add(ct1, ct2) { return this._addsub(ct1, ct2, false); }
    async subtract(ct1, ct2) { return this._addsub(ct1, ct2, true); }
    async negate(ct) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct);
        const out = this._buf(a.comps * this._n);
        await this._ctx.negateAsync(a.buf, out);
        return this._ct(out, ct.keyId, ct.noiseBudget, ct.degree, { packed: a.packed });
      });
    }
    /** add_plain (:638-665): c0 + encode(pt), the rest copied; budget - 0.5 */
    async addPlain(ct, pt) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct), n = this._n;
        const out = this._buf(a.comps * n);
        await this._ctx.addPlainAsync(this._t, a.buf.view(0, 2 * n), this._upload(this._slots(pt)), ct.isNtt ? 1 : 0,
          out.view(0, 2 * n));
        if (a.comps === 3) out.copyFrom(a.buf, 2 * n, 2 * n, n);
        return this._ct(out, ct.keyId, ct.noiseBudget - 0.5, ct.degree,
          { packed: a.packed || !!(pt.isPacked && pt.values.length > 1) });
      });
    }
    /** add_scalar (:685-688) */
    async addScalar(ct, value) { return this.addPlain(ct, this.createPlaintext(value)); }
    /** The checks a chain of add() makes over a whole list, in its order: the
     *  running sum keeps the first key and degree and is in coefficient
     *  form from the first addition on. */
    _sumInputs(cts) {
      const first = this._rlwe(cts[0]);
      const run = { keyId: cts[0].keyId, isNtt: cts[0].isNtt, comps: first.comps };
      const bufs = [first.buf];
      let packed = first.packed;
      for (let i = 1; i < cts.length; i++) {
        const b = this._rlwe(cts[i]);
        this._sameKey(run, cts[i], 'add');
        if (run.isNtt !== cts[i].isNtt) throw new FHEError('Cannot combine ciphertexts in different representations (NTT vs coefficient)', FHEErrorCode.INVALID_PARAMETERS);
        if (run.comps !== b.comps) throw new FHEError('ciphertext degrees differ', FHEErrorCode.INVALID_PARAMETERS);
        run.isNtt = false;
        run.comps = cts[0].degree + 1;
        bufs.push(b.buf);
        packed = packed || b.packed;
      }
      return { bufs, packed, comps: run.comps };
    }
    /** One launch over every input (fhe_ct_sum_ptrs); the words equal the chain's and the tree's */
    async _sum(cts, noiseBudget) {
      const f = this._sumInputs(cts);
      const out = this._buf(f.comps * this._n);
      await this._ctx.sumAsync(f.bufs, out);
      return this._ct(out, cts[0].keyId, noiseBudget, cts[0].degree, { packed: f.packed });
    }
    /** batch_add (:1327-1364) as a chain of add(): budget min - 1 per input */
    async batchAdd(cts, progress) {
      this._check();
      if (!Array.isArray(cts) || cts.length === 0) throw new FHEError('Empty array', FHEErrorCode.INVALID_PARAMETERS);
      if (cts.length === 1) return cts[0];
      const start = Date.now();
      let budget = cts[0].noiseBudget;
      for (let i = 1; i < cts.length; i++) budget = Math.min(budget, cts[i].noiseBudget) - 1;
      const r = await guard(async () => this._sum(cts, budget));
      for (let i = 1; progress && i < cts.length; i++) {
        progress({ stage: 'batch_add', current: i + 1, total: cts.length, elapsedMs: Date.now() - start,
          progressPercent: ((i + 1) / cts.length) * 100 });
      }
      return r;
    }

    // ---- ballot aggregation (encryption.cpp:1061-1168)
    /** tally_votes (:1061-1067) = batch_add_tree (:1366-1458): budget min - 1
     *  per tree level, an odd element carried up unchanged; progress counts
     *  the count - 1 additions */
    async tallyVotes(ballots, progress) {
      this._check();
      if (!Array.isArray(ballots) || ballots.length === 0) {
        throw new FHEError('Cannot add empty vector of ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
      }
      const start = Date.now();
      let level = ballots.map((b) => b.noiseBudget);
      while (level.length > 1) {
        const next = [];
        for (let i = 0; i + 1 < level.length; i += 2) next.push(Math.min(level[i], level[i + 1]) - 1);
        if (level.length % 2 === 1) next.push(level[level.length - 1]);
        level = next;
      }
      const r = await guard(async () => this._sum(ballots, level[0]));
      const total = ballots.length - 1;
      for (let i = 1; progress && i <= total; i++) {
        progress({ stage: 'tally_votes', current: i, total, elapsedMs: Date.now() - start, progressPercent: (i / total) * 100 });
      }
      return r;
    }
    /** tally_multi_candidate (:1153-1168): packed ballots, one slot per candidate */
    async tallyMultiCandidate(ballots, numCandidates, progress) {
      this._check();
      if (numCandidates > this._n) {
        throw new FHEError('Number of candidates exceeds polynomial degree', FHEErrorCode.INVALID_PARAMETERS);
      }
      return this.tallyVotes(ballots, progress);
    }
    /** update_tally (:1145-1151) */
    async updateTally(tally, ballot) { return this.add(tally, ballot); }
    /** tally_weighted_votes (:1069-1110): multiply + relinearize per ballot
     *  (progress every 100, of 2 * count), then one tally (progress count +
     *  completed of count + (count - 1)) */
    async tallyWeightedVotes(ballots, weights, ek, progress, options) {
      this._check();
      if (!Array.isArray(ballots) || !Array.isArray(weights) || ballots.length !== weights.length) {
        throw new FHEError('Ballots and weights must have the same size', FHEErrorCode.INVALID_PARAMETERS);
      }
      if (ballots.length === 0) throw new FHEError('Cannot tally empty ballot list', FHEErrorCode.INVALID_PARAMETERS);
      const mode = options && options.relinearize !== undefined ? options.relinearize : 'each';
      if (mode !== 'each' && mode !== 'once') {
        throw new FHEError("options.relinearize must be 'each' or 'once'", FHEErrorCode.INVALID_PARAMETERS);
      }
      const start = Date.now(), total = ballots.length;
      const report = (current, of) => progress({ stage: 'tally_weighted_votes', current, total: of,
        elapsedMs: Date.now() - start, progressPercent: (current / of) * 100 });
      if (options && options.scaled) {
        // the scale-invariant inner product (one rescale by t/q after the sum),
        // then one relinearisation: opens to sum w_i b_i with real keys
        const r = await this.relinearize(await this.dotProductScaled(ballots, weights), ek);
        for (let i = 0; progress && i < total; i++) if ((i + 1) % 100 === 0) report(i + 1, total * 2);
        for (let i = 1; progress && i < total; i++) report(total + i, total + total - 1);
        return r;
      }
      if (mode === 'once') {
        // lazy relinearisation: the fused degree-2 sum, then one key switch.
        // Same plaintext, less noise; not the words of the per-ballot fold
        // (the digit decomposition is not linear).  Same progress calls.
        const r = await this.relinearize(await this.dotProduct(ballots, weights), ek);
        for (let i = 0; progress && i < total; i++) if ((i + 1) % 100 === 0) report(i + 1, total * 2);
        for (let i = 1; progress && i < total; i++) report(total + i, total + total - 1);
        return r;
      }
      const weighted = [];
      for (let i = 0; i < total; i++) {
        weighted.push(await this.multiplyRelin(ballots[i], weights[i], ek));
        if (progress && (i + 1) % 100 === 0) report(i + 1, total * 2);
      }
      return this.tallyVotes(weighted, progress ? (p) => report(total + p.current, total + p.total) : undefined);
    }
    /** Ciphertext inner product sum_i multiply(cts1[i], cts2[i]) as one
     *  degree-2 ciphertext, in one fused launch (fhe_ct_dot_ptrs); the words
     *  equal the chain of multiply() and add().  Checks in that chain's
     *  order (every pair shares cts1[0]'s representation); budget: multiply's
     *  rule per pair, folded by tallyVotes' tree rule; progress counts the
     *  pairs. */
    async dotProduct(cts1, cts2, progress) {
      this._check();
      if (!Array.isArray(cts1) || !Array.isArray(cts2) || cts1.length !== cts2.length) {
        throw new FHEError('Ballots and weights must have the same size', FHEErrorCode.INVALID_PARAMETERS);
      }
      if (cts1.length === 0) throw new FHEError('Cannot tally empty ballot list', FHEErrorCode.INVALID_PARAMETERS);
      const start = Date.now(), total = cts1.length;
      const r = await guard(async () => {
        const A = [], B = [];
        const red = Math.log2(this._n) + 5;
        let level = [], packed = false;
        for (let i = 0; i < total; i++) {
          const a = this._rlwe(cts1[i]), b = this._rlwe(cts2[i]);
          this._sameKey(cts1[i], cts2[i], 'multiply');
          if (a.comps !== 2 || b.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
          if (i > 0) {
            this._sameKey(cts1[0], cts1[i], 'add');
            if (cts1[i].isNtt !== cts1[0].isNtt) throw new FHEError('Cannot combine ciphertexts in different representations (NTT vs coefficient)', FHEErrorCode.INVALID_PARAMETERS);
          }
          A.push(a.buf);
          B.push(b.buf);
          packed = packed || a.packed || b.packed;
          level.push(Math.min(cts1[i].noiseBudget, cts2[i].noiseBudget) - red);
        }
        while (level.length > 1) {
          const next = [];
          for (let i = 0; i + 1 < level.length; i += 2) next.push(Math.min(level[i], level[i + 1]) - 1);
          if (level.length % 2 === 1) next.push(level[level.length - 1]);
          level = next;
        }
        const out = this._buf(3 * this._n);
        await this._ctx.dotAsync(A, B, out, !!cts1[0].isNtt);
        return this._ct(out, cts1[0].keyId, level[0], 2, { packed });
      });
      for (let i = 1; progress && i <= total; i++) {
        progress({ stage: 'dot_product', current: i, total, elapsedMs: Date.now() - start, progressPercent: (i / total) * 100 });
      }
      return r;
    }
    // ---- scale-invariant BFV products (fhe_ct_multiply_scaled_batch,
    // fhe_ct_dot_scaled_batch, fhe_ct_square_scaled_batch): round(t/q (ct1 (x)
    // ct2)) over the integers.  The result carries Delta m (multiply()'s
    // carries Delta^2 m) and opens with real keys after relinearize(); its
    // phase is c0 - c1 s + c2 s^2, so decrypt() of the degree-2 result is not
    // the way to open it.  Mode 'negacyclic', coefficient form, one device.
    _scaledPair(ct1, ct2) {
      const a = this._rlwe(ct1), b = this._rlwe(ct2);
      this._sameKey(ct1, ct2, 'multiply');
      if (a.comps !== 2 || b.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
      if (ct1.isNtt || ct2.isNtt) throw new FHEError('scaled products take coefficient-form ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
      return [a, b];
    }
    async multiplyScaled(ct1, ct2) {
      this._check();
      return guard(async () => {
        const [a, b] = this._scaledPair(ct1, ct2);
        const out = this._buf(3 * this._n);
        await this._ctx.ctMultiplyScaledAsync(this._t, a.buf, b.buf, out);
        const red = Math.log2(this._n) + 5;
        return this._ct(out, ct1.keyId, Math.min(ct1.noiseBudget, ct2.noiseBudget) - red, 2, { packed: a.packed || b.packed });
      });
    }
    async squareScaled(ct) {
      this._check();
      return guard(async () => {
        const [a] = this._scaledPair(ct, ct);
        const out = this._buf(3 * this._n);
        await this._ctx.ctSquareScaledAsync(this._t, a.buf, null, out);
        return this._ct(out, ct.keyId, ct.noiseBudget - (Math.log2(this._n) + 5), 2, { packed: a.packed });
      });
    }
    /** sum_i cts1[i] (x) cts2[i] with ONE rescale after the sum: one rounding
     *  error instead of count, so not the words of a sum of multiplyScaled() */
    async dotProductScaled(cts1, cts2, progress) {
      this._check();
      if (!Array.isArray(cts1) || !Array.isArray(cts2) || cts1.length !== cts2.length) {
        throw new FHEError('Ballots and weights must have the same size', FHEErrorCode.INVALID_PARAMETERS);
      }
      if (cts1.length === 0) throw new FHEError('Cannot tally empty ballot list', FHEErrorCode.INVALID_PARAMETERS);
      const start = Date.now(), total = cts1.length, w = 2 * this._n;
      const r = await guard(async () => {
        const A = this._buf(total * w), B = this._buf(total * w);
        let budget = Infinity, packed = false;
        for (let i = 0; i < total; i++) {
          const [a, b] = this._scaledPair(cts1[i], cts2[i]);
          if (i > 0) this._sameKey(cts1[0], cts1[i], 'add');
          A.copyFrom(a.buf, i * w);
          B.copyFrom(b.buf, i * w);
          packed = packed || a.packed || b.packed;
          budget = Math.min(budget, cts1[i].noiseBudget, cts2[i].noiseBudget);
        }
        const out = this._buf(3 * this._n);
        await this._ctx.ctDotScaledAsync(this._t, A, B, total, out);
        A.free();
        B.free();
        const red = Math.log2(this._n) + 5 + Math.ceil(Math.log2(total));
        return this._ct(out, cts1[0].keyId, budget - red, 2, { packed });
      });
      for (let i = 1; progress && i <= total; i++) {
        progress({ stage: 'dot_product_scaled', current: i, total, elapsedMs: Date.now() - start, progressPercent: (i / total) * 100 });
      }
      return r;
    }
    /** Public integer weights: sum_i multiplyScalar(ballots[i], weights[i])
     *  folded by add(), in one launch (fhe_ct_sum_scaled_ptrs); the words
     *  equal that chain's.  Checks in tallyVotes' order after the length
     *  check; budget: multiplyScalar's - 1 per ballot, folded by tallyVotes'
     *  tree rule; progress counts the count - 1 additions. */
    async tallyScalarWeightedVotes(ballots, weights, progress) {
      this._check();
      if (!Array.isArray(ballots) || !Array.isArray(weights) || ballots.length !== weights.length) {
        throw new FHEError('Ballots and weights must have the same size', FHEErrorCode.INVALID_PARAMETERS);
      }
      if (ballots.length === 0) {
        throw new FHEError('Cannot add empty vector of ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
      }
      const start = Date.now();
      let level = ballots.map((b) => b.noiseBudget - 1);
      while (level.length > 1) {
        const next = [];
        for (let i = 0; i + 1 < level.length; i += 2) next.push(Math.min(level[i], level[i + 1]) - 1);
        if (level.length % 2 === 1) next.push(level[level.length - 1]);
        level = next;
      }
      const r = await guard(async () => {
        const f = this._sumInputs(ballots);
        const scalars = new BigUint64Array(weights.length);
        for (let i = 0; i < weights.length; i++) scalars[i] = u64(weights[i]);
        const out = this._buf(f.comps * this._n);
        await this._ctx.sumScaledAsync(f.bufs, scalars, out);
        return this._ct(out, ballots[0].keyId, level[0], ballots[0].degree, { packed: f.packed });
      });
      const total = ballots.length - 1;
      for (let i = 1; progress && i <= total; i++) {
        progress({ stage: 'tally_scalar_weighted_votes', current: i, total, elapsedMs: Date.now() - start,
          progressPercent: (i / total) * 100 });
      }
      return r;
    }
    /** Public plaintext weights: sum_i multiplyPlain(cts[i], pts[i]) as one
     *  degree-1 ciphertext, in one fused launch (fhe_ct_dot_plain_ptrs); the
     *  words equal the chain of multiplyPlain() and add().  The plaintexts
     *  are encoded as multiplyPlain's (_encoded), one upload per distinct
     *  Plaintext object.  Degree-1 ciphertexts only; every ciphertext shares
     *  cts[0]'s key and representation; budget: multiplyPlain's - 2 per
     *  ballot, folded by tallyVotes' tree rule; progress counts the pairs. */
    async dotPlain(cts, pts, progress) {
      this._check();
      if (!Array.isArray(cts) || !Array.isArray(pts) || cts.length !== pts.length) {
        throw new FHEError('Ballots and weights must have the same size', FHEErrorCode.INVALID_PARAMETERS);
      }
      if (cts.length === 0) throw new FHEError('Cannot tally empty ballot list', FHEErrorCode.INVALID_PARAMETERS);
      const start = Date.now(), total = cts.length;
      const r = await guard(async () => {
        const A = [], P = [], uploaded = new Map();
        let level = [], packed = false;
        for (let i = 0; i < total; i++) {
          const a = this._rlwe(cts[i]);
          if (a.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
          if (i > 0) {
            this._sameKey(cts[0], cts[i], 'add');
            if (cts[i].isNtt !== cts[0].isNtt) throw new FHEError('Cannot combine ciphertexts in different representations (NTT vs coefficient)', FHEErrorCode.INVALID_PARAMETERS);
          }
          let p = uploaded.get(pts[i]);
          if (!p) {
            p = this._upload(this._encoded(pts[i]));
            uploaded.set(pts[i], p);
          }
          A.push(a.buf);
          P.push(p);
          packed = packed || a.packed;
          level.push(cts[i].noiseBudget - 2);
        }
        while (level.length > 1) {
          const next = [];
          for (let i = 0; i + 1 < level.length; i += 2) next.push(Math.min(level[i], level[i + 1]) - 1);
          if (level.length % 2 === 1) next.push(level[level.length - 1]);
          level = next;
        }
        const out = this._buf(2 * this._n);
        await this._ctx.dotPlainAsync(A, P, out, !!cts[0].isNtt);
        return this._ct(out, cts[0].keyId, level[0], 1, { packed });
      });
      for (let i = 1; progress && i <= total; i++) {
        progress({ stage: 'dot_plain', current: i, total, elapsedMs: Date.now() - start, progressPercent: (i / total) * 100 });
      }
      return r;
    }

    // ---- multiplicative operations (encryption.cpp:737-980)
    async multiply(ct1, ct2) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct1), b = this._rlwe(ct2);
        this._sameKey(ct1, ct2, 'multiply');
        if (a.comps !== 2 || b.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
        const out = this._buf(3 * this._n);
        await this._ctx.ctMultiplyAsync(a.buf, b.buf, out, ct1.isNtt ? 1 : 0);
        const red = Math.log2(this._n) + 5;
        return this._ct(out, ct1.keyId, Math.min(ct1.noiseBudget, ct2.noiseBudget) - red, 2,
          { packed: a.packed || b.packed });
      });
    }
    async relinearize(ct, ek) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct);
        if (a.comps === 2) {  // already degree 1: a copy (:906-909)
          const out = this._buf(2 * this._n);
          out.copyFrom(a.buf);
          return this._ct(out, ct.keyId, ct.noiseBudget, 1, { packed: a.packed });
        }
        const e = this._st(ek, 'EvaluationKey');
        if (ct.keyId !== ek.keyId) throw new FHEError('Evaluation key does not match ciphertext key', FHEErrorCode.KEY_MISMATCH);
        const out = this._buf(2 * this._n);
        await this._ctx.relinearizePreparedAsync(a.buf, e.prep, e.baseLog, out);
        return this._ct(out, ct.keyId, ct.noiseBudget - 1, 1, { packed: a.packed });
      });
    }
    async multiplyRelin(ct1, ct2, ek) { return this.relinearize(await this.multiply(ct1, ct2), ek); }
    /** square (:1004-1050) in its own kernel (fhe_ct_square_batch: 2 forward
     *  + 3 inverse transforms); words, budget and checks of multiply(ct, ct) */
    async square(ct) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct);
        if (a.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
        const out = this._buf(3 * this._n);
        await this._ctx.ctSquareAsync(a.buf, null, out, ct.isNtt ? 1 : 0);
        const red = Math.log2(this._n) + 5;
        return this._ct(out, ct.keyId, ct.noiseBudget - red, 2, { packed: a.packed });
      });
    }
    /** relinearize(square(ct - ref)) in one call (fhe_ct_square_relin_batch);
     *  ref: the state of a second ciphertext, or null */
    async _squareRelin(ct, a, ref, ek, budget, packed) {
      const e = this._st(ek, 'EvaluationKey');
      if (ct.keyId !== ek.keyId) throw new FHEError('Evaluation key does not match ciphertext key', FHEErrorCode.KEY_MISMATCH);
      const out = this._buf(2 * this._n);
      await this._ctx.ctSquareRelinPreparedAsync(a.buf, ref ? ref.buf : null, e.prep, e.baseLog, out);
      return this._ct(out, ct.keyId, budget, 1, { packed });
    }
    /** square_relin (:1052-1055): checks and budget of relinearize(square(ct)) */
    async squareRelin(ct, ek) {
      this._check();
      if (ct && ct.isNtt) return this.relinearize(await this.square(ct), ek);  // relinearisation is coefficient form
      return guard(async () => {
        const a = this._rlwe(ct);
        if (a.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
        const red = Math.log2(this._n) + 5;
        return this._squareRelin(ct, a, null, ek, ct.noiseBudget - red - 1, a.packed);
      });
    }
    /** compute_anomaly_score (:1305-1321): relinearize(square(subtract(ballot,
     *  expected))) with the subtraction done while the kernel loads; checks in
     *  that chain's order, its words and its budget (subtract's - 1, square's
     *  - (log2 n + 5), relinearize's - 1) */
    async computeAnomalyScore(ballot, expected, ek) {
      this._check();
      if (ballot && ballot.isNtt) {
        const d = await this.subtract(ballot, expected);
        return this.relinearize(await this.multiply(d, d), ek);
      }
      return guard(async () => {
        const a = this._rlwe(ballot), b = this._rlwe(expected);
        this._sameKey(ballot, expected, 'subtract');
        if (ballot.isNtt !== expected.isNtt) throw new FHEError('Cannot combine ciphertexts in different representations (NTT vs coefficient)', FHEErrorCode.INVALID_PARAMETERS);
        if (a.comps !== b.comps) throw new FHEError('ciphertext degrees differ', FHEErrorCode.INVALID_PARAMETERS);
        if (a.comps !== 2) throw new FHEError('multiply takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
        const red = Math.log2(this._n) + 5;
        const budget = Math.min(ballot.noiseBudget, expected.noiseBudget) - 1 - red - 1;
        return this._squareRelin(ballot, a, b, ek, budget, a.packed || b.packed);
      });
    }
    /** multiply_plain (:809-848): each component times encode(pt); budget - 2.
     *  A degree-1 ciphertext takes the fused plain dot with one pair (one
     *  upload of encode(pt), three forward transforms); the words are those
     *  of the polymul path, which degree-2 inputs keep. */
    async multiplyPlain(ct, pt) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct), n = this._n;
        const enc = this._encoded(pt);
        if (a.comps === 2) {
          const out = this._buf(2 * n);
          await this._ctx.dotPlainAsync([a.buf], [this._upload(enc)], out, false);
          return this._ct(out, ct.keyId, ct.noiseBudget - 2, ct.degree, { packed: a.packed });
        }
        const rep = this._buf(a.comps * n);
        for (let c = 0; c < a.comps; c++) rep.upload(enc, c * n);
        const out = this._buf(a.comps * n);
        await this._ctx.polymulAsync(a.buf, rep, out);
        return this._ct(out, ct.keyId, ct.noiseBudget - 2, ct.degree, { packed: a.packed });
      });
    }
    /** multiply_scalar (:890-903): budget - 1 */
    async multiplyScalar(ct, scalar) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct);
        const out = this._buf(a.comps * this._n);
        await this._ctx.mulScalarAsync(a.buf, u64(scalar), out);
        return this._ct(out, ct.keyId, ct.noiseBudget - 1, ct.degree, { packed: a.packed });
      });
    }

    // ---- bootstrapping (bootstrap_engine.cpp:676-758)
    async _bootstrap(ct, bk, testPoly) {
      const b = this._st(bk, 'BootstrapKey');
      const c = this._st(ct, 'Ciphertext');
      if (ct.keyId !== bk.keyId) throw new FHEError('Bootstrap key does not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
      const n = this._n, dim = b.dim;
      let la, lb;
      if (c.kind === 'lwe') {
        la = c.buf.view(0, dim);
        lb = c.buf.view(dim, 1);
      } else {
        if (c.comps !== 2) throw new FHEError('bootstrap takes degree-1 ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
        // RLWE (c0, c1) is the GLWE (mask c1, body c0): sample_extract
        // (:594-624) of coefficient 0, then key_switch (:626-674) to the LWE key
        const glwe = this._buf(2 * n);
        glwe.copyFrom(c.buf, 0, n, n);
        glwe.copyFrom(c.buf, n, 0, n);
        const ea = this._buf(n), eb = this._buf(1);
        await this._ctx.sampleExtractAsync(1, glwe, ea, eb);
        la = this._buf(dim);
        lb = this._buf(1);
        await this._ctx.keySwitchAsync(b.ksBaseLog, b.ksLevel, b.kskA, b.kskB, ea, eb, la, lb);
      }
      const out = this._buf(dim + 1);
      await this._ctx.bootstrapPreparedAsync(la, lb, b.bskPrep, testPoly, b.kskA, b.kskB, b.baseLog, b.level,
        b.ksBaseLog, b.ksLevel, out.view(0, dim), out.view(dim, 1));
      return this._handle('Ciphertext', { keyId: ct.keyId, noiseBudget: this._params.noiseBudget, isNtt: false, degree: 1 },
        { buf: out, kind: 'lwe', comps: 0, dim, packed: false });
    }
    async bootstrap(ct, bk) {
      this._check();
      return guard(async () => this._bootstrap(ct, bk, this._st(bk, 'BootstrapKey').testPoly));
    }
    async programmableBootstrap(ct, bk, lut) {
      this._check();
      return guard(async () => {
        if (!Array.isArray(lut) || lut.length === 0) throw new FHEError('lut must be a non-empty bigint[]', FHEErrorCode.INVALID_PARAMETERS);
        return this._bootstrap(ct, bk, this._upload(this._lutPoly(lut)));
      });
    }

    // ---- encrypted comparisons (encryption.cpp:1112-1303, which stop at "the
    // difference, ready for PBS").  SIGN(D, off) = slot extraction with body
    // offset off, key switch to the LWE key, bootstrap with the constant test
    // polynomial h = delta / 2: +h for a phase in [0, q/2), -h otherwise.  Slot
    // values lie in [0, t/2).  The SIGN terms of one operation share one key
    // switch and one bootstrap call; lweSum adds them and the body offset.
    // Results are 'lwe' ciphertexts: ~delta when the predicate holds, ~0 else.
    _half() { return this._delta / 2n; }
    _enc(v) { return ((u64(v) * this._delta) & M64) % this._q; }
    _modq(v) { return ((v % this._q) + this._q) % this._q; }
    _slotOf(options) {
      const s = options && options.slot !== undefined ? Number(options.slot) : 0;
      if (!Number.isInteger(s) || s < 0 || s >= this._n) throw new FHEError('slot index out of range', FHEErrorCode.INVALID_PARAMETERS);
      return s;
    }
    /** terms: [{ ct, ref | null, negate, offsets: bigint[] per slot }] -> one 'lwe' Ciphertext per slot */
    async _signSum(bk, terms, slots, bodyOffset) {
      const b = this._st(bk, 'BootstrapKey');
      const n = this._n, dim = b.dim, S = slots.length, H = terms.length;
      const keyId = terms[0].ct.keyId;
      if (keyId !== bk.keyId) throw new FHEError('Bootstrap key does not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
      const slotWords = BigUint64Array.from(slots, (s) => BigInt(s));
      const ea = this._buf(H * S * n), eb = this._buf(H * S);
      for (let i = 0; i < H; i++) {
        const t = terms[i];
        const c = this._rlwe(t.ct);
        const r = t.ref ? this._rlwe(t.ref) : null;
        if (c.comps !== 2 || (r && r.comps !== 2)) throw new FHEError('comparisons take degree-1 ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
        if (r) this._sameKey(t.ct, t.ref, 'compare');
        await this._ctx.slotExtractAsync(c.buf.view(0, 2 * n), r ? r.buf.view(0, 2 * n) : null, t.negate ? 1 : 0, slotWords,
          BigUint64Array.from(t.offsets, (o) => this._modq(o)), ea.view(i * S * n, S * n), eb.view(i * S, S));
      }
      const la = this._buf(H * S * dim), lb = this._buf(H * S);
      await this._ctx.keySwitchAsync(b.ksBaseLog, b.ksLevel, b.kskA, b.kskB, ea, eb, la, lb);
      if (!this._signPoly) this._signPoly = this._upload(new BigUint64Array(n).fill(this._half()));
      const sa = this._buf(H * S * dim), sb = this._buf(H * S);
      await this._ctx.bootstrapPreparedAsync(la, lb, b.bskPrep, this._signPoly, b.kskA, b.kskB, b.baseLog, b.level,
        b.ksBaseLog, b.ksLevel, sa, sb);
      const oa = this._buf(S * dim), ob = this._buf(S);
      await this._ctx.lweSumAsync(sa, sb, H, this._modq(bodyOffset), oa, ob);
      for (const x of [ea, eb, la, lb, sa, sb]) x.free();
      const out = [];
      for (let s = 0; s < S; s++) {
        const o = this._buf(dim + 1);
        o.copyFrom(oa, 0, s * dim, dim);
        o.copyFrom(ob, dim, s, 1);
        out.push(this._lwe(o, keyId, dim));
      }
      oa.free();
      ob.free();
      return out;
    }
    _lwe(buf, keyId, dim) {
      return this._handle('Ciphertext', { keyId, noiseBudget: this._params.noiseBudget, isNtt: false, degree: 1 },
        { buf, kind: 'lwe', comps: 0, dim, packed: false });
    }
    /** [a > b] (compare_greater_than :1174): SIGN(a - b, h - delta) + h */
    async compareGreaterThan(a, b, bk, options) {
      this._check();
      return guard(async () => {
        const h = this._half();
        return (await this._signSum(bk, [{ ct: a, ref: b, negate: false, offsets: [h - this._delta] }], [this._slotOf(options)], h))[0];
      });
    }
    /** [a < b] (compare_less_than :1197-1204): compareGreaterThan(b, a), the difference negated in the extraction */
    async compareLessThan(a, b, bk, options) {
      this._check();
      return guard(async () => {
        const h = this._half();
        return (await this._signSum(bk, [{ ct: a, ref: b, negate: true, offsets: [h - this._delta] }], [this._slotOf(options)], h))[0];
      });
    }
    /** [a == b] (compare_equal :1206): SIGN(a - b, h) + SIGN(b - a, h) */
    async compareEqual(a, b, bk, options) {
      this._check();
      return guard(async () => {
        const h = this._half();
        return (await this._signSum(bk, [{ ct: a, ref: b, negate: false, offsets: [h] },
          { ct: a, ref: b, negate: true, offsets: [h] }], [this._slotOf(options)], 0n))[0];
      });
    }
    /** [tally >= threshold] (check_threshold :1112-1143): SIGN(tally, h - encode(threshold)) + h */
    async checkThreshold(tally, threshold, bk, options) {
      this._check();
      return guard(async () => {
        const h = this._half();
        return (await this._signSum(bk, [{ ct: tally, ref: null, negate: false, offsets: [h - this._enc(threshold)] }],
          [this._slotOf(options)], h))[0];
      });
    }
    /** check_threshold per candidate: thresholds[j] against slot j, one LWE per candidate from one extraction */
    async checkThresholds(tally, thresholds, bk) {
      this._check();
      return guard(async () => {
        if (!Array.isArray(thresholds) || thresholds.length === 0 || thresholds.length > this._n) {
          throw new FHEError('thresholds must be a non-empty bigint[] of at most polyDegree entries', FHEErrorCode.INVALID_PARAMETERS);
        }
        const h = this._half();
        return this._signSum(bk, [{ ct: tally, ref: null, negate: false, offsets: thresholds.map((v) => h - this._enc(v)) }],
          thresholds.map((_, j) => j), h);
      });
    }
    /** [min <= ct <= max] (check_range :1228): SIGN(ct, h - encode(min)) + SIGN(-ct, h + encode(max)) */
    async checkRange(ct, min, max, bk, options) {
      this._check();
      return guard(async () => {
        // an empty range would make both terms -h: the sum would leave the {0, delta} encoding
        if (BigInt(min) > BigInt(max)) throw new FHEError('checkRange needs min <= max', FHEErrorCode.INVALID_PARAMETERS);
        const h = this._half();
        return (await this._signSum(bk, [{ ct, ref: null, negate: false, offsets: [h - this._enc(min)] },
          { ct, ref: null, negate: true, offsets: [h + this._enc(max)] }], [this._slotOf(options)], 0n))[0];
      });
    }
    /** the number of `existing` ballots equal to `ct` (detect_duplicate :1293-1300: the equality tests added) */
    async detectDuplicate(ct, existing, bk, options) {
      this._check();
      return guard(async () => {
        if (!Array.isArray(existing)) throw new FHEError('existing must be a Ciphertext[]', FHEErrorCode.INVALID_PARAMETERS);
        const slot = this._slotOf(options), h = this._half();
        if (existing.length === 0) {
          const b = this._st(bk, 'BootstrapKey');
          this._rlwe(ct);
          return this._lwe(this._upload(new BigUint64Array(b.dim + 1)), ct.keyId, b.dim);
        }
        const terms = [];
        for (const e of existing) {
          terms.push({ ct, ref: e, negate: false, offsets: [h] }, { ct, ref: e, negate: true, offsets: [h] });
        }
        return (await this._signSum(bk, terms, [slot], 0n))[0];
      });
    }

    // ---- LWE-to-RLWE packing (fhe_lwe_pack_batch): the comparison bits back
    // as one BFV ciphertext, bit s at coefficient slots[s], so that the tally,
    // the weighted tally and the threshold decryption apply to them.
    /** The packing key of the bootstrap key's LWE key under sk (fhe_pack_key_generate):
     *  rows (i, l) encrypt lweSk[i] 2^((level-1-l) baseLog); level * baseLog must
     *  cover the modulus for the packed ciphertext to decrypt (the default does). */
    async generatePackKey(sk, bk, options) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        const b = this._st(bk, 'BootstrapKey');
        if (sk.keyId !== bk.keyId || !s.lweDev) throw new FHEError('Bootstrap key does not match the secret key', FHEErrorCode.KEY_MISMATCH);
        const o = options || {};
        const bl = o.decompBaseLog || 8;
        const bits = (this._q - 1n).toString(2).length;
        const lv = o.decompLevel || Math.ceil(bits / bl);
        if (bl < 1 || bl > 63 || lv < 1 || (lv - 1) * bl >= 64) throw new FHEError('invalid decomposition (baseLog, level)', FHEErrorCode.INVALID_PARAMETERS);
        const key = this._buf(b.dim * lv * 2 * this._n);
        await this._ctx.packKeyGenerateAsync(s.buf, s.lweDev, bl, lv, this._seed, this._streams(2), this._std, key);
        return this._handle('PackKey', { keyId: sk.keyId, decompBaseLog: bl, decompLevel: lv, lweDimension: b.dim },
          { buf: key, baseLog: bl, level: lv, dim: b.dim });
      });
    }
    /** bits: bootstrapped LWE ciphertexts (what the comparisons return); the result
     *  decrypts (packed) to bit s at slot slots[s]; repeated slots add their bits. */
    async packBits(bits, slots, packKey) {
      this._check();
      return guard(async () => {
        const p = this._st(packKey, 'PackKey');
        if (!Array.isArray(bits) || bits.length === 0 || !Array.isArray(slots) || slots.length !== bits.length) {
          throw new FHEError('bits must be a non-empty Ciphertext[] with one slot each', FHEErrorCode.INVALID_PARAMETERS);
        }
        const S = bits.length, dim = p.dim, n = this._n;
        for (const h of slots) {
          if (!Number.isInteger(h) || h < 0 || h >= n) throw new FHEError('slot index out of range', FHEErrorCode.INVALID_PARAMETERS);
        }
        const la = this._buf(S * dim), lb = this._buf(S);
        bits.forEach((ct, s) => {
          const c = this._st(ct, 'Ciphertext');
          if (c.kind !== 'lwe' || c.dim !== dim) throw new FHEError('packBits takes bootstrapped LWE ciphertexts of the key\'s dimension', FHEErrorCode.INVALID_PARAMETERS);
          if (ct.keyId !== packKey.keyId) throw new FHEError('Pack key does not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
          la.copyFrom(c.buf, s * dim, 0, dim);
          lb.copyFrom(c.buf, s, dim, 1);
        });
        const out = this._buf(2 * n);
        await this._ctx.lwePackAsync(p.baseLog, p.level, p.buf, la, lb, BigUint64Array.from(slots, (h) => BigInt(h)), 0, out);
        la.free();
        lb.free();
        return this._ct(out, packKey.keyId, Math.min(...bits.map((c) => c.noiseBudget)) - 1, 1, { packed: true });
      });
    }

    // ---- Galois automorphisms, re-keying and the slot-isolating trace
    // (fhe_switch_key_generate, fhe_ct_galois_batch, fhe_ct_trace_batch).
    _switchDecomp(options) {
      const o = options || {};
      const bl = o.decompBaseLog || 8;
      const lv = o.decompLevel || Math.ceil((this._q - 1n).toString(2).length / bl);
      if (bl < 1 || bl > 63 || lv < 1 || (lv - 1) * bl >= 64) throw new FHEError('invalid decomposition (baseLog, level)', FHEErrorCode.INVALID_PARAMETERS);
      return { bl, lv };
    }
    /** raw pairs (a_l, b_l) into `raw`, one key of 2 * lv streams */
    async _switchKeyInto(to, from, g, bl, lv, raw) {
      await this._ctx.switchKeyGenerateAsync(to.buf, from.buf, g, bl, lv, this._seed, this._streams(2 * lv), this._std, raw);
    }
    /** The key that hands ciphertexts of skFrom to skTo; options.galoisElement g (odd,
     *  below 2n; default 1) makes it the key of applyGalois(ct, g, key).  skFrom = skTo
     *  with g != 1 is a Galois key, g = 1 with two keys a re-keying key. */
    async generateSwitchKey(skTo, skFrom, options) {
      this._check();
      return guard(async () => {
        const to = this._st(skTo, 'SecretKey'), from = this._st(skFrom, 'SecretKey');
        const g = (options && options.galoisElement) || 1;
        if (!Number.isInteger(g) || g < 1 || g >= 2 * this._n || g % 2 === 0) throw new FHEError('Galois element must be odd and below 2n', FHEErrorCode.INVALID_PARAMETERS);
        const { bl, lv } = this._switchDecomp(options);
        const raw = this._buf(lv * 2 * this._n), prep = this._buf(lv * 2 * this._n);
        await this._switchKeyInto(to, from, g, bl, lv, raw);
        await this._ctx.prepareRelinKeyAsync(raw, prep);
        raw.free();
        return this._handle('SwitchKey', { keyId: skTo.keyId, fromKeyId: skFrom.keyId, galoisElement: g, decompBaseLog: bl, decompLevel: lv },
          { buf: prep, baseLog: bl, level: lv, g });
      });
    }
    /** The Galois keys g_i = n / 2^i + 1 of `steps` trace steps (default log2 n: the full trace) in one buffer */
    async generateGaloisKeys(sk, steps, options) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        const n = this._n, full = Math.log2(n);
        const st = steps === undefined || steps === null ? full : steps;
        if (!Number.isInteger(st) || st < 1 || st > full) throw new FHEError('steps must be between 1 and log2(polyDegree)', FHEErrorCode.INVALID_PARAMETERS);
        const { bl, lv } = this._switchDecomp(options);
        const per = lv * 2 * n;
        const raw = this._buf(st * per), prep = this._buf(st * per);
        for (let i = 0; i < st; i++) await this._switchKeyInto(s, s, n / 2 ** i + 1, bl, lv, raw.view(i * per, per));
        await this._ctx.prepareRelinKeyAsync(raw, prep);
        raw.free();
        return this._handle('GaloisKeys', { keyId: sk.keyId, steps: st, decompBaseLog: bl, decompLevel: lv },
          { buf: prep, baseLog: bl, level: lv, steps: st });
      });
    }
    async _applyKey(ct, key, g) {
      const a = this._rlwe(ct), k = this._st(key, 'SwitchKey');
      if (a.comps !== 2) throw new FHEError('key switching takes degree-1 ciphertexts (relinearize first)', FHEErrorCode.INVALID_PARAMETERS);
      if (ct.isNtt) throw new FHEError('key switching takes coefficient-form ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
      if (k.g !== g) throw new FHEError(`switch key is for Galois element ${k.g}, not ${g}`, FHEErrorCode.INVALID_PARAMETERS);
      if (ct.keyId !== key.fromKeyId) throw new FHEError('Switch key does not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
      const out = this._buf(2 * this._n);
      await this._ctx.ctGaloisAsync(k.baseLog, g, k.buf, a.buf, 0, out);
      return this._ct(out, key.keyId, ct.noiseBudget - 1, 1, { packed: a.packed });
    }
    /** The encryption of sigma_g(message), X -> X^g; needs mode 'negacyclic' to decrypt for g != 1 */
    async applyGalois(ct, g, key) {
      this._check();
      return guard(async () => this._applyKey(ct, key, g));
    }
    /** The same message under the key's target secret key, without decrypting */
    async reKey(ct, key) {
      this._check();
      return guard(async () => {
        if (this._st(key, 'SwitchKey').g !== 1) throw new FHEError('reKey needs a switch key with Galois element 1', FHEErrorCode.INVALID_PARAMETERS);
        return this._applyKey(ct, key, 1);
      });
    }
    /** Every slot of the packed message but `slot` becomes 0: rotate by X^-slot, the
     *  full trace, rotate back.  Needs the log2(n) keys of generateGaloisKeys(sk)
     *  and mode 'negacyclic'. */
    async isolateSlot(ct, slot, keys) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct), k = this._st(keys, 'GaloisKeys'), n = this._n;
        if (this._mode !== 1) throw new FHEError('isolateSlot needs mode negacyclic', FHEErrorCode.INVALID_PARAMETERS);
        if (a.comps !== 2 || ct.isNtt) throw new FHEError('isolateSlot takes degree-1 coefficient-form ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
        if (!Number.isInteger(slot) || slot < 0 || slot >= n) throw new FHEError('slot index out of range', FHEErrorCode.INVALID_PARAMETERS);
        if (k.steps !== Math.log2(n)) throw new FHEError('isolateSlot needs the log2(polyDegree) keys of the full trace', FHEErrorCode.INVALID_PARAMETERS);
        if (ct.keyId !== keys.keyId) throw new FHEError('Galois keys do not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
        // X^-slot = -X^(n - slot): the ring product with a monomial is the exact rotation
        const rotate = async (src, index, value) => {
          const mono = new BigUint64Array(2 * n);
          mono[index] = value;
          mono[n + index] = value;
          const rep = this._upload(mono), dst = this._buf(2 * n);
          await this._ctx.polymulAsync(src, rep, dst);
          rep.free();
          return dst;
        };
        const x = slot ? await rotate(a.buf, n - slot, this._q - 1n) : a.buf;
        const y = this._buf(2 * n);
        await this._ctx.ctTraceAsync(k.baseLog, k.steps, k.buf, x, y);
        const out = slot ? await rotate(y, slot, 1n) : y;
        if (slot) { x.free(); y.free(); }
        return this._ct(out, ct.keyId, ct.noiseBudget - k.steps - 1, 1, { packed: true });
      });
    }

    // ---- SIMD batching (fhe_simd_encode_batch, fhe_simd_decode_batch,
    // fhe_ct_galois_chain_batch): n values mod t in the slots of one plaintext
    // (t = 1 mod 2n), products slot by slot, slot rotations and slot sums.
    // These are SIMD slots; isolateSlot / packBits address coefficients.
    // Mode 'negacyclic', coefficient form, one device.
    /** 3^(2^i) mod 2n for i < log2(n/2), then 2n - 1: row rotations by 2^i, then the row swap */
    _slotSumElements() {
      const n = this._n, gs = [];
      let g = 3;
      for (let i = 0; i < Math.log2(n / 2); i++) { gs.push(g); g = (g * g) % (2 * n); }
      gs.push(2 * n - 1);
      return gs;
    }
    _simdWords(values) {
      if (!Array.isArray(values) || values.length > this._n) throw new FHEError('expected at most polyDegree slot values', FHEErrorCode.INVALID_PARAMETERS);
      const w = new BigUint64Array(this._n);
      values.forEach((v, i) => { w[i] = u64(v); });
      return w;
    }
    /** Slot values (fewer than n are zero-padded) -> the packed plaintext whose encryption
     *  multiplies, rotates and sums slot by slot; options.lift gives the centred form mod q */
    async encodeSimd(values, options) {
      this._check();
      return guard(async () => {
        const src = this._upload(this._simdWords(values)), out = this._buf(this._n);
        await this._ctx.simdEncodeAsync(this._tEff, src, options && options.lift ? 1 : 0, out);
        const words = out.download();
        src.free();
        out.free();
        return this.createPackedPlaintext(Array.from(words));
      });
    }
    /** The slot values of a packed plaintext (decryptPacked's values, or a DecryptionResult's plaintext) */
    async decodeSimd(plaintext) {
      this._check();
      return guard(async () => {
        const vals = Array.isArray(plaintext) ? plaintext : (plaintext && plaintext.values);
        const src = this._upload(this._simdWords(vals)), out = this._buf(this._n);
        await this._ctx.simdDecodeAsync(this._tEff, src, out);
        const words = out.download();
        src.free();
        out.free();
        return Array.from(words);
      });
    }
    /** The Galois keys of rotateRows / rotateColumns / sumSlots in one buffer: log2(n) keys */
    async generateRotationKeys(sk, options) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        const n = this._n, gs = this._slotSumElements();
        const { bl, lv } = this._switchDecomp(options);
        const per = lv * 2 * n;
        const raw = this._buf(gs.length * per), prep = this._buf(gs.length * per);
        for (let i = 0; i < gs.length; i++) await this._switchKeyInto(s, s, gs[i], bl, lv, raw.view(i * per, per));
        await this._ctx.prepareRelinKeyAsync(raw, prep);
        raw.free();
        return this._handle('RotationKeys', { keyId: sk.keyId, steps: gs.length, decompBaseLog: bl, decompLevel: lv },
          { buf: prep, baseLog: bl, level: lv, gs });
      });
    }
    async _galoisChain(ct, keys, idx, addInput) {
      const a = this._rlwe(ct), k = this._st(keys, 'RotationKeys'), n = this._n;
      if (this._mode !== 1) throw new FHEError('slot rotations need mode negacyclic', FHEErrorCode.INVALID_PARAMETERS);
      if (a.comps !== 2 || ct.isNtt) throw new FHEError('slot rotations take degree-1 coefficient-form ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
      if (ct.keyId !== keys.keyId) throw new FHEError('Rotation keys do not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
      if (k.forSteps) throw new FHEError('these keys hold explicit steps: use rotateMany / linearTransform', FHEErrorCode.INVALID_PARAMETERS);
      const out = this._buf(2 * n);
      if (idx.length === 0) {
        await this._ctx.polyGaloisAsync(a.buf, 1, out);
        return this._ct(out, ct.keyId, ct.noiseBudget, 1, { packed: true });
      }
      await this._ctx.ctGaloisChainAsync(k.baseLog, k.level, BigUint64Array.from(idx, (i) => BigInt(k.gs[i])),
        BigUint64Array.from(idx, (i) => BigInt(i)), k.buf, a.buf, addInput ? 1 : 0, out);
      return this._ct(out, ct.keyId, ct.noiseBudget - idx.length * (addInput ? 2 : 1), 1, { packed: true });
    }
    /** Both slot rows rotated left by `steps` (negative: right): one chain call over the
     *  power-of-two keys of the binary digits of steps mod n/2 */
    async rotateRows(ct, steps, keys) {
      this._check();
      return guard(async () => {
        if (!Number.isInteger(steps)) throw new FHEError('steps must be an integer', FHEErrorCode.INVALID_PARAMETERS);
        const half = this._n / 2, m = ((steps % half) + half) % half, idx = [];
        for (let i = 0; i < Math.log2(half); i++) if ((m >> i) & 1) idx.push(i);
        return this._galoisChain(ct, keys, idx, false);
      });
    }
    /** The two slot rows swapped */
    async rotateColumns(ct, keys) {
      this._check();
      return guard(async () => this._galoisChain(ct, keys, [Math.log2(this._n) - 1], false));
    }
    /** The sum of all slots in every slot (options.rowsOnly: each row's sum in its slots).
     *  Every step doubles the noise: after a multiplication use a small t (include/fhe_gpu.h). */
    async sumSlots(ct, keys, options) {
      this._check();
      return guard(async () => {
        const steps = Math.log2(this._n) - (options && options.rowsOnly ? 1 : 0);
        return this._galoisChain(ct, keys, Array.from({ length: steps }, (_, i) => i), true);
      });
    }
    /** <v, w> mod t in every slot: multiplyScaled, relinearize, sumSlots */
    async innerProductScaled(ct1, ct2, ek, keys) {
      const prod = await this.relinearize(await this.multiplyScaled(ct1, ct2), ek);
      return this.sumSlots(prod, keys);
    }

    // ---- hoisted rotations and the plaintext linear transform (fhe_ct_hoist_batch,
    // fhe_ct_hoisted_galois_batch, fhe_ct_hoisted_linear_batch): a ciphertext is decomposed and
    // transformed once, every rotation of it is then a gathered key product on the spectra.
    /** 3^(steps mod n/2) mod 2n: the Galois element of a row rotation by `steps` */
    _rotationElement(steps) {
      if (!Number.isInteger(steps)) throw new FHEError('steps must be integers', FHEErrorCode.INVALID_PARAMETERS);
      const half = this._n / 2, two = BigInt(2 * this._n);
      let m = ((steps % half) + half) % half, g = 1n, b = 3n;
      for (; m; m = Math.floor(m / 2)) { if (m & 1) g = (g * b) % two; b = (b * b) % two; }
      return Number(g);
    }
    /** One Galois key per requested row-rotation step (generateRotationKeys holds the
     *  power-of-two steps only): the keys of rotateMany / linearTransform */
    async generateRotationKeysFor(sk, steps, options) {
      this._check();
      return guard(async () => {
        const s = this._st(sk, 'SecretKey');
        if (!Array.isArray(steps) || steps.length === 0) throw new FHEError('expected a list of steps', FHEErrorCode.INVALID_PARAMETERS);
        const n = this._n, gs = steps.map((st) => this._rotationElement(st));
        const { bl, lv } = this._switchDecomp(options);
        const per = lv * 2 * n;
        const raw = this._buf(gs.length * per), prep = this._buf(gs.length * per);
        for (let i = 0; i < gs.length; i++) await this._switchKeyInto(s, s, gs[i], bl, lv, raw.view(i * per, per));
        await this._ctx.prepareRelinKeyAsync(raw, prep);
        raw.free();
        return this._handle('RotationKeys', { keyId: sk.keyId, steps: gs.length, decompBaseLog: bl, decompLevel: lv },
          { buf: prep, baseLog: bl, level: lv, gs, forSteps: true });
      });
    }
    _stepKeys(steps, k) {
      const gs = steps.map((st) => this._rotationElement(st));
      const idx = gs.map((g) => k.gs.indexOf(g));
      if (idx.some((i) => i < 0)) throw new FHEError('no key for a requested rotation step (generateRotationKeysFor)', FHEErrorCode.INVALID_PARAMETERS);
      return { gs: BigUint64Array.from(gs, (g) => BigInt(g)), idx: BigUint64Array.from(idx, (i) => BigInt(i)) };
    }
    async _hoisted(x, k, keys) {
      if (x && x.__brand === 'HoistedCiphertext') {
        const h = this._st(x, 'HoistedCiphertext');
        if (h.baseLog !== k.baseLog || h.level !== k.level) throw new FHEError('the hoisted ciphertext and the keys differ in their decomposition', FHEErrorCode.INVALID_PARAMETERS);
        if (x.keyId !== keys.keyId) throw new FHEError('Rotation keys do not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
        return h;
      }
      return this._st(await this.hoist(x, keys), 'HoistedCiphertext');
    }
    /** Decompose and transform a degree-1 ciphertext once for any number of rotations with `keys` */
    async hoist(ct, keys) {
      this._check();
      return guard(async () => {
        const a = this._rlwe(ct), k = this._st(keys, 'RotationKeys'), n = this._n;
        if (this._mode !== 1) throw new FHEError('slot rotations need mode negacyclic', FHEErrorCode.INVALID_PARAMETERS);
        if (a.comps !== 2 || ct.isNtt) throw new FHEError('slot rotations take degree-1 coefficient-form ciphertexts', FHEErrorCode.INVALID_PARAMETERS);
        if (ct.keyId !== keys.keyId) throw new FHEError('Rotation keys do not match the ciphertext key', FHEErrorCode.KEY_MISMATCH);
        const buf = this._buf((1 + k.level) * n);
        await this._ctx.ctHoistAsync(k.baseLog, k.level, a.buf, buf);
        return this._handle('HoistedCiphertext', { keyId: ct.keyId, noiseBudget: ct.noiseBudget, decompBaseLog: k.baseLog, decompLevel: k.level },
          { buf, ct: a.buf, baseLog: k.baseLog, level: k.level });
      });
    }
    /** Every row rotation in `steps` of one ciphertext (or hoisted ciphertext) in one call */
    async rotateMany(ct, steps, keys) {
      this._check();
      return guard(async () => {
        const k = this._st(keys, 'RotationKeys'), n = this._n;
        if (!Array.isArray(steps) || steps.length === 0) throw new FHEError('expected a list of steps', FHEErrorCode.INVALID_PARAMETERS);
        const h = await this._hoisted(ct, k, keys), t = this._stepKeys(steps, k);
        const all = this._buf(steps.length * 2 * n);
        await this._ctx.ctHoistedGaloisAsync(k.level, t.gs, t.idx, k.buf, h.buf, all);
        const out = steps.map((_, i) => this._ct(this._buf(2 * n).copyFrom(all, 0, i * 2 * n, 2 * n), ct.keyId, ct.noiseBudget - 1, 1, { packed: true }));
        all.free();
        return out;
      });
    }
    /** sum over the entries [step, slot values] of `diagonals` of values (*) rotate(ct, step):
     *  one hoisted call, level + 1 forward and two inverse transforms for the whole sum.  Step 0
     *  (mod n/2) needs no key: it enters as a plaintext product. */
    async linearTransform(ct, diagonals, keys) {
      this._check();
      return guard(async () => {
        const k = this._st(keys, 'RotationKeys'), n = this._n, half = n / 2;
        const entries = diagonals instanceof Map ? Array.from(diagonals.entries()) : diagonals;
        if (!Array.isArray(entries) || entries.length === 0) throw new FHEError('expected [step, values] entries', FHEErrorCode.INVALID_PARAMETERS);
        const h = await this._hoisted(ct, k, keys);
        const out = this._buf(2 * n), steps = [], rows = [];
        let acc = 0;
        for (const [st, values] of entries) {
          const src = this._upload(this._simdWords(values)), enc = this._buf(n);
          await this._ctx.simdEncodeAsync(this._tEff, src, 1, enc);
          src.free();
          if (((st % half) + half) % half === 0) {
            if (acc) throw new FHEError('step 0 given twice', FHEErrorCode.INVALID_PARAMETERS);
            const rep = this._buf(2 * n).copyFrom(enc, 0, 0, n).copyFrom(enc, n, 0, n);
            await this._ctx.polymulAsync(h.ct, rep, out);
            rep.free();
            enc.free();
            acc = 1;
          } else {
            steps.push(st);
            rows.push(enc);
          }
        }
        if (rows.length) {
          const t = this._stepKeys(steps, k), pts = this._buf(rows.length * n);
          rows.forEach((r, i) => { pts.copyFrom(r, i * n, 0, n); r.free(); });
          await this._ctx.forwardAsync(pts, pts);
          await this._ctx.ctHoistedLinearAsync(k.level, t.gs, t.idx, k.buf, pts, h.buf, acc, out);
          pts.free();
        }
        const budget = (ct.noiseBudget === undefined ? 0 : ct.noiseBudget) - 3;
        return this._ct(out, ct.keyId, budget, 1, { packed: true });
      });
    }

    // ---- serialisation: binary = header words + the native words, checksum = SHA-256
    _serialize(kind, h, words, meta, opts) {
      const fmt = (opts && opts.format) || 'binary';
      const head = [BigInt(SERIAL_MAGIC), 1n, BigInt(KINDS.indexOf(kind)), BigInt(this._n), this._q, BigInt(h.keyId)];
      const metaJson = Buffer.from(JSON.stringify(meta, (k, v) => (typeof v === 'bigint' ? v.toString() : v)));
      const hw = BigUint64Array.from(head);
      let data = Buffer.concat([Buffer.from(hw.buffer), Buffer.from(new Uint32Array([metaJson.length]).buffer), metaJson,
        Buffer.from(words.buffer, words.byteOffset, words.byteLength)]);
      if (fmt === 'json') {
        data = Buffer.from(JSON.stringify({ head: head.map(String), meta: metaJson.toString(),
          words: Buffer.from(words.buffer, words.byteOffset, words.byteLength).toString('base64') }));
      } else if (fmt === 'compressed') {
        data = zlib.deflateSync(data);
      } else if (fmt !== 'binary') {
        throw new FHEError(`unknown format ${fmt}`, FHEErrorCode.SERIALIZATION_ERROR);
      }
      return { data: new Uint8Array(data), format: fmt, checksum: new Uint8Array(crypto.createHash('sha256').update(data).digest()) };
    }
    _parse(s, kind) {
      if (!s || !s.data) throw new FHEError('no serialized data', FHEErrorCode.SERIALIZATION_ERROR);
      const data = Buffer.from(s.data);
      const sum = crypto.createHash('sha256').update(data).digest();
      if (s.checksum && !sum.equals(Buffer.from(s.checksum))) throw new FHEError('checksum mismatch', FHEErrorCode.SERIALIZATION_ERROR);
      try {
        let head, meta, words;
        if (s.format === 'json') {
          const j = JSON.parse(data.toString());
          head = j.head.map(BigInt);
          meta = JSON.parse(j.meta);
          const w = Buffer.from(j.words, 'base64');
          words = new BigUint64Array(w.buffer.slice(w.byteOffset, w.byteOffset + w.length));
        } else {
          const raw = s.format === 'compressed' ? zlib.inflateSync(data) : data;
          const b = Buffer.from(raw);
          const hw = new BigUint64Array(b.buffer.slice(b.byteOffset, b.byteOffset + 48));
          head = Array.from(hw);
          const ml = b.readUInt32LE(48);
          meta = JSON.parse(b.slice(52, 52 + ml).toString());
          const wb = b.slice(52 + ml);
          words = new BigUint64Array(wb.buffer.slice(wb.byteOffset, wb.byteOffset + wb.length));
        }
        if (head[0] !== BigInt(SERIAL_MAGIC) || head[1] !== 1n || KINDS[Number(head[2])] !== kind) throw new Error('header');
        if (head[3] !== BigInt(this._n) || head[4] !== this._q) throw new Error('parameters differ from this engine');
        return { keyId: head[5], meta, words };
      } catch (e) {
        throw new FHEError(`malformed ${kind} data: ${e.message}`, FHEErrorCode.SERIALIZATION_ERROR);
      }
    }
    async serializeSecretKey(sk, opts) {
      this._check();
      const s = this._st(sk, 'SecretKey');
      const r = this._serialize('secret', sk, s.buf.download(), { lweSk: s.lweSk ? Array.from(s.lweSk, String) : null }, opts);
      return Object.assign(r, { keyType: 'secret', version: 1 });
    }
    async deserializeSecretKey(data) {
      this._check();
      return guard(async () => {
        const { keyId, meta, words } = this._parse(data, 'secret');
        const buf = this._upload(words), prep = this._buf(2 * this._n);
        await this._ctx.prepareSecretKeyAsync(buf, prep);
        const st = { buf, prep };
        if (meta.lweSk) {
          st.lweSk = BigInt64Array.from(meta.lweSk.map(BigInt));
          st.lweDev = this._upload(st.lweSk);
        }
        return this._handle('SecretKey', { keyId }, st);
      });
    }
    async serializePublicKey(pk, opts) {
      this._check();
      const s = this._st(pk, 'PublicKey');
      return Object.assign(this._serialize('public', pk, s.buf.download(), {}, opts), { keyType: 'public', version: 1 });
    }
    async deserializePublicKey(data) {
      this._check();
      return guard(async () => {
        const { keyId, words } = this._parse(data, 'public');
        const buf = this._upload(words), prep = this._buf(2 * this._n);
        await this._ctx.preparePublicKeyAsync(buf, prep);
        return this._handle('PublicKey', { keyId }, { buf, prep });
      });
    }
    async serializeCiphertext(ct, opts) {
      this._check();
      const c = this._st(ct, 'Ciphertext');
      const meta = { noiseBudget: ct.noiseBudget, isNtt: ct.isNtt, degree: ct.degree, kind: c.kind, comps: c.comps,
        dim: c.dim || 0, packed: c.packed };
      const r = this._serialize('ciphertext', ct, c.buf.download(), meta, opts);
      return Object.assign(r, { keyId: ct.keyId, version: 1 });
    }
    async deserializeCiphertext(data) {
      this._check();
      return guard(async () => {
        const { keyId, meta, words } = this._parse(data, 'ciphertext');
        return this._handle('Ciphertext', { keyId, noiseBudget: meta.noiseBudget, isNtt: meta.isNtt, degree: meta.degree },
          { buf: this._upload(words), kind: meta.kind, comps: meta.comps, dim: meta.dim, packed: meta.packed });
      });
    }

    // ---- plaintexts and introspection
    createPlaintext(value) {
      this._check();
      return Object.freeze({ __brand: 'Plaintext', values: [BigInt(value)], plaintextModulus: this._tEff, isPacked: false });
    }
    createPackedPlaintext(values) {
      this._check();
      return Object.freeze({ __brand: 'Plaintext', values: values.map((v) => BigInt(v)), plaintextModulus: this._tEff, isPacked: true });
    }
    getParams() { this._check(); return this._params; }
    getHardwareCapabilities() {
      this._check();
      const hw = native.detectHardware();
      return { hasSme: false, hasMetal: false, hasNeon: false, hasAmx: false, hasNeuralEngine: false, metalGpuCores: 0,
        unifiedMemorySize: 0n, hasHip: hw.hasHip, gpuDevices: hw.gpuDevices, computeUnits: hw.computeUnits,
        hbmBytes: BigInt(hw.hbmBytes), arch: hw.arch, deviceName: hw.deviceName };
    }
    getSlotCount() { this._check(); return this._n; }
    /** the native context (NttContext) for batched array-level work */
    get context() { return this._ctx; }
    /** the DeviceBuffer behind a handle (advanced use: batched kernels) */
    /** the device buffer behind a handle; `part` names another native buffer of
     *  it (a bootstrap key's 'kskA' / 'kskB') */
    deviceBuffer(h, part) {
      const s = h && state.get(h);
      if (!s) return undefined;
      if (part === undefined) return s.buf;
      return s[part] instanceof DeviceBuffer ? s[part] : undefined;
    }
    dispose() {
      if (!this._disposed) {
        this._disposed = true;
        this._ctx = null;
      }
    }
  }

  async function createEngine(params, options) {
    const p = createParameterSet(params);
    try {
      return new FHEEngineImpl(p, options);
    } catch (e) {
      throw toFHEError(e);
    }
  }
  return { FHEEngineImpl, createEngine };
}

/**
 * Context defaults from the environment (SURVEY.md section 5 config flags):
 * FHE_NTT_MODE = compat | negacyclic when no mode is given; FHE_GPU_DEVICES
 * = comma-separated GPU ordinals when neither device nor devices is given
 * (one entry: that device; several: a multi-device context).
 */
function envDefaults({ mode, device, devices } = {}) {
  if (mode === undefined) mode = (process.env.FHE_NTT_MODE || 'compat').trim() || 'compat';
  if (device === undefined && devices === undefined && process.env.FHE_GPU_DEVICES) {
    const list = process.env.FHE_GPU_DEVICES.split(',').filter((x) => x.trim() !== '').map(Number);
    if (list.some((d) => !Number.isInteger(d) || d < 0)) {
      throw new RangeError(`FHE_GPU_DEVICES must be a comma-separated list of ordinals, got ${process.env.FHE_GPU_DEVICES}`);
    }
    if (list.length === 1) device = list[0];
    else if (list.length > 1) devices = list;
  }
  if (device === undefined) device = devices ? devices[0] : 0;
  return { mode, device, devices };
}

module.exports = {
  envDefaults, FHEError, FHEErrorCode, NTT_PRIMES, calculateDerivedParameters, createParameterSet, getAvailablePresets,
  makeEngineClass, toFHEError,
};
