// Type declarations of the MI355X backend's JS entry point (lib/index.js).
//
// createEngine() returns the reference's FHEEngine
// (/root/reference/src/api/fhe-engine.ts:33-78) over the types of
// src/api/types.ts:18-166, restated here so a TypeScript caller of the
// reference binds against this package unchanged; the native-level classes
// below (NttContext, DeviceBuffer, PolynomialEngine, GpuFHEEngine) are this
// backend's batched array surface (INTEGRATION.md).  `tsc` is not part of
// this image: tests/test_abi.py checks that every name declared here is
// exported by lib/index.js and every FHEEngine method exists on the engine.

// ---------------------------------------------------------------- handles
// Opaque, frozen handles of device-resident objects (types.ts:18-71).
export interface SecretKey {
  readonly __brand: 'SecretKey';
  readonly handle: bigint;
  readonly keyId: bigint;
}
export interface PublicKey {
  readonly __brand: 'PublicKey';
  readonly handle: bigint;
  readonly keyId: bigint;
}
export interface EvaluationKey {
  readonly __brand: 'EvaluationKey';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly decompBaseLog: number;
  readonly decompLevel: number;
}
export interface BootstrapKey {
  readonly __brand: 'BootstrapKey';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly lweDimension: number;
}
/** The packing key-switch key of generatePackKey (the bootstrap key's LWE key under the ring key). */
export interface PackKey {
  readonly __brand: 'PackKey';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly decompBaseLog: number;
  readonly decompLevel: number;
  readonly lweDimension: number;
}
export interface Ciphertext {
  readonly __brand: 'Ciphertext';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly noiseBudget: number;
  readonly isNtt: boolean;
  readonly degree: number;
}
export interface Plaintext {
  readonly __brand: 'Plaintext';
  readonly values: bigint[];
  readonly plaintextModulus: bigint;
  readonly isPacked: boolean;
}

// ---------------------------------------------------------------- parameters (types.ts:77-135)
export type SecurityLevel = 128 | 192 | 256;
export type FHEScheme = 'TFHE' | 'BFV' | 'CKKS';
export type ParameterPreset =
  | 'tfhe-128-fast' | 'tfhe-128-balanced' | 'tfhe-256-secure'
  | 'bfv-128-simd' | 'ckks-128-ml' | 'tfhe-128-voting';
export interface CustomParameters {
  polyDegree: number;
  moduli: bigint[];
  lweDimension?: number;
  lweNoiseStd?: number;
  glweDimension?: number;
  decompBaseLog?: number;
  decompLevel?: number;
  securityLevel: SecurityLevel;
}
export interface ParameterSet {
  scheme: FHEScheme;
  security: SecurityLevel;
  polyDegree: number;
  moduli: bigint[];
  lweDimension: number;
  lweNoiseStd: number;
  glweDimension: number;
  decompBaseLog: number;
  decompLevel: number;
  plaintextModulus: bigint;
  noiseBudget: number;
  maxMultDepth: number;
}

// ---------------------------------------------------------------- errors (types.ts:140-166)
export enum FHEErrorCode {
  NOISE_BUDGET_EXHAUSTED = 'NOISE_BUDGET_EXHAUSTED',
  INVALID_PARAMETERS = 'INVALID_PARAMETERS',
  KEY_MISMATCH = 'KEY_MISMATCH',
  HARDWARE_UNAVAILABLE = 'HARDWARE_UNAVAILABLE',
  SERIALIZATION_ERROR = 'SERIALIZATION_ERROR',
  PROOF_VERIFICATION_FAILED = 'PROOF_VERIFICATION_FAILED',
  THRESHOLD_NOT_MET = 'THRESHOLD_NOT_MET',
  INVALID_BALLOT = 'INVALID_BALLOT',
  DUPLICATE_VOTE = 'DUPLICATE_VOTE',
  NATIVE_ERROR = 'NATIVE_ERROR',
}
export class FHEError extends Error {
  constructor(message: string, code: FHEErrorCode, details?: Record<string, unknown>);
  readonly code: FHEErrorCode;
  readonly details?: Record<string, unknown>;
}

// ---------------------------------------------------------------- hardware (types.ts:171-190)
// The reference's Apple fields, reported false / 0 here, plus the HIP device.
export interface HardwareCapabilities {
  hasSme: boolean;
  hasMetal: boolean;
  hasNeon: boolean;
  hasAmx: boolean;
  hasNeuralEngine: boolean;
  metalGpuCores: number;
  unifiedMemorySize: bigint;
  hasHip?: boolean;
  gpuDevices?: number;
  computeUnits?: number;
  arch?: string;
  name?: string;
}

// ---------------------------------------------------------------- keys, encryption, progress
export type SecretKeyDistribution = 'TERNARY' | 'GAUSSIAN' | 'BINARY' | 'UNIFORM';
export interface KeyGenerationOptions {
  distribution?: SecretKeyDistribution;
  decompBaseLog?: number;
  decompLevel?: number;
}
export interface ThresholdConfig { threshold: number; totalShares: number; }
export interface SecretKeyShare {
  readonly shareId: number;
  readonly handle: bigint;
  readonly commitment: Uint8Array;
  readonly keyId: bigint;
}
export interface ThresholdKeys {
  shares: SecretKeyShare[];
  publicKey: PublicKey;
  threshold: number;
  totalShares: number;
}
export interface PartialDecryption { shareId: number; partialResult: bigint[]; proof?: Uint8Array; }
export interface EncryptionResult { ciphertext: Ciphertext; proof?: Uint8Array; }
export interface DecryptionResult {
  plaintext: Plaintext;
  remainingNoiseBudget: number;
  success: boolean;
  errorMessage?: string;
}
export interface BatchEncryptionOptions { generateProofs?: boolean; useGpu?: boolean; batchSize?: number; }
export interface BatchEncryptionResult {
  ciphertexts: Ciphertext[];
  proofs?: Uint8Array[];
  elapsedMs: number;
  throughputPerSecond: number;
}
export interface ProgressInfo {
  stage: string;
  current: number;
  total: number;
  elapsedMs: number;
  estimatedRemainingMs?: number;
  progressPercent: number;
}
export type ProgressCallback = (progress: ProgressInfo) => void;
export type SerializationFormat = 'binary' | 'json' | 'compressed';
export interface SerializationOptions { format?: SerializationFormat; includeMetadata?: boolean; compress?: boolean; }
export interface SerializedKey {
  data: Uint8Array;
  format: SerializationFormat;
  keyType: 'secret' | 'public' | 'evaluation' | 'bootstrap';
  version: number;
  checksum: Uint8Array;
}
export interface SerializedCiphertext {
  data: Uint8Array;
  format: SerializationFormat;
  keyId: bigint;
  version: number;
  checksum: Uint8Array;
}

// ---------------------------------------------------------------- FHEEngine (fhe-engine.ts:33-78)
export interface FHEEngine {
  generateSecretKey(options?: KeyGenerationOptions): Promise<SecretKey>;
  generatePublicKey(sk: SecretKey): Promise<PublicKey>;
  generateEvalKey(sk: SecretKey, options?: KeyGenerationOptions): Promise<EvaluationKey>;
  generateBootstrapKey(sk: SecretKey): Promise<BootstrapKey>;
  generateThresholdKeys(config: ThresholdConfig): Promise<ThresholdKeys>;
  encrypt(plaintext: Plaintext, pk: PublicKey): Promise<EncryptionResult>;
  encryptValue(value: bigint, pk: PublicKey): Promise<Ciphertext>;
  encryptPacked(values: bigint[], pk: PublicKey): Promise<Ciphertext>;
  decrypt(ciphertext: Ciphertext, sk: SecretKey): Promise<DecryptionResult>;
  decryptValue(ciphertext: Ciphertext, sk: SecretKey): Promise<bigint>;
  decryptPacked(ct: Ciphertext, sk: SecretKey, numValues: number): Promise<bigint[]>;
  batchEncrypt(pts: Plaintext[], pk: PublicKey, opts?: BatchEncryptionOptions): Promise<BatchEncryptionResult>;
  add(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  addPlain(ct: Ciphertext, pt: Plaintext): Promise<Ciphertext>;
  addScalar(ct: Ciphertext, value: bigint): Promise<Ciphertext>;
  subtract(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  negate(ct: Ciphertext): Promise<Ciphertext>;
  batchAdd(cts: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  multiply(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  multiplyRelin(ct1: Ciphertext, ct2: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  multiplyPlain(ct: Ciphertext, pt: Plaintext): Promise<Ciphertext>;
  multiplyScalar(ct: Ciphertext, scalar: bigint): Promise<Ciphertext>;
  relinearize(ct: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  square(ct: Ciphertext): Promise<Ciphertext>;
  squareRelin(ct: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  bootstrap(ct: Ciphertext, bk: BootstrapKey): Promise<Ciphertext>;
  programmableBootstrap(ct: Ciphertext, bk: BootstrapKey, lut: bigint[]): Promise<Ciphertext>;
  partialDecrypt(ct: Ciphertext, share: ThresholdKeys['shares'][0]): Promise<PartialDecryption>;
  combinePartialDecryptions(ct: Ciphertext, partials: PartialDecryption[], t: number): Promise<DecryptionResult>;
  getNoiseBudget(ct: Ciphertext, sk: SecretKey): Promise<number>;
  estimateNoiseBudget(ct: Ciphertext): number;
  serializeSecretKey(sk: SecretKey, opts?: SerializationOptions): Promise<SerializedKey>;
  deserializeSecretKey(data: SerializedKey): Promise<SecretKey>;
  serializePublicKey(pk: PublicKey, opts?: SerializationOptions): Promise<SerializedKey>;
  deserializePublicKey(data: SerializedKey): Promise<PublicKey>;
  serializeCiphertext(ct: Ciphertext, opts?: SerializationOptions): Promise<SerializedCiphertext>;
  deserializeCiphertext(data: SerializedCiphertext): Promise<Ciphertext>;
  createPlaintext(value: bigint): Plaintext;
  createPackedPlaintext(values: bigint[]): Plaintext;
  getZeroCiphertext(pk: PublicKey): Promise<Ciphertext>;
  getParams(): ParameterSet;
  getHardwareCapabilities(): HardwareCapabilities;
  getSlotCount(): number;
  dispose(): void;
}

/** Ballot aggregation (EncryptionEngine::tally_votes, tally_multi_candidate,
 * update_tally, tally_weighted_votes; encryption.cpp:1061-1168): every sum is
 * one device launch over all ballots. */
export interface FHETallyEngine extends FHEEngine {
  tallyVotes(ballots: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  tallyMultiCandidate(ballots: Ciphertext[], numCandidates: number, progress?: ProgressCallback): Promise<Ciphertext>;
  updateTally(tally: Ciphertext, ballot: Ciphertext): Promise<Ciphertext>;
  tallyWeightedVotes(ballots: Ciphertext[], weights: Ciphertext[], ek: EvaluationKey,
    progress?: ProgressCallback): Promise<Ciphertext>;
}

/** tallyWeightedVotes' fifth argument.  'each' (default): multiply and
 * relinearise per ballot, the reference's words.  'once': the fused degree-2
 * sum (dotProduct) and one relinearisation: the same plaintext with less
 * noise, not the same words (the digit decomposition is not linear). */
export interface TallyWeightedOptions {
  relinearize?: 'each' | 'once';
  /** dotProductScaled and one relinearisation (FHEScaledEngine): opens to sum w_i b_i with real keys */
  scaled?: boolean;
}

/** Ciphertext inner product: sum_i multiply(cts1[i], cts2[i]) as one degree-2
 * ciphertext in one fused launch (fhe_ct_dot_ptrs), word-identical to the
 * chain of multiply() and add(). */
export interface FHEDotEngine extends FHETallyEngine {
  dotProduct(cts1: Ciphertext[], cts2: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
}

/** Tallies under public weights, one launch each and no relinearisation key.
 * tallyScalarWeightedVotes: sum_i multiplyScalar(ballots[i], weights[i])
 * (fhe_ct_sum_scaled_ptrs).  dotPlain: sum_i multiplyPlain(cts[i], pts[i]) over
 * degree-1 ciphertexts (fhe_ct_dot_plain_ptrs).  Both are word-identical to
 * the chain of multiplyScalar() / multiplyPlain() and add(). */
export interface FHEPublicWeightEngine extends FHEDotEngine {
  tallyScalarWeightedVotes(ballots: Ciphertext[], weights: bigint[], progress?: ProgressCallback): Promise<Ciphertext>;
  dotPlain(cts: Ciphertext[], pts: Plaintext[], progress?: ProgressCallback): Promise<Ciphertext>;
}

/** Fraud scoring (EncryptionEngine::compute_anomaly_score, encryption.cpp:
 * 1305-1321): relinearize(square(subtract(ballot, expected))) in one call
 * (fhe_ct_square_relin_batch; the subtraction happens while the squaring kernel
 * loads), word-identical to that chain, with its key checks and noise budget. */
export interface FHEAnomalyEngine extends FHEPublicWeightEngine {
  computeAnomalyScore(ballot: Ciphertext, expected: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
}

/** Batched threshold decryption: a trustee's partial decryptions of many tallies
 * in one launch (fhe_partial_decrypt_batch, the share's transform prepared once),
 * and their combination, decoding and noise measurement in one launch
 * (fhe_combine_partials_batch).  partials[i] is trustee i's list, index-aligned
 * with cts; the results equal partialDecrypt / combinePartialDecryptions per
 * ciphertext, with remainingNoiseBudget taken from the measured noise. */
export interface FHEThresholdEngine extends FHEAnomalyEngine {
  partialDecryptBatch(cts: Ciphertext[], share: ThresholdKeys['shares'][0]): Promise<PartialDecryption[]>;
  combinePartialDecryptionsBatch(cts: Ciphertext[], partials: PartialDecryption[][], t: number): Promise<DecryptionResult[]>;
}

/** The coefficient (packed slot) a comparison reads; default 0. */
export interface CompareOptions {
  slot?: number;
}

/** Encrypted comparisons (the fraud-detection surface of encryption.cpp:1112-1303,
 * which stops at "the difference, ready for PBS"): the LWE ciphertext at the slot
 * of the difference (fhe_slot_extract_batch), a key switch, the sign bootstrap
 * (constant test polynomial delta / 2) and the sum of the sign terms
 * (fhe_lwe_sum_batch).  Slot values lie in [0, t / 2).  Each result is a
 * bootstrapped LWE ciphertext (as bootstrap() returns) that decrypts to 1 when the
 * predicate holds and 0 otherwise; detectDuplicate to the number of matches;
 * checkThresholds to one ciphertext per candidate slot j against thresholds[j]. */
export interface FHECompareEngine extends FHEThresholdEngine {
  compareGreaterThan(a: Ciphertext, b: Ciphertext, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  compareLessThan(a: Ciphertext, b: Ciphertext, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  compareEqual(a: Ciphertext, b: Ciphertext, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  checkThreshold(tally: Ciphertext, threshold: bigint, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  checkThresholds(tally: Ciphertext, thresholds: bigint[], bk: BootstrapKey): Promise<Ciphertext[]>;
  checkRange(ct: Ciphertext, min: bigint, max: bigint, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  detectDuplicate(ct: Ciphertext, existing: Ciphertext[], bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
}

/** Decomposition of a pack key; the default (base 2^8, enough levels to cover the modulus) decrypts. */
export interface PackKeyOptions {
  decompBaseLog?: number;
  decompLevel?: number;
}

/** LWE-to-RLWE packing (fhe_lwe_pack_batch): the encrypted bits of the comparisons, which are LWE
 * ciphertexts under the bootstrap key's LWE key, come back as ONE BFV ciphertext with bit s at
 * coefficient slots[s] (repeated slots add), so that the tallies, the weighted tallies and the
 * threshold decryption apply to them.  Slots other than 0 need mode 'negacyclic' to decrypt. */
export interface FHEPackEngine extends FHECompareEngine {
  generatePackKey(sk: SecretKey, bk: BootstrapKey, options?: PackKeyOptions): Promise<PackKey>;
  packBits(bits: Ciphertext[], slots: number[], packKey: PackKey): Promise<Ciphertext>;
}

/** A key-switching key of generateSwitchKey: hands sigma_g of a ciphertext of `fromKeyId` to `keyId`. */
export interface SwitchKey {
  readonly __brand: 'SwitchKey';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly fromKeyId: bigint;
  readonly galoisElement: number;
  readonly decompBaseLog: number;
  readonly decompLevel: number;
}
/** The Galois keys g_i = n / 2^i + 1 of `steps` trace steps (generateGaloisKeys). */
export interface GaloisKeys {
  readonly __brand: 'GaloisKeys';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly steps: number;
  readonly decompBaseLog: number;
  readonly decompLevel: number;
}
/** Decomposition and Galois element of a switch key; the default (g = 1, base 2^8, enough levels
 * to cover the modulus) re-keys and decrypts. */
export interface SwitchKeyOptions {
  galoisElement?: number;
  decompBaseLog?: number;
  decompLevel?: number;
}

/** Key switching of degree-1 ciphertexts (fhe_ct_galois_batch, fhe_ct_trace_batch): re-keying
 * without decrypting, the automorphisms X -> X^g, and the trace that opens one slot of a packed
 * ciphertext and nothing else.  g != 1 and isolateSlot need mode 'negacyclic' to decrypt. */
export interface FHEGaloisEngine extends FHEPackEngine {
  generateSwitchKey(skTo: SecretKey, skFrom: SecretKey, options?: SwitchKeyOptions): Promise<SwitchKey>;
  generateGaloisKeys(sk: SecretKey, steps?: number, options?: PackKeyOptions): Promise<GaloisKeys>;
  applyGalois(ct: Ciphertext, g: number, key: SwitchKey): Promise<Ciphertext>;
  reKey(ct: Ciphertext, key: SwitchKey): Promise<Ciphertext>;
  isolateSlot(ct: Ciphertext, slot: number, keys: GaloisKeys): Promise<Ciphertext>;
}

/** Scale-invariant BFV products (fhe_ct_multiply_scaled_batch, fhe_ct_dot_scaled_batch,
 * fhe_ct_square_scaled_batch): round(t/q (ct1 (x) ct2)) over the integers.  The degree-2 result
 * carries Delta m (multiply()'s carries Delta^2 m) and opens with real keys after relinearize();
 * its phase is c0 - c1 s + c2 s^2, so decrypt() of the degree-2 result itself does not open it.
 * dotProductScaled rescales once after the sum: not the words of a sum of multiplyScaled().
 * Mode 'negacyclic', coefficient form, single device. */
export interface FHEScaledEngine extends FHEGaloisEngine {
  multiplyScaled(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  dotProductScaled(cts1: Ciphertext[], cts2: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  squareScaled(ct: Ciphertext): Promise<Ciphertext>;
  tallyWeightedVotes(ballots: Ciphertext[], weights: Ciphertext[], ek: EvaluationKey,
    progress?: ProgressCallback, options?: TallyWeightedOptions): Promise<Ciphertext>;
}

/** The Galois keys of the slot rotations (generateRotationKeys): log2(n) keys, for the row
 * rotations by 2^i and the row swap. */
export interface RotationKeys {
  readonly __brand: 'RotationKeys';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly steps: number;
  readonly decompBaseLog: number;
  readonly decompLevel: number;
}

/** SIMD batching (fhe_simd_encode_batch, fhe_simd_decode_batch, fhe_ct_galois_chain_batch): with
 * plaintextModulus = 1 mod 2 polyDegree a plaintext holds polyDegree slot values in 2 rows;
 * products of encodings act slot by slot, rotateRows / rotateColumns move the slots and sumSlots
 * leaves their sum in every slot.  These are SIMD slots: isolateSlot and packBits address
 * coefficients.  Mode 'negacyclic', coefficient form, single device. */
export interface FHESimdEngine extends FHEScaledEngine {
  generateRotationKeys(sk: SecretKey, options?: PackKeyOptions): Promise<RotationKeys>;
  encodeSimd(values: bigint[], options?: { lift?: boolean }): Promise<Plaintext>;
  decodeSimd(plaintext: Plaintext | bigint[]): Promise<bigint[]>;
  rotateRows(ct: Ciphertext, steps: number, keys: RotationKeys): Promise<Ciphertext>;
  rotateColumns(ct: Ciphertext, keys: RotationKeys): Promise<Ciphertext>;
  sumSlots(ct: Ciphertext, keys: RotationKeys, options?: { rowsOnly?: boolean }): Promise<Ciphertext>;
  innerProductScaled(ct1: Ciphertext, ct2: Ciphertext, ek: EvaluationKey, keys: RotationKeys): Promise<Ciphertext>;
}

/** A ciphertext decomposed and transformed once (FHEHoistEngine.hoist) for any number of rotations */
export interface HoistedCiphertext {
  readonly __brand: 'HoistedCiphertext';
  readonly handle: bigint;
  readonly keyId: bigint;
  readonly noiseBudget: number;
  readonly decompBaseLog: number;
  readonly decompLevel: number;
}

/** Hoisted rotations and the plaintext linear transform (fhe_ct_hoist_batch,
 * fhe_ct_hoisted_galois_batch, fhe_ct_hoisted_linear_batch): many rotations of one ciphertext
 * share one decomposition and level + 1 forward transforms; linearTransform sums
 * values (*) rotate(ct, step) over its entries with two inverse transforms in all. */
export interface FHEHoistEngine extends FHESimdEngine {
  generateRotationKeysFor(sk: SecretKey, steps: number[], options?: PackKeyOptions): Promise<RotationKeys>;
  hoist(ct: Ciphertext, keys: RotationKeys): Promise<HoistedCiphertext>;
  rotateMany(ct: Ciphertext | HoistedCiphertext, steps: number[], keys: RotationKeys): Promise<Ciphertext[]>;
  linearTransform(ct: Ciphertext | HoistedCiphertext, diagonals: Map<number, bigint[]> | Array<[number, bigint[]]>, keys: RotationKeys): Promise<Ciphertext>;
}

/** Options of this backend (environment defaults FHE_NTT_MODE, FHE_GPU_DEVICES). */
export interface EngineOptions {
  mode?: 'compat' | 'negacyclic';
  device?: number;
  devices?: number[];
}

export declare class FHEEngineImpl implements FHETallyEngine {
  constructor(params: ParameterSet, options?: EngineOptions);
  generateSecretKey(options?: KeyGenerationOptions): Promise<SecretKey>;
  generatePublicKey(sk: SecretKey): Promise<PublicKey>;
  generateEvalKey(sk: SecretKey, options?: KeyGenerationOptions): Promise<EvaluationKey>;
  generateBootstrapKey(sk: SecretKey): Promise<BootstrapKey>;
  generateThresholdKeys(config: ThresholdConfig): Promise<ThresholdKeys>;
  encrypt(plaintext: Plaintext, pk: PublicKey): Promise<EncryptionResult>;
  encryptValue(value: bigint, pk: PublicKey): Promise<Ciphertext>;
  encryptPacked(values: bigint[], pk: PublicKey): Promise<Ciphertext>;
  decrypt(ciphertext: Ciphertext, sk: SecretKey): Promise<DecryptionResult>;
  decryptValue(ciphertext: Ciphertext, sk: SecretKey): Promise<bigint>;
  decryptPacked(ct: Ciphertext, sk: SecretKey, numValues: number): Promise<bigint[]>;
  batchEncrypt(pts: Plaintext[], pk: PublicKey, opts?: BatchEncryptionOptions): Promise<BatchEncryptionResult>;
  add(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  addPlain(ct: Ciphertext, pt: Plaintext): Promise<Ciphertext>;
  addScalar(ct: Ciphertext, value: bigint): Promise<Ciphertext>;
  subtract(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  negate(ct: Ciphertext): Promise<Ciphertext>;
  batchAdd(cts: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  multiply(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  multiplyRelin(ct1: Ciphertext, ct2: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  multiplyPlain(ct: Ciphertext, pt: Plaintext): Promise<Ciphertext>;
  multiplyScalar(ct: Ciphertext, scalar: bigint): Promise<Ciphertext>;
  relinearize(ct: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  square(ct: Ciphertext): Promise<Ciphertext>;
  squareRelin(ct: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  bootstrap(ct: Ciphertext, bk: BootstrapKey): Promise<Ciphertext>;
  programmableBootstrap(ct: Ciphertext, bk: BootstrapKey, lut: bigint[]): Promise<Ciphertext>;
  partialDecrypt(ct: Ciphertext, share: ThresholdKeys['shares'][0]): Promise<PartialDecryption>;
  combinePartialDecryptions(ct: Ciphertext, partials: PartialDecryption[], t: number): Promise<DecryptionResult>;
  getNoiseBudget(ct: Ciphertext, sk: SecretKey): Promise<number>;
  estimateNoiseBudget(ct: Ciphertext): number;
  serializeSecretKey(sk: SecretKey, opts?: SerializationOptions): Promise<SerializedKey>;
  deserializeSecretKey(data: SerializedKey): Promise<SecretKey>;
  serializePublicKey(pk: PublicKey, opts?: SerializationOptions): Promise<SerializedKey>;
  deserializePublicKey(data: SerializedKey): Promise<PublicKey>;
  serializeCiphertext(ct: Ciphertext, opts?: SerializationOptions): Promise<SerializedCiphertext>;
  deserializeCiphertext(data: SerializedCiphertext): Promise<Ciphertext>;
  createPlaintext(value: bigint): Plaintext;
  createPackedPlaintext(values: bigint[]): Plaintext;
  getZeroCiphertext(pk: PublicKey): Promise<Ciphertext>;
  getParams(): ParameterSet;
  getHardwareCapabilities(): HardwareCapabilities;
  getSlotCount(): number;
  dispose(): void;
  tallyVotes(ballots: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  tallyMultiCandidate(ballots: Ciphertext[], numCandidates: number, progress?: ProgressCallback): Promise<Ciphertext>;
  updateTally(tally: Ciphertext, ballot: Ciphertext): Promise<Ciphertext>;
  tallyWeightedVotes(ballots: Ciphertext[], weights: Ciphertext[], ek: EvaluationKey,
    progress?: ProgressCallback, options?: TallyWeightedOptions): Promise<Ciphertext>;
  dotProduct(cts1: Ciphertext[], cts2: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  tallyScalarWeightedVotes(ballots: Ciphertext[], weights: bigint[], progress?: ProgressCallback): Promise<Ciphertext>;
  dotPlain(cts: Ciphertext[], pts: Plaintext[], progress?: ProgressCallback): Promise<Ciphertext>;
  computeAnomalyScore(ballot: Ciphertext, expected: Ciphertext, ek: EvaluationKey): Promise<Ciphertext>;
  partialDecryptBatch(cts: Ciphertext[], share: ThresholdKeys['shares'][0]): Promise<PartialDecryption[]>;
  combinePartialDecryptionsBatch(cts: Ciphertext[], partials: PartialDecryption[][], t: number): Promise<DecryptionResult[]>;
  compareGreaterThan(a: Ciphertext, b: Ciphertext, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  compareLessThan(a: Ciphertext, b: Ciphertext, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  compareEqual(a: Ciphertext, b: Ciphertext, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  checkThreshold(tally: Ciphertext, threshold: bigint, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  checkThresholds(tally: Ciphertext, thresholds: bigint[], bk: BootstrapKey): Promise<Ciphertext[]>;
  checkRange(ct: Ciphertext, min: bigint, max: bigint, bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  detectDuplicate(ct: Ciphertext, existing: Ciphertext[], bk: BootstrapKey, options?: CompareOptions): Promise<Ciphertext>;
  generatePackKey(sk: SecretKey, bk: BootstrapKey, options?: PackKeyOptions): Promise<PackKey>;
  packBits(bits: Ciphertext[], slots: number[], packKey: PackKey): Promise<Ciphertext>;
  generateSwitchKey(skTo: SecretKey, skFrom: SecretKey, options?: SwitchKeyOptions): Promise<SwitchKey>;
  generateGaloisKeys(sk: SecretKey, steps?: number, options?: PackKeyOptions): Promise<GaloisKeys>;
  applyGalois(ct: Ciphertext, g: number, key: SwitchKey): Promise<Ciphertext>;
  reKey(ct: Ciphertext, key: SwitchKey): Promise<Ciphertext>;
  isolateSlot(ct: Ciphertext, slot: number, keys: GaloisKeys): Promise<Ciphertext>;
  multiplyScaled(ct1: Ciphertext, ct2: Ciphertext): Promise<Ciphertext>;
  dotProductScaled(cts1: Ciphertext[], cts2: Ciphertext[], progress?: ProgressCallback): Promise<Ciphertext>;
  squareScaled(ct: Ciphertext): Promise<Ciphertext>;
  generateRotationKeys(sk: SecretKey, options?: PackKeyOptions): Promise<RotationKeys>;
  encodeSimd(values: bigint[], options?: { lift?: boolean }): Promise<Plaintext>;
  decodeSimd(plaintext: Plaintext | bigint[]): Promise<bigint[]>;
  rotateRows(ct: Ciphertext, steps: number, keys: RotationKeys): Promise<Ciphertext>;
  rotateColumns(ct: Ciphertext, keys: RotationKeys): Promise<Ciphertext>;
  sumSlots(ct: Ciphertext, keys: RotationKeys, options?: { rowsOnly?: boolean }): Promise<Ciphertext>;
  innerProductScaled(ct1: Ciphertext, ct2: Ciphertext, ek: EvaluationKey, keys: RotationKeys): Promise<Ciphertext>;
  generateRotationKeysFor(sk: SecretKey, steps: number[], options?: PackKeyOptions): Promise<RotationKeys>;
  hoist(ct: Ciphertext, keys: RotationKeys): Promise<HoistedCiphertext>;
  rotateMany(ct: Ciphertext | HoistedCiphertext, steps: number[], keys: RotationKeys): Promise<Ciphertext[]>;
  linearTransform(ct: Ciphertext | HoistedCiphertext, diagonals: Map<number, bigint[]> | Array<[number, bigint[]]>, keys: RotationKeys): Promise<Ciphertext>;
  /** The device buffer behind a handle (this backend's extension); part names another
   * native buffer of the handle (a bootstrap key's 'kskA' / 'kskB'). */
  deviceBuffer(handle: unknown, part?: string): DeviceBuffer | undefined;
}

/** createEngine (src/index.ts:108): a preset name or custom parameters. */
export function createEngine(params: ParameterPreset | CustomParameters, options?: EngineOptions): Promise<FHEEngine>;
export const createFHEEngine: typeof createEngine;
export function createParameterSet(preset: ParameterPreset): ParameterSet;
export function getAvailablePresets(): ParameterPreset[];
export function calculateDerivedParameters(params: ParameterSet): { noiseBudget: number; maxMultDepth: number };
export const NTT_PRIMES: Record<string, bigint>;

// ---------------------------------------------------------------- native surface
// The reference napi-rs exports (index.d.ts:14-44 of the reference).
export function initialize(): void;
export function detectHardware(): HardwareCapabilities;
export function version(): string;
export declare class ModularArithmetic {
  constructor(modulus: number);
  montgomeryMul(a: number, b: number): number;
  modAdd(a: number, b: number): number;
  modSub(a: number, b: number): number;
  toMontgomery(a: number): number;
  fromMontgomery(a: number): number;
  getModulus(): number;
}

/** u64 coefficient buffers: host arrays (staged through HBM per call) or
 * DeviceBuffers of the same context (device-resident). */
export type Words = BigUint64Array | DeviceBuffer;

export interface NttContextInfo {
  degree: number;
  modulus: bigint;
  primitiveRoot: bigint;
  mode: number;
  devices: number;
  [key: string]: unknown;
}

/** One libfhe_gpu context (fhe_ctx_create / fhe_ctx_create_multi).  Every
 * compute method X has a promise form XAsync (napi_async_work). */
export declare class NttContext {
  constructor(degree: number, modulus: bigint | number, mode?: number, device?: number | number[]);
  info(): NttContextInfo;
  synchronize(): void;
  /** Ciphertexts of two-CU blind rotations recomputed by the one-CU repair pass
   * (a partner workgroup was not co-resident; results are exact either way). */
  brRepairCount(): number;
  forward(a: Words, out?: Words): Words;
  inverse(a: Words, out?: Words): Words;
  polymul(a: Words, b: Words, out: Words): Words;
  pointwise(a: Words, b: Words, out: Words): Words;
  forwardMul(a: Words, w: Words, out: Words): Words;
  add(a: Words, b: Words, out: Words): Words;
  sub(a: Words, b: Words, out: Words): Words;
  negate(a: Words, out: Words): Words;
  mulScalar(a: Words, s: bigint, out: Words): Words;
  /** out = the sum of the ciphertexts in `buffers` (1..3 polynomials each, out.words
   * words; an entry may repeat; out is none of them): one launch (fhe_ct_sum_ptrs). */
  sum(buffers: DeviceBuffer[], out: DeviceBuffer): DeviceBuffer;
  sumAsync(buffers: DeviceBuffer[], out: DeviceBuffer): Promise<DeviceBuffer>;
  /** out (3 n words) = sum_i multiply(buffersA[i], buffersB[i]) over ciphertexts of 2 n
   * words; entries may repeat, buffersA[i] may be buffersB[i]; out is none of them: one
   * fused launch (fhe_ct_dot_ptrs). */
  dot(buffersA: DeviceBuffer[], buffersB: DeviceBuffer[], out: DeviceBuffer, isNtt?: boolean): DeviceBuffer;
  dotAsync(buffersA: DeviceBuffer[], buffersB: DeviceBuffer[], out: DeviceBuffer, isNtt?: boolean): Promise<DeviceBuffer>;
  /** out = sum_i buffers[i] * scalars[i] (entries as sum(); scalars a host array of
   * buffers.length words, copied by the call): one launch (fhe_ct_sum_scaled_ptrs). */
  sumScaled(buffers: DeviceBuffer[], scalars: BigUint64Array, out: DeviceBuffer): DeviceBuffer;
  sumScaledAsync(buffers: DeviceBuffer[], scalars: BigUint64Array, out: DeviceBuffer): Promise<DeviceBuffer>;
  /** out (2 n words) = sum_i multiplyPlain(ctBuffers[i], ptBuffers[i]) over ciphertexts of
   * 2 n words and encoded plaintext polynomials of n words; entries may repeat; out is none
   * of them: one fused launch (fhe_ct_dot_plain_ptrs).  isNtt: the ciphertexts and out are
   * NTT-domain, the plaintexts still coefficient form. */
  dotPlain(ctBuffers: DeviceBuffer[], ptBuffers: DeviceBuffer[], out: DeviceBuffer, isNtt?: boolean): DeviceBuffer;
  dotPlainAsync(ctBuffers: DeviceBuffer[], ptBuffers: DeviceBuffer[], out: DeviceBuffer, isNtt?: boolean): Promise<DeviceBuffer>;
  ctMultiply(ct1: Words, ct2: Words, out: Words, isNtt?: number): Words;
  /** out [batch][3][n] = square(ct - ref) of ct [batch][2][n] (fhe_ct_square_batch); ref: null,
   * one ciphertext [2][n] for the whole batch, or one per ciphertext; out overlaps neither. */
  ctSquare(ct: Words, ref: Words | null, out: Words, isNtt?: number): Words;
  ctSquareAsync(ct: Words, ref: Words | null, out: Words, isNtt?: number): Promise<Words>;
  /** out [batch][2][n] = relinearize(ctSquare(ct, ref)) with a key from prepareRelinKey
   * (fhe_ct_square_relin_batch); coefficient form. */
  ctSquareRelinPrepared(ct: Words, ref: Words | null, rlkPrep: Words, baseLog: number, out: Words): Words;
  ctSquareRelinPreparedAsync(ct: Words, ref: Words | null, rlkPrep: Words, baseLog: number, out: Words): Promise<Words>;
  /** shares [total][n] of generate_threshold_keys at the points 1..total from coeffs
   * [threshold][n] (fhe_shamir_shares_batch). */
  shamirShares(coeffs: Words, total: number, out: Words): Words;
  shamirSharesAsync(coeffs: Words, total: number, out: Words): Promise<Words>;
  /** shares [count][n] -> their NTT-domain form for partialDecryptPrepared (fhe_key_share_prepare). */
  prepareKeyShares(shares: Words, out: Words): Words;
  prepareKeySharesAsync(shares: Words, out: Words): Promise<Words>;
  /** out [nshares][batch][n] = c1 * share for ct [batch][2][n] (fhe_partial_decrypt_batch). */
  partialDecryptPrepared(sharesPrep: Words, ct: Words, out: Words): Words;
  partialDecryptPreparedAsync(sharesPrep: Words, ct: Words, out: Words): Promise<Words>;
  /** phase = c0 - sum_i partials[i] lambdas[i] of ct [batch][2][n], partials [count][batch][n],
   * decoded into values [batch][n] with maxNoise [batch] (fhe_combine_partials_batch);
   * lambdas is always a host array. */
  combinePartials(t: bigint, ct: Words, partials: Words, lambdas: BigUint64Array, values: Words, maxNoise: Words,
    phase?: Words): Words;
  combinePartialsAsync(t: bigint, ct: Words, partials: Words, lambdas: BigUint64Array, values: Words, maxNoise: Words,
    phase?: Words): Promise<Words>;
  /** lweA [batch][S][n], lweB [batch][S] = the LWE ciphertexts at the coefficients `slots` of
   * ct - ref (negate: ref - ct; ref as ctSquare), bodies plus offsets[s] (fhe_slot_extract_batch);
   * slots and offsets are always host arrays. */
  slotExtract(ct: Words, ref: Words | null, negate: number, slots: BigUint64Array, offsets: BigUint64Array | null,
    lweA: Words, lweB: Words): Words;
  slotExtractAsync(ct: Words, ref: Words | null, negate: number, slots: BigUint64Array, offsets: BigUint64Array | null,
    lweA: Words, lweB: Words): Promise<Words>;
  /** outA [batch][dim], outB [batch] = the sum over lweA [terms][batch][dim], lweB [terms][batch]
   * plus bodyOffset on the body, modulo the ring modulus (fhe_lwe_sum_batch). */
  lweSum(lweA: Words, lweB: Words, terms: number, bodyOffset: bigint, outA: Words, outB: Words): Words;
  lweSumAsync(lweA: Words, lweB: Words, terms: number, bodyOffset: bigint, outA: Words, outB: Words): Promise<Words>;
  /** out [batch][2][n] (+= with accumulate) = the packing key switch of lweA [batch][S][dim], lweB [batch][S]
   * under packKey [dim*level][2][n], LWE s at coefficient slots[s] (fhe_lwe_pack_batch); slots is a host array. */
  lwePack(baseLog: number, level: number, packKey: Words, lweA: Words, lweB: Words, slots: BigUint64Array,
    accumulate: number, out: Words): Words;
  lwePackAsync(baseLog: number, level: number, packKey: Words, lweA: Words, lweB: Words, slots: BigUint64Array,
    accumulate: number, out: Words): Promise<Words>;
  /** out [dim*level][2][n] = the pack key of lweSk (BigInt64Array or device words) under sk (fhe_pack_key_generate). */
  packKeyGenerate(sk: Words, lweSk: BigInt64Array | Words, baseLog: number, level: number, seed: BigUint64Array,
    stream: bigint | number, noiseStd: number, out: Words): Words;
  packKeyGenerateAsync(sk: Words, lweSk: BigInt64Array | Words, baseLog: number, level: number, seed: BigUint64Array,
    stream: bigint | number, noiseStd: number, out: Words): Promise<Words>;
  /** out [batch][n] = sigma_g(a), the automorphism X -> X^g (odd g < 2n) as a signed permutation (fhe_poly_galois_batch). */
  polyGalois(a: Words, g: number, out: Words): Words;
  polyGaloisAsync(a: Words, g: number, out: Words): Promise<Words>;
  /** out [level][2][n] = the key that switches sigma_g(ct) from sigma_g(skFrom) to skTo (fhe_switch_key_generate);
   * prepared with prepareRelinKey. */
  switchKeyGenerate(skTo: Words, skFrom: Words, g: number, baseLog: number, level: number, seed: BigUint64Array,
    stream: bigint | number, noiseStd: number, out: Words): Words;
  switchKeyGenerateAsync(skTo: Words, skFrom: Words, g: number, baseLog: number, level: number, seed: BigUint64Array,
    stream: bigint | number, noiseStd: number, out: Words): Promise<Words>;
  /** out [batch][2][n] = the key switch of sigma_g(ct) (+ ct with addInput) under swkPrep [level][2][n]
   * (fhe_ct_galois_batch). */
  ctGalois(baseLog: number, g: number, swkPrep: Words, ct: Words, addInput: number, out: Words): Words;
  ctGaloisAsync(baseLog: number, g: number, swkPrep: Words, ct: Words, addInput: number, out: Words): Promise<Words>;
  /** out [batch][2][n] = `steps` steps of the field trace under keysPrep [steps][level][2][n], key i for
   * g_i = n / 2^i + 1 (fhe_ct_trace_batch). */
  ctTrace(baseLog: number, steps: number, keysPrep: Words, ct: Words, out: Words): Words;
  ctTraceAsync(baseLog: number, steps: number, keysPrep: Words, ct: Words, out: Words): Promise<Words>;
  /** fhe_simd_encode_batch / fhe_simd_decode_batch with the codec context of plaintext modulus t */
  simdEncode(t: bigint | number, values: Words, lift: number, out: Words): Words;
  simdEncodeAsync(t: bigint | number, values: Words, lift: number, out: Words): Promise<Words>;
  simdDecode(t: bigint | number, polys: Words, out: Words): Words;
  simdDecodeAsync(t: bigint | number, polys: Words, out: Words): Promise<Words>;
  /** fhe_ct_galois_chain_batch: x <- ctGalois(gs[i], key keyIdx[i] of keysPrep, x, addInput) for every i */
  ctGaloisChain(baseLog: number, level: number, gs: BigUint64Array, keyIdx: BigUint64Array, keysPrep: Words, ct: Words, addInput: number, out: Words): Words;
  ctGaloisChainAsync(baseLog: number, level: number, gs: BigUint64Array, keyIdx: BigUint64Array, keysPrep: Words, ct: Words, addInput: number, out: Words): Promise<Words>;
  /** fhe_ct_hoist_batch: ct [batch][2][n] -> out [batch][1 + level][n], the spectra of c0 and of the digits of c1 */
  ctHoist(baseLog: number, level: number, ct: Words, out: Words): Words;
  ctHoistAsync(baseLog: number, level: number, ct: Words, out: Words): Promise<Words>;
  /** fhe_ct_hoisted_galois_batch: out [batch][gs.length][2][n], rotation gs[r] with key keyIdx[r] of keysPrep */
  ctHoistedGalois(level: number, gs: BigUint64Array, keyIdx: BigUint64Array, keysPrep: Words, hoisted: Words, out: Words): Words;
  ctHoistedGaloisAsync(level: number, gs: BigUint64Array, keyIdx: BigUint64Array, keysPrep: Words, hoisted: Words, out: Words): Promise<Words>;
  /** fhe_ct_hoisted_linear_batch: out [batch][2][n] = sum_r ptsNtt[r] (*) rotation r (+ out when accumulate) */
  ctHoistedLinear(level: number, gs: BigUint64Array, keyIdx: BigUint64Array, keysPrep: Words, ptsNtt: Words, hoisted: Words, accumulate: number, out: Words): Words;
  ctHoistedLinearAsync(level: number, gs: BigUint64Array, keyIdx: BigUint64Array, keysPrep: Words, ptsNtt: Words, hoisted: Words, accumulate: number, out: Words): Promise<Words>;
  /** Scale-invariant products round(t/q (ct1 (x) ct2)) (t: plaintext modulus, 0 selects 4); the
   * context keeps one scale context per t.  ct [batch][2][n] -> out [batch][3][n] */
  ctMultiplyScaled(t: bigint | number, ct1: Words, ct2: Words, out: Words): Words;
  ctMultiplyScaledAsync(t: bigint | number, ct1: Words, ct2: Words, out: Words): Promise<Words>;
  /** a, b [groups][count][2][n] -> out [groups][3][n], one rescale per group */
  ctDotScaled(t: bigint | number, a: Words, b: Words, count: number, out: Words): Words;
  ctDotScaledAsync(t: bigint | number, a: Words, b: Words, count: number, out: Words): Promise<Words>;
  /** square(ct - ref), ref as ctSquare */
  ctSquareScaled(t: bigint | number, ct: Words, ref: Words | null, out: Words): Words;
  ctSquareScaledAsync(t: bigint | number, ct: Words, ref: Words | null, out: Words): Promise<Words>;
  relinearize(ct3: Words, rlk: Words, baseLog: number, out: Words): Words;
  externalProduct(glwe: Words, ggsw: Words, baseLog: number, level: number, out: Words): Words;
  blindRotate(acc: Words, lweA: Words, lweB: Words, bsk: Words, baseLog: number, level: number): Words;
  forwardAsync(a: Words, out?: Words): Promise<Words>;
  inverseAsync(a: Words, out?: Words): Promise<Words>;
  polymulAsync(a: Words, b: Words, out: Words): Promise<Words>;
  ctMultiplyAsync(ct1: Words, ct2: Words, out: Words, isNtt?: number): Promise<Words>;
  relinearizeAsync(ct3: Words, rlk: Words, baseLog: number, out: Words): Promise<Words>;
  [method: string]: unknown;
}

/** Device memory of one NttContext (refcounted; views share it). */
export declare class DeviceBuffer {
  constructor(ctx: NttContext, words: number);
  constructor(parent: DeviceBuffer, offsetWords: number, words: number);
  readonly words: number;
  readonly handle: bigint;
  upload(src: BigUint64Array | BigInt64Array, offsetWords?: number): this;
  download(dst?: BigUint64Array, offsetWords?: number, words?: number): BigUint64Array;
  copyFrom(src: DeviceBuffer, dstOffset?: number, srcOffset?: number, words?: number): this;
  view(offsetWords: number, words: number): DeviceBuffer;
  free(): void;
}

export function modmulBatch(q: bigint, a: BigUint64Array, b: BigUint64Array, out: BigUint64Array): BigUint64Array;
export function mlMontgomeryMulBatch(q: BigUint64Array, a: BigUint64Array, b: BigUint64Array,
                                     out: BigUint64Array): BigUint64Array;

/** Batched polynomial arithmetic over Z_q[X] (array level). */
export declare class PolynomialEngine {
  constructor(degree: number, modulus: bigint | number, opts?: EngineOptions);
  readonly degree: number;
  readonly modulus: bigint;
  alloc(batch?: number): BigUint64Array;
  toNtt(a: Words, out?: Words): Words;
  fromNtt(a: Words, out?: Words): Words;
  multiply(a: Words, b: Words, out?: Words): Words;
  pointwiseMultiply(a: Words, b: Words, out?: Words): Words;
  add(a: Words, b: Words, out?: Words): Words;
  subtract(a: Words, b: Words, out?: Words): Words;
  negate(a: Words, out?: Words): Words;
  multiplyScalar(a: Words, s: bigint | number, out?: Words): Words;
  forwardMultiply(a: Words, w: Words, out?: Words): Words;
  externalProduct(glwe: Words, ggsw: Words, baseLog: number, level: number, out?: Words): Words;
  ctMultiply(ct1: Words, ct2: Words, opts?: { isNtt?: boolean }, out?: Words): Words;
  ctSquare(ct: Words, ref?: Words | null, opts?: { isNtt?: boolean }, out?: Words): Words;
  partialDecrypt(ct: Words, shares: Words, out?: Words): Words;
  combinePartials(ct: Words, partials: Words, lambdas: ArrayLike<bigint>, t?: bigint):
    { values: BigUint64Array; maxNoise: BigUint64Array; phase: BigUint64Array };
  relinearize(ct3: Words, rlk: Words, baseLog?: number, out?: Words): Words;
  multiplyRelin(ct1: Words, ct2: Words, rlk: Words, baseLog?: number): Words;
  blindRotate(acc: Words, lweA: Words, lweB: Words, bsk: Words, baseLog: number, level: number): Words;
  brRepairCount(): number;
  info(): NttContextInfo;
}

/** The FHEEngine operations at array level (ciphertexts as BigUint64Array). */
export declare class GpuFHEEngine {
  constructor(params: ParameterPreset | Partial<ParameterSet> & { polyDegree: number; moduli: bigint[] },
              opts?: EngineOptions);
  readonly n: number;
  readonly q: bigint;
  readonly t: bigint;
  getSlotCount(): number;
  [method: string]: unknown;
}

export const PRESETS: Record<ParameterPreset, Partial<ParameterSet> & { polyDegree: number; moduli: bigint[] }>;
export const sampling: {
  uniformMod(q: bigint, count: number): BigUint64Array;
  ternary(q: bigint, count: number): BigUint64Array;
  gaussian(q: bigint, std: number, count: number): BigUint64Array;
};
