/*
 * fhe_gpu.h -- C ABI of the MI355X (gfx950) FHE polynomial-arithmetic
 * backend (libfhe_gpu.so).  Drop-in replacement for the compute path of
 * Digital-Defiance/node-fhe-accelerate: NTTProcessor, PolynomialRing,
 * ModularArithmetic / BarrettReducer / MultiLimbModularArithmetic and
 * BootstrapEngine::external_product, plus the N-API-visible
 * ModularArithmetic class and detectHardware().
 *
 * Conventions
 *   - Plain C: pointers + sizes, no C++ or torch types, no exceptions.
 *   - Every function returns FHE_OK (0) or a negative FHE_ERR_* code; the
 *     message (the reference's exception text where one exists) is
 *     available from fhe_last_error() (thread-local).
 *   - Polynomial data: contiguous row-major [batch][n] uint64 (the layout of
 *     the reference's Polynomial / Metal buffers, metal_compute.mm:400-410).
 *     Inputs may be any u64 and behave as x mod q (every reference path
 *     reduces); outputs are canonical residues in [0, q).
 *   - where = FHE_DEVICE: pointers are device (HBM) pointers of the context's
 *     device, work is enqueued on the context stream and NOT synchronised.
 *     where = FHE_HOST: pointers are host memory; the call stages through
 *     device scratch and returns after the result is back in host memory.
 *   - A context is immutable after creation (except its stream); concurrent
 *     calls on distinct buffers are safe, as with the reference's shared
 *     read-only NTTProcessor (encryption.cpp:520-533).
 */
#ifndef FHE_GPU_H
#define FHE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_GPU_ABI_VERSION 1

/* ---- status codes (messages mirror the reference's std::invalid_argument) */
#define FHE_OK 0
#define FHE_ERR_DEGREE_POW2 (-1)     /* "Polynomial degree must be a power of 2"      ntt_processor.cpp:142 */
#define FHE_ERR_DEGREE_RANGE (-2)    /* "Polynomial degree must be between 4 and 65536" ntt_processor.cpp:147 */
#define FHE_ERR_MODULUS_EVEN (-3)    /* "Modulus must be odd"                          ntt_processor.cpp:152 */
#define FHE_ERR_NOT_NTT_FRIENDLY (-4) /* "Modulus is not NTT-friendly: q != 1 (mod 2N)" ntt_processor.cpp:104 */
#define FHE_ERR_COUNT (-5)           /* "Coefficient count must equal polynomial degree" ntt_processor.cpp:264 */
#define FHE_ERR_NO_ROOT (-6)         /* "Could not find primitive root ..."            ntt_processor.cpp:127 */
#define FHE_ERR_MONT_MODULUS (-7)    /* "Modulus must be odd and non-zero for Montgomery arithmetic" modular_arithmetic.cpp:54 */
#define FHE_ERR_ZERO_MODULUS (-8)    /* "Modulus must be non-zero for Barrett reduction" modular_arithmetic.cpp:240 */
#define FHE_ERR_INVALID_ARG (-9)
#define FHE_ERR_UNSUPPORTED (-10)    /* parameter outside what the GPU kernels implement */
#define FHE_ERR_DEVICE (-11)         /* HIP runtime error / no device */
#define FHE_ERR_OOM (-12)

#define FHE_MODE_COMPAT 0      /* the reference's transform, bit-exact */
#define FHE_MODE_NEGACYCLIC 1  /* psi-twisted cyclic NTT: polymul == a*b mod (X^N+1) */

#define FHE_HOST 0
#define FHE_DEVICE 1

typedef struct fhe_ctx fhe_ctx;

/* Thread-local message of the last failing call on this thread. */
const char *fhe_last_error(void);
const char *fhe_version(void);
/* Hash of the sources and flags this library was built from (16 hex
 * digits).  Profiles under profiles/ are stamped with it; bench.py uses a
 * PMC traffic figure only when it matches the loaded library.  No reference
 * counterpart (measurement plumbing). */
const char *fhe_build_id(void);

/* ---- hardware ------------------------------------------------------------
 * Replaces HardwareDetector::detect() (hardware_detector.mm; N-API
 * detectHardware(), src/native/lib.rs:123-127, index.d.ts:22-30).          */
typedef struct {
    int32_t device_count;
    int32_t compute_units;     /* of device 0 */
    int32_t wavefront_size;
    int32_t xcds;
    uint64_t hbm_bytes;        /* of device 0 */
    uint64_t lds_bytes_per_cu;
    char arch[32];             /* "gfx950" */
    char name[96];
} fhe_hw_caps;
int fhe_detect(fhe_hw_caps *caps);

/* ---- context: NTTProcessor(degree, modulus) + PolynomialRing(degree, q)
 * (ntt_processor.cpp:134-208, polynomial_ring.cpp:213-222).
 * Validation order and messages follow the reference constructor.  n must
 * be a power of two in [4, 65536]; the GPU kernels implement every such n
 * and every odd q whose root search succeeds: q < 2^62 in the lazy kernel
 * family, 2^62 <= q < 2^64 in the canonical one (ntt_wide.hip; there
 * encrypt / decrypt / add_plain are composed from batched transforms,
 * engine_composed.hip, as they are for n > 16384, and
 * compat mode keeps the reference's psi^-1 and N^-1, which are not inverses
 * at q >= 2^63, ntt_processor.cpp:63-89).  n > 16384 runs as a
 * two-pass row/column split and the context holds 512 MiB of device
 * scratch (every entry point takes such contexts: fused kernels up to
 * n = 16384, composed ones above).
 * device: HIP device ordinal.
 * Side effect: call temporaries come from the device's default
 * stream-ordered memory pool, and creating a context sets that pool's
 * release threshold to FHE_POOL_KEEP_MB MiB (environment, default 8192), so
 * up to that much freed memory stays cached across synchronisations.  The
 * pool is process-wide (other HIP users of the device share it);
 * FHE_POOL_KEEP_MB=0 leaves it unchanged.                                   */
int fhe_ctx_create(uint32_t n, uint64_t q, int mode, int device, fhe_ctx **out);
void fhe_ctx_destroy(fhe_ctx *ctx);
/* Multi-device context (SURVEY.md 8(b) `devices, ndev`): one transform
 * context per listed device (tables, scratch and stream replicated; a
 * device may be listed twice).  Every batch entry point below accepts it:
 *   FHE_HOST    the batch is cut into ndev contiguous balanced ranges, each
 *               staged through its own device by its own host thread (the
 *               reference's batch_encrypt chunks a batch over threads sharing
 *               one read-only NTTProcessor, encryption.cpp:472, 520-533);
 *               returns when every range is back in host memory;
 *   FHE_DEVICE  the pointers are device memory of one listed device and the
 *               call runs there (data stays where it lives; shard across
 *               devices by calling once per device-resident shard).
 * Key preparation (fhe_ggsw_prepare, fhe_relin_key_prepare, fhe_secret_key_prepare,
 * fhe_public_key_prepare) runs on the first device for FHE_HOST.
 * fhe_ctx_set_stream binds the stream to the sub-context of its device.     */
int fhe_ctx_create_multi(uint32_t n, uint64_t q, int mode, const int *devices, int ndev, fhe_ctx **out);
int fhe_ctx_device_count(const fhe_ctx *ctx, int *ndev);
/* The per-device context i (borrowed; owned by ctx).  A single-device
 * context returns itself for i = 0. */
int fhe_ctx_sub(const fhe_ctx *ctx, int i, fhe_ctx **out);
/* Enqueue all later work of this context on the given hipStream_t (e.g. the
 * caller's torch stream).  NULL selects the null (legacy default) stream,
 * which is torch's default stream.  A new context uses a private
 * non-blocking stream until this is called. */
int fhe_ctx_set_stream(fhe_ctx *ctx, void *hip_stream);
void *fhe_ctx_stream(const fhe_ctx *ctx);
int fhe_ctx_synchronize(fhe_ctx *ctx);

typedef struct {
    uint32_t n, log_n;
    uint64_t q;
    uint64_t psi;          /* primitive 2N-th root (smallest generator rule, ntt_processor.cpp:92-128) */
    uint64_t psi_inv;
    uint64_t inv_n;        /* N^-1 mod q */
    int32_t mode;
    int32_t word_bits;     /* 32 (q < 2^30) or 64 (q < 2^64) kernel arithmetic */
    int32_t device;
    int32_t polys_per_block;
    int32_t threads_per_block;
} fhe_ctx_info;
int fhe_ctx_get_info(const fhe_ctx *ctx, fhe_ctx_info *info);
/* The reference's twiddle vectors psi^i / psi^-i, i < n (ntt_processor.cpp:188-202). */
int fhe_ctx_get_twiddles(const fhe_ctx *ctx, uint64_t *forward, uint64_t *inverse);

/* ---- transforms (ntt_processor.cpp:262-408) -----------------------------
 * In place allowed (out == in).                                            */
int fhe_ntt_fwd_batch(fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch, int where);
int fhe_ntt_inv_batch(fhe_ctx *ctx, const uint64_t *in, uint64_t *out, size_t batch, int where);
/* out = to_ntt(a) (.) w, per polynomial (config C3: NTT + modmul). */
int fhe_ntt_fwd_mul_batch(fhe_ctx *ctx, const uint64_t *a, const uint64_t *w, uint64_t *out, size_t batch,
                          int where);

/* ---- PolynomialRing (polynomial_ring.cpp) ------------------------------- */
/* multiply (:421-447) on coefficient-form inputs: inv(fwd(a) (.) fwd(b)). */
int fhe_polymul_batch(fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch, int where);
/* pointwise_multiply (:493-530): c = a*b mod q over n*batch coefficients. */
int fhe_pointwise_batch(fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch, int where);
int fhe_poly_add_batch(fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch, int where);
int fhe_poly_sub_batch(fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch, int where);
int fhe_poly_neg_batch(fhe_ctx *ctx, const uint64_t *a, uint64_t *c, size_t batch, int where);
int fhe_poly_mul_scalar_batch(fhe_ctx *ctx, const uint64_t *a, uint64_t scalar, uint64_t *c, size_t batch,
                              int where);

/* ---- TFHE external product (bootstrap_engine.cpp:152-185, 431-518) ------
 * glwe:  [batch][k+1][n] (k mask polynomials, then the body)
 * ggsw:  [(k+1)*level rows][k+1][n], rows ordered as the reference's
 *        ggsw.matrix (mask digit rows first, digit level inner).
 * fhe_ggsw_prepare turns a coefficient-form GGSW into the NTT-domain form
 * fhe_external_product_batch consumes (same shape).  GLWE dimension k = 1..16:
 * fused kernels for k = 1 and n <= 16384, composed (decompose, batched
 * transforms, key MAC, inverse) otherwise. */
int fhe_ggsw_prepare(fhe_ctx *ctx, uint32_t k, uint32_t level, const uint64_t *ggsw, uint64_t *ggsw_ntt, int where);
int fhe_external_product_batch(fhe_ctx *ctx, uint32_t k, uint32_t base_log, uint32_t level, const uint64_t *glwe,
                               const uint64_t *ggsw_ntt, uint64_t *out, size_t batch, int where);
/* decompose_polynomial (:152-185) for npoly polynomials: out [npoly][level][n]. */
int fhe_decompose_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *poly, uint64_t *out,
                        size_t npoly, int where);

/* ---- RNS multi-modulus ring (PolynomialRing(degree, moduli),
 * polynomial_ring.cpp:224-237): one transform context per modulus, all on
 * one stream.  RNS polynomials are modulus-major: [count][batch][n] (limb i
 * of every polynomial contiguous).  FHE_DEVICE calls run each operation as
 * ONE launch over all limbs (grid.y = limb, per-limb constants from device
 * tables built at creation) when every limb shares the kernel shape (n <=
 * 16384, q < 2^62, all limbs in 32-bit or all in 64-bit lanes, same
 * laziness); otherwise, and for FHE_HOST calls (staged limb by limb), one
 * launch per limb.  FHE_RNS_ONE_LAUNCH=0 forces one launch per limb.  The
 * reference's ring operations use moduli_[0] only; these apply the
 * operation to every limb. */
typedef struct fhe_rns_ctx fhe_rns_ctx;
int fhe_rns_ctx_create(uint32_t n, const uint64_t *moduli, uint32_t count, int mode, int device, fhe_rns_ctx **out);
void fhe_rns_ctx_destroy(fhe_rns_ctx *rns);
int fhe_rns_ctx_limb(const fhe_rns_ctx *rns, uint32_t i, fhe_ctx **out);
int fhe_rns_ntt_fwd_batch(fhe_rns_ctx *rns, const uint64_t *in, uint64_t *out, size_t batch, int where);
int fhe_rns_ntt_inv_batch(fhe_rns_ctx *rns, const uint64_t *in, uint64_t *out, size_t batch, int where);
int fhe_rns_polymul_batch(fhe_rns_ctx *rns, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch,
                          int where);
int fhe_rns_pointwise_batch(fhe_rns_ctx *rns, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch,
                            int where);
int fhe_rns_add_batch(fhe_rns_ctx *rns, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch, int where);
int fhe_rns_sub_batch(fhe_rns_ctx *rns, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch, int where);

/* ---- BFV-style ciphertext multiplication (encryption.cpp:737-980) -------
 * A ciphertext is its component polynomials, contiguous: ct [batch][2][n]
 * (c0, c1); a degree-2 product [batch][3][n] (c0, c1, c2).
 * fhe_ct_multiply_batch  EncryptionEngine::multiply (:737-798): is_ntt = 0
 *   for coefficient-form inputs (4 forward + 3 inverse transforms in one
 *   kernel), 1 when both inputs are already NTT-domain (tensor only).
 * fhe_relin_key_prepare  the KeySwitchKey pairs (a_l, b_l) of
 *   key_manager.cpp:296-324, rlk [level][2][n], into the NTT-domain form
 *   fhe_relinearize_batch consumes (same shape).
 * fhe_relinearize_batch  EncryptionEngine::relinearize (:904-980): digit l
 *   of c2 is (c2 >> l*base_log) & (2^base_log - 1); out [batch][2][n] =
 *   (c0 + sum_l d_l * b_l, c1 + sum_l d_l * a_l).  level = number of key
 *   pairs used (the reference's min(decomp_level, keys.size())); level 0
 *   copies c0, c1.  Requires (level - 1) * base_log < 64, 1 <= base_log <= 63.
 * fhe_ct_multiply_relin_batch  multiply_relin (:800-807): both steps. */
int fhe_ct_multiply_batch(fhe_ctx *ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *out, size_t batch,
                          int is_ntt, int where);
int fhe_relin_key_prepare(fhe_ctx *ctx, uint32_t level, const uint64_t *rlk, uint64_t *rlk_ntt, int where);
int fhe_relinearize_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *ct3,
                          const uint64_t *rlk_ntt, uint64_t *out, size_t batch, int where);
int fhe_ct_multiply_relin_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *ct1,
                                const uint64_t *ct2, const uint64_t *rlk_ntt, uint64_t *out, size_t batch,
                                int where);

/* ---- Galois automorphisms, re-keying and the slot-isolating trace --------
 * Key switching of a degree-1 ciphertext, with or without the automorphism
 * X -> X^g in front of it.  (No reference counterpart: its EncryptionEngine
 * switches only s^2 -> s.)
 * sigma_g  for odd g, 1 <= g < 2n: for every j < n, with k = j*g mod 2n,
 *   out[k] = in[j] mod q when k < n, else out[k - n] = (q - in[j] mod q) % q.
 *   Input words may be any u64, outputs are canonical; g = 1 is the identity,
 *   a copy of the reduced words.
 * fhe_poly_galois_batch    sigma_g of npoly polynomials [npoly][n], out of
 *   place.  Every context: any n, any odd q < 2^64, either mode (no transform
 *   runs).  FHE_ERR_INVALID_ARG: "Galois element must be odd", "Galois element
 *   out of range" (g >= 2n), out overlapping in, a null buffer, npoly == 0; the
 *   parity, null and zero-count checks come before the context is looked at.
 *   A multi-device context splits npoly.
 * fhe_ct_galois_batch      ct [batch][2][n] = (c0, c1) -> out [batch][2][n].
 *   With d_l = (sigma_g(c1) >> l*base_log) & (2^base_log - 1), relinearisation's
 *   unsigned LSB-first digit of the canonical word, and swk_ntt [level][2][n]
 *   the prepared pairs (a_l, b_l) of fhe_switch_key_generate:
 *     out0 = sigma_g(c0) [+ c0 mod q] + sum_l d_l (*) b_l
 *     out1 =             [  c1 mod q] + sum_l d_l (*) a_l
 *   the bracketed terms present when add_input != 0 (the trace step ct +
 *   sigma_g(ct) in one launch).  Word-identical to the chain
 *   fhe_poly_galois_batch on both components, fhe_poly_add_batch when
 *   add_input, and fhe_relinearize_batch on ct3 = (sigma_g(c0) [+ c0],
 *   [c1 mod q | 0], sigma_g(c1)); level 0 therefore copies rows 0 and 1 of that
 *   ct3.  Coefficient form only.  Every context: one fused kernel for n <=
 *   16384 and q < 2^62, otherwise the permutation kernel into a bounded
 *   stream-ordered temporary and the composed relinearisation.  (base_log,
 *   level) as fhe_relinearize_batch.  FHE_ERR_INVALID_ARG: the g errors above,
 *   a null ct or out (or key with level > 0), batch == 0, out overlapping ct;
 *   all but the range and overlap checks come before the context is looked
 *   at.  A multi-device context splits the batch; FHE_HOST stages every
 *   buffer, the key included.
 * fhe_ct_trace_batch       the partial field trace: swk_ntt
 *   [steps][level][2][n], block i the prepared Galois key of g_i = n / 2^i + 1
 *   (g_0 = n + 1 negates the odd coefficients; the last of a full trace is
 *   g = 3); 1 <= steps <= log2(n).  Words: x = fhe_poly_mul_scalar_batch(ct,
 *   (2^steps)^-1 mod q), then x <- fhe_ct_galois_batch(g_i, key_i, x,
 *   add_input = 1) for i = 0 .. steps-1, bit-identical to that chain; the
 *   steps ping-pong between out and one stream-ordered temporary without a
 *   host synchronisation.  In negacyclic mode the coefficients of the phase at
 *   multiples of 2^steps come back exactly (message and input noise; the
 *   pre-multiplication is mod q, not mod t, so t may be even) and every other
 *   coefficient becomes 0 plus key-switch noise; after steps = log2(n) only
 *   coefficient 0 survives.
 * Meaning and modes: the words are defined in both modes.  For g != 1 the
 *   result decrypts to sigma_g of the message only under FHE_MODE_NEGACYCLIC:
 *   the compat transform product does not commute with sigma_g, exactly as
 *   packed slots other than 0.  For g = 1 (re-keying) the message moves to
 *   sk_to in both modes (only the bilinearity and associativity of the
 *   context's product (*) are used), but the key-switch noise sum_l d_l (*) e_l
 *   is small only under the true ring product: the compat product of two small
 *   polynomials is not small once their degrees add up to n or more.  A
 *   re-keyed ciphertext therefore decrypts under sk_to in compat mode only
 *   with key errors confined to coefficient 0 (constants multiply as scalars),
 *   and with real keys only under FHE_MODE_NEGACYCLIC; the exact-integer model
 *   of tests/test_galois_abi.py shows both. */
int fhe_poly_galois_batch(fhe_ctx *ctx, uint32_t g, const uint64_t *in, uint64_t *out, size_t npoly, int where);
int fhe_ct_galois_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, uint32_t g, const uint64_t *swk_ntt,
                        const uint64_t *ct, int add_input, uint64_t *out, size_t batch, int where);
int fhe_ct_trace_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, uint32_t steps, const uint64_t *swk_ntt,
                       const uint64_t *ct, uint64_t *out, size_t batch, int where);

/* ---- ciphertext squaring and anomaly score (encryption.cpp:1004-1055, 1305-1321)
 * EncryptionEngine::square / square_relin and compute_anomaly_score's
 * relinearize(square(subtract(ballot, expected))).  The words equal
 * fhe_ct_multiply_batch(d, d) with d = ct - ref from fhe_poly_sub_batch, bit
 * for bit; input words may be any u64 (mod_sub's contract).  Coefficient form
 * runs 2 forward + 3 inverse transforms in one kernel with the subtraction
 * done while loading; is_ntt = 1 is one streaming pass.
 * out[i] = square(ct[i] - ref[...]) : ct [batch][2][n] -> out [batch][3][n].
 * ref == NULL, ref_count == 0: plain square.  ref_count == 1: one ciphertext for the whole batch.
 * ref_count == batch: one per ciphertext.  Any other count: FHE_ERR_INVALID_ARG.
 * out may not overlap ct or ref. */
int fhe_ct_square_batch(fhe_ctx *ctx, const uint64_t *ct, const uint64_t *ref, size_t ref_count,
                        uint64_t *out, size_t batch, int is_ntt, int where);
/* relinearize(the above): out [batch][2][n]; coefficient form only, as fhe_ct_multiply_relin_batch */
int fhe_ct_square_relin_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *ct,
                              const uint64_t *ref, size_t ref_count, const uint64_t *rlk_ntt,
                              uint64_t *out, size_t batch, int where);

/* ---- scale-invariant BFV multiplication ----------------------------------
 * fhe_ct_multiply_batch, fhe_ct_dot_batch and fhe_ct_square_batch are the
 * reference's multiply: the tensor product mod q, whose result carries
 * Delta^2 m.  The calls below are the BFV product round(t/q (ct1 (x) ct2))
 * taken over the integers, whose result carries Delta m and decrypts with
 * real keys and real noise.  They are new entry points; the words of the
 * calls above are unchanged.
 *
 * Definition (exact integers).  q is the context modulus (odd), t the
 * plaintext modulus (0 selects 4), 2 <= t < q.
 *   lift(x), any u64 x: r = x mod q; r when r <= (q-1)/2, else r - q.
 *   For a = (a0, a1), b = (b0, b1) and (*) the negacyclic product in
 *   Z[X]/(X^n + 1) over the integers:
 *     X0 = lift(a0) (*) lift(b0)
 *     X1 = lift(a0) (*) lift(b1) + lift(a1) (*) lift(b0)
 *     X2 = lift(a1) (*) lift(b1)
 *   rnd(Y) = the integer nearest to Y / q (no ties: q is odd).
 *   out word = rnd(t X) mod q, canonical in [0, q).
 * fhe_ct_dot_scaled_batch rescales ONCE, after summing: out[g] = rnd(t sum_i
 * X_i) mod q.  Rounding is not linear, so this is NOT word-identical to a sum
 * of fhe_ct_multiply_scaled_batch results: it carries one rounding error
 * instead of `count` (the same kind of difference as the lazy relinearisation
 * of fhe_ct_dot_batch).  fhe_ct_square_scaled_batch is the multiply of d = ct
 * - ref (fhe_poly_sub_batch) with itself, word for word.
 *
 * Opening.  The phase of the result is c0 - c1 s + c2 s^2, the sign that
 * fhe_relinearize_batch implements.  The reference's degree-2 decrypt
 * SUBTRACTS c2 s^2, so fhe_decrypt_batch(components = 3) is not the way to
 * open these: relinearise first (fhe_relinearize_batch, unchanged) and
 * decrypt the degree-1 result.
 *
 * Contexts.  FHE_MODE_NEGACYCLIC only (a compat context fails at creation
 * with FHE_ERR_UNSUPPORTED: the rescale has a meaning only under the true ring
 * product), coefficient form only, single-device contexts only
 * (FHE_ERR_UNSUPPORTED for a multi-device one).  Every n and odd q the
 * negacyclic context takes.  The scale context BORROWS ctx, follows ctx's
 * stream at every call, and must be destroyed before ctx.
 *
 * Method.  The tensor runs in three channels with the existing kernels: mod q
 * on ctx, and mod two auxiliary NTT primes (fhe_scale_info.aux; fixed library
 * constants below 2^62, = 1 mod 2^17, different from q) on two auxiliary
 * contexts, fed by fhe_poly_center_lift_batch's kernel.  Reduction Z -> Z_p
 * commutes with (*), so each channel is exact, and fhe_poly_scale_round_batch's
 * kernel recovers rnd(t X) from the three residues as long as
 * t count n q < aux[0] aux[1] (about 2^122).  max_count is the largest such
 * count; a larger count answers FHE_ERR_UNSUPPORTED and the message names it;
 * a (q, t, n) with max_count 0 fails at creation.  When t count n q < aux[0]
 * the first auxiliary prime alone determines the result and only its channel
 * runs (decided per call; the words are the same by definition).  Batches run in chunks of
 * pairs with stream-ordered temporaries of at most 1 GiB; FHE_SCALE_CHUNK=
 * <pairs> forces the chunk (read per call).  FHE_HOST stages chunk by chunk.
 *
 * FHE_ERR_INVALID_ARG: a null pointer; batch, count, groups or npoly 0; a bad
 * ref_count (as fhe_ct_square_batch); an output overlapping an input; t < 2 or
 * t >= q; device buffers not 16-byte aligned.  The null and zero-count checks
 * come before the context is looked at. */
typedef struct fhe_scale_ctx fhe_scale_ctx;
typedef struct { uint64_t q, t, aux[2]; uint32_t n, naux; uint64_t max_count; } fhe_scale_info;
int fhe_scale_ctx_create(fhe_ctx *ctx, uint64_t t, fhe_scale_ctx **out);
void fhe_scale_ctx_destroy(fhe_scale_ctx *sc);
int fhe_scale_ctx_get_info(const fhe_scale_ctx *sc, fhe_scale_info *info);
/* the two kernels, callable on their own.  in [npoly][n], any u64 words ->
 * out_p1, out_p2 [npoly][n] = lift(in) mod aux[0], mod aux[1], canonical */
int fhe_poly_center_lift_batch(fhe_scale_ctx *sc, const uint64_t *in, uint64_t *out_p1, uint64_t *out_p2, size_t npoly, int where);
/* the lift of ct - ref (mod_sub, then lift): ct [batch][2][n], ref / ref_count as fhe_ct_square_batch */
int fhe_ct_center_lift_batch(fhe_scale_ctx *sc, const uint64_t *ct, const uint64_t *ref, size_t ref_count, uint64_t *out_p1, uint64_t *out_p2, size_t batch, int where);
/* xq, xp1, xp2 [npoly][n]: X mod q, mod aux[0], mod aux[1] (any u64 words,
 * read mod their modulus) -> out [npoly][n] = rnd(t X) mod q for the X with
 * |rnd(t X)| < aux[0] aux[1] / 2 */
int fhe_poly_scale_round_batch(fhe_scale_ctx *sc, const uint64_t *xq, const uint64_t *xp1, const uint64_t *xp2, uint64_t *out, size_t npoly, int where);
/* ct1, ct2 [batch][2][n] -> out [batch][3][n] */
int fhe_ct_multiply_scaled_batch(fhe_scale_ctx *sc, const uint64_t *ct1, const uint64_t *ct2, uint64_t *out, size_t batch, int where);
/* a, b [groups][count][2][n] -> out [groups][3][n], one rescale per group */
int fhe_ct_dot_scaled_batch(fhe_scale_ctx *sc, const uint64_t *a, const uint64_t *b, size_t count, size_t groups, uint64_t *out, int where);
/* square(ct - ref), ref / ref_count as fhe_ct_square_batch */
int fhe_ct_square_scaled_batch(fhe_scale_ctx *sc, const uint64_t *ct, const uint64_t *ref, size_t ref_count, uint64_t *out, size_t batch, int where);

/* ---- SIMD batching: slot encode / decode, slot rotations, slot sums -------
 * CRT batching of BFV plaintexts.  (No reference counterpart: its "packed"
 * plaintext writes values into coefficients.)  n a power of two >= 4, t odd
 * with t = 1 (mod 2n), psi the primitive 2n-th root that a negacyclic context
 * (n, t) reports (fhe_ctx_info.psi; fhe_simd_info.psi).
 *
 * Slots.  n slots in 2 rows of n/2 columns, s = r n/2 + i.  Exponent e(s) =
 *   3^i mod 2n for r = 0 and 2n - (3^i mod 2n) for r = 1 (every odd residue
 *   below 2n exactly once); transform index k(s) = (e(s) - 1) / 2, the table
 *   fhe_simd_slot_index returns (host [n]).
 * encode.  X[k(s)] = values[s] mod t; out = the words of fhe_ntt_inv_batch on
 *   the negacyclic context (n, t) applied to X, canonical in [0, t): the
 *   polynomial with out(psi^e(s)) = values[s].  With lift != 0 each word c is
 *   returned as its centred representative mod q: c when c <= (t - 1) / 2,
 *   else q - (t - c) -- the form multiply_plain / fhe_ct_dot_plain_batch want;
 *   lift == 0 is the form fhe_encrypt_batch / fhe_add_plain_batch take as
 *   `values`.  Input words are any u64, read mod t.
 * decode.  out[s] = Y[k(s)], Y the words of fhe_ntt_fwd_batch on that context
 *   applied to the input (any u64, read mod t): the `values` output of
 *   fhe_decrypt_batch / fhe_combine_partials_batch.
 * The slot-wise meaning assumes a prime t: t is not tested for primality, and
 *   for a composite t that passes the inner context's checks the words are
 *   still the ones defined above.  Ring products of encodings decode to
 *   slot-wise products mod t, sums to slot-wise sums.
 * Rotation element.  g(steps, swap) = 3^(steps mod n/2) (2n - 1)^swap mod 2n
 *   (fhe_simd_rotation_element: pure host arithmetic, no GPU; steps is signed,
 *   a negative value rotates right; FHE_ERR_INVALID_ARG for n not a power of
 *   two in [4, 65536] or a null g).  If m encodes v, sigma_g(m)
 *   (fhe_poly_galois_batch) decodes to w[r][i] = v[r xor swap][(i + steps)
 *   mod n/2].
 * Slot sum.  With g_i = 3^(2^i) mod 2n for i < log2(n/2), then g = 2n - 1
 *   (log2 n elements in all), x <- x + sigma_{g_i}(x) over all of them leaves
 *   sum_s v_s in every slot; without the last element each slot holds its
 *   row's sum.  On ciphertexts this is fhe_ct_galois_chain_batch with
 *   add_input = 1 (sum_slots).  Noise: every step doubles the noise and adds
 *   one key switch, so log2 n steps cost about n x the input noise.  At
 *   t = 65537 with a 62-bit q and a 2^16 x 4 key-switch base the slot sum
 *   after a scaled product has a margin of only 8 - 17 at n = 64 and no longer
 *   decodes at n = 256: sum_slots after a multiplication needs a small t
 *   (t = 257 leaves a margin above 10^7 there) or a finer key-switch base.
 * These are SIMD slots.  The "slot" of fhe_slot_extract_batch,
 *   fhe_lwe_pack_batch and the slot-isolating trace is a COEFFICIENT index:
 *   fhe_ct_trace_batch keeps coefficients, not SIMD slots, and a packed
 *   comparison bit sits at a coefficient.
 *
 * fhe_simd_ctx_create mirrors fhe_scale_ctx_create: it BORROWS ctx (n, device,
 *   q for `lift`, and the stream, followed at every call) and must be
 *   destroyed before ctx.  It owns a negacyclic context (n, t) on the same
 *   device and the two index tables on the device.  Errors: "null out" / "null
 *   context" before anything else; FHE_ERR_UNSUPPORTED for a compat or a
 *   multi-device ctx; FHE_ERR_INVALID_ARG for t < 3 or t >= q; otherwise
 *   whatever the inner fhe_ctx_create(n, t) answers (even t, t != 1 mod 2n, no
 *   root), code and message unchanged.
 * fhe_simd_encode_batch / fhe_simd_decode_batch: buffers [batch][n], out of
 *   place (overlap: FHE_ERR_INVALID_ARG).  A null buffer and batch == 0 are
 *   checked before the context is looked at ("null buffer", "at least one
 *   polynomial is needed", then "null simd context").  Device buffers must be
 *   16-byte aligned; FHE_HOST stages chunk by chunk.  Every n the context
 *   takes and every t: n <= 16384 and t < 2^62 run one fused kernel (the
 *   permutation is part of the transform's load / store; 32-bit lanes for t <
 *   2^30); n > 16384 or t >= 2^62 run composed -- a permutation kernel and the
 *   batched transforms through one stream-ordered temporary of at most 1 GiB
 *   per chunk, no host synchronisation -- with bit-identical words.
 *   FHE_SIMD_FUSED=0 (read per call) forces the composed path.
 * fhe_ct_galois_chain_batch: x_0 = ct, x_{i+1} = fhe_ct_galois_batch(g =
 *   gs[i], key block key_idx ? key_idx[i] : i of swk_ntt [nkeys][level][2][n],
 *   x_i, add_input) for i < nsteps, out = x_nsteps: word-identical to that
 *   chain of calls.  gs / key_idx are HOST arrays in both residences, copied
 *   before the call returns.  Every context fhe_ct_galois_batch takes, a
 *   multi-device one (splits the batch) and FHE_HOST included; the steps
 *   ping-pong between out and one stream-ordered temporary without a host
 *   synchronisation.  add_input = 0 composes rotations, add_input = 1 is
 *   rotate-and-sum.  Errors: fhe_ct_galois_batch's own; nsteps == 0 or nsteps
 *   > 64: "steps must be between 1 and 64"; a null gs; every g is checked
 *   (odd, then range) before any launch. */
typedef struct fhe_simd_ctx fhe_simd_ctx;
typedef struct { uint64_t q, t, psi; uint32_t n; int32_t word_bits; } fhe_simd_info;   /* 32 bytes */
int fhe_simd_ctx_create(fhe_ctx *ctx, uint64_t t, fhe_simd_ctx **out);
void fhe_simd_ctx_destroy(fhe_simd_ctx *sc);
int fhe_simd_ctx_get_info(const fhe_simd_ctx *sc, fhe_simd_info *info);
int fhe_simd_slot_index(const fhe_simd_ctx *sc, uint32_t *index);          /* host [n]: k(s) */
int fhe_simd_rotation_element(uint32_t n, int64_t steps, int swap_rows, uint32_t *g);   /* host only, no GPU */
int fhe_simd_encode_batch(fhe_simd_ctx *sc, const uint64_t *values, int lift, uint64_t *out, size_t batch, int where);
int fhe_simd_decode_batch(fhe_simd_ctx *sc, const uint64_t *in, uint64_t *out, size_t batch, int where);
int fhe_ct_galois_chain_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, uint32_t nsteps, const uint32_t *gs,
                              const uint32_t *key_idx, const uint64_t *swk_ntt, const uint64_t *ct, int add_input,
                              uint64_t *out, size_t batch, int where);

/* ---- hoisted rotations and the plaintext linear transform -----------------
 * Many rotations of ONE ciphertext, and sum_r p_r (*) rot_r(ct) for plaintext
 * polynomials p_r (a plaintext matrix applied to a packed encrypted vector, one
 * term per diagonal).  (No reference counterpart.)  The ciphertext is
 * decomposed and transformed once; every automorphism then acts on spectra.
 * In the negacyclic transform X_k = a(psi^(2k+1)), natural order, and sigma_g
 * is the index map pi_g(k) = (((2k+1) g mod 2n) - 1) / 2 = g k + (g - 1) / 2
 * mod n: fwd(sigma_g(a))[k] = fwd(a)[pi_g(k)], no sign and no arithmetic.
 * R rotations cost level + 1 forward transforms in all and two inverse
 * transforms each; a whole linear transform costs level + 1 forward and two
 * inverse transforms.
 *
 * fhe_ct_hoist_batch          ct [batch][2][n] (any u64 words) -> hoisted
 *   [batch][1 + level][n]:
 *     row 0     = the words of fhe_ntt_fwd_batch(c0)
 *     row 1 + l = the words of fhe_ntt_fwd_batch(d_l),
 *                 d_l = ((c1 mod q) >> l*base_log) & (2^base_log - 1)
 *   relinearisation's unsigned digits of c1 ITSELF, not of sigma_g(c1).
 *   (base_log, level) as fhe_relinearize_batch, and level >= 1 ("at least one
 *   decomposition level is needed").
 * fhe_ct_hoisted_galois_batch hoisted -> out [batch][nrot][2][n].  With g =
 *   gs[r] and (a_l, b_l) key block key_idx ? key_idx[r] : r of swk_ntt
 *   [nkeys][level][2][n] (the prepared Galois keys of fhe_switch_key_generate,
 *   unchanged: sum_l sigma_g(d_l) 2^(l base_log) = sigma_g(c1) mod q):
 *     out0 = sigma_g(c0) + sum_l sigma_g(d_l) (*) b_l
 *     out1 =               sum_l sigma_g(d_l) (*) a_l
 *   canonical, coefficient form.  Word-identical to the chain:
 *   fhe_poly_galois_batch on c0 and on each digit row (sigma_g mod q turns a
 *   digit d into q - d where it negates), fhe_ntt_fwd_batch,
 *   fhe_pointwise_batch with fhe_ntt_fwd_batch of the key rows a_l / b_l (the
 *   prepared rows without their Montgomery factor), fhe_poly_add_batch,
 *   fhe_ntt_inv_batch.  For g = 1 the words equal fhe_ct_galois_batch(g = 1,
 *   add_input = 0) exactly.  For g != 1 they DIFFER from fhe_ct_galois_batch,
 *   whose digits are those of sigma_g(c1) (digits in [0, 2^base_log)), while
 *   here they are sigma_g of the digits of c1 (in (-2^base_log, 2^base_log)):
 *   both decrypt to sigma_g of the message with the same noise bound,
 *   level n (2^base_log - 1) max|e|.  1 <= nrot <= 4096 ("rotations must be
 *   between 1 and 4096").
 * fhe_ct_hoisted_linear_batch pts_ntt [nterms][n]: the fhe_ntt_fwd_batch
 *   words of already-encoded, lifted plaintext polynomials p_r, shared by the
 *   batch.  out[b] = sum_r p_r (*) (rotation r of ciphertext b as above),
 *   [batch][2][n]; accumulate != 0 reads out as one more degree-1 term (the
 *   unrotated diagonal enters this way without a key switch: multiply_plain
 *   first).  Word-identical to fhe_ct_hoisted_galois_batch, fhe_polymul_batch
 *   of both components with fhe_ntt_inv_batch(p_r), fhe_ct_sum_batch: every
 *   step is exact arithmetic on canonical residues.  The plaintext is
 *   multiplied in once per term, on the spectrum of the bracket, and the sum
 *   over r runs on spectra.  1 <= nterms <= 4096 ("terms must be between 1 and
 *   4096").  Noise: terms n (t/2) (input noise + the key-switch bound above).
 * Common rules.  FHE_MODE_NEGACYCLIC single-device contexts only: a compat or
 *   a multi-device context answers FHE_ERR_UNSUPPORTED (the compat transform
 *   does not turn sigma_g into a spectrum permutation), as fhe_simd_ctx_create.
 *   where: device, or host (every buffer staged, keys and plaintexts included).
 *   gs / key_idx are HOST arrays in both residences, copied before the call
 *   returns.  Every g is checked (odd first, then range) and every entry of
 *   key_idx (below n: a ring of degree n has n Galois elements, no table of
 *   distinct keys is longer; "key index out of range") before any launch.  The call carries no key count:
 *   THE CALLER GUARANTEES that swk_ntt holds max(key_idx) + 1 key blocks (nrot /
 *   nterms blocks with key_idx == NULL); an index beyond the table reads past it.  FHE_ERR_INVALID_ARG: a null
 *   buffer, batch == 0, a zero or too large count, out overlapping an input
 *   ("output must not overlap ..."), device buffers not 16-byte aligned; the
 *   count, null, parity and zero-batch checks come before the context is looked
 *   at.  Hoisted and plaintext rows are read as canonical words.
 * Paths.  Two, with bit-identical words and no host synchronisation.  Fused
 *   kernels (n <= 16384 and q < 2^62 only): the digit extraction inside the
 *   forward transforms; the gathered key MAC, one workgroup per (ciphertext,
 *   rotation, component), inside the inverse transform.  Composed: a digit
 *   kernel and the batched forward transform; a streaming gathered MAC and the
 *   batched inverse transform in place in the output (the accumulating linear
 *   transform through a stream-ordered temporary of at most 1 GiB per chunk).
 *   The fused path is taken where its grid fills the device: the hoist from 256
 *   ciphertexts, the rotations from batch * nrot >= 4096; the linear transform
 *   and everything smaller run composed.  FHE_HOIST_FUSED=0 (read per call)
 *   forces the composed path, FHE_HOIST_FUSED=1 the fused one where it exists. */
int fhe_ct_hoist_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *ct, uint64_t *hoisted,
                       size_t batch, int where);
int fhe_ct_hoisted_galois_batch(fhe_ctx *ctx, uint32_t level, uint32_t nrot, const uint32_t *gs, const uint32_t *key_idx,
                                const uint64_t *swk_ntt, const uint64_t *hoisted, uint64_t *out, size_t batch, int where);
int fhe_ct_hoisted_linear_batch(fhe_ctx *ctx, uint32_t level, uint32_t nterms, const uint32_t *gs, const uint32_t *key_idx,
                                const uint64_t *swk_ntt, const uint64_t *pts_ntt, const uint64_t *hoisted, int accumulate,
                                uint64_t *out, size_t batch, int where);

/* ---- ciphertext tally (encryption.cpp:1061-1067, 1153-1168, 1327-1460) ---
 * EncryptionEngine::batch_add / batch_add_tree / tally_votes /
 * tally_multi_candidate: the sum of `count` ciphertexts of `polys` (1..3)
 * polynomials each, out[w] = sum_i (ct_i[w] mod q) mod q over the polys * n
 * words of a ciphertext, canonical.  mod_add is associative and commutative
 * on residues, so the result equals the reference's sequential and tree
 * folds bit for bit; input words may be any u64 (mod_add's contract).  One
 * kernel launch reads every ballot once (two when the ballots are split
 * across the chip; FHE_TALLY_SPLIT=<S> forces the number of slices, clamped
 * to count).  count == 0 fails with "Cannot add empty vector of ciphertexts"
 * (:1329); count == 1 gives that ciphertext reduced mod q (the reference
 * returns a copy).  accumulate != 0 reads `out` as one more term.  `out` must
 * not overlap any input (not checked).
 * fhe_ct_sum_batch  cts [groups][count][polys][n] -> out [groups][polys][n]:
 *   `groups` independent tallies.  FHE_HOST stages the ballots chunk by
 *   chunk and folds the chunks with the accumulate flag.  A multi-device
 *   context splits the groups.
 * fhe_ct_sum_ptrs   cts is a HOST array of `count` DEVICE pointers, each to
 *   polys * n words and 16-byte aligned (every ciphertext in its own buffer;
 *   a pointer may repeat); out is a device buffer.  The table is copied
 *   before the call returns: the caller may free it at once.  On a
 *   multi-device context the call runs on the device that holds cts[0], and
 *   every pointer must be memory of that device. */
int fhe_ct_sum_batch(fhe_ctx *ctx, const uint64_t *cts, uint32_t polys, size_t count, size_t groups, int accumulate,
                     uint64_t *out, int where);
int fhe_ct_sum_ptrs(fhe_ctx *ctx, const uint64_t *const *cts, uint32_t polys, size_t count, int accumulate,
                    uint64_t *out);

/* ---- ciphertext inner product (encryption.cpp:1069-1110, :737-798) -------
 * out[g] = sum_i multiply(a[g][i], b[g][i]), the degree-2 sum folded by
 * add(): the weighted tally of EncryptionEngine::tally_weighted_votes before
 * its relinearisation, an encrypted dot product, a sum of squares.  The
 * inverse transform is a Z_q-linear map, so on canonical residues
 *   sum_i multiply(a_i, b_i) = ( inv(sum X0_i Y0_i),
 *                                inv(sum (X0_i Y1_i + X1_i Y0_i)),
 *                                inv(sum X1_i Y1_i) )
 * holds bit for bit: the call runs four forward transforms per pair and three
 * inverse transforms per slice of pairs, writes no intermediate ciphertext,
 * and its words equal fhe_ct_multiply_batch followed by fhe_ct_sum_batch
 * (polys = 3).  Inputs may be any u64 (read as x mod q); outputs are
 * canonical.  The pairs are split into slices across the chip and the partial
 * rows folded by the tally kernel; FHE_DOT_SPLIT=<S> forces the number of
 * slices (read per call, clamped to count).  While three times the slices
 * still fit on the chip (few pairs), each of the three sums of a slice runs on
 * a workgroup of its own; FHE_DOT_COMPONENTS=0|1 forces that off or on.
 * Between the two (one pair per slice, too many slices for that) contiguous
 * operands take the multiply kernel into the partial rows: there the fused
 * kernel would be a multiply that also parks its spectra.
 * is_ntt != 0: the inputs are
 * NTT-domain and so is the result (no transform runs).  count == 0 fails with
 * "Cannot tally empty ballot list" (:1080).  accumulate != 0 reads `out` as
 * one more degree-2 term (any u64 words).  `out` must not overlap an input.
 * Shapes outside the fused family (n > 16384, or q >= 2^62) run composed:
 * chunks of the unfused multiply into a bounded temporary, each folded into
 * `out` by the tally kernel -- bit-exact, not expected to be fast.
 *
 * Relinearising the sum once (lazy relinearisation) is NOT word-identical to
 * the reference's relinearise-per-ballot fold: the digit decomposition of c2
 * is not linear.  It decrypts to the same plaintext, with less noise (one
 * key-switch error instead of `count`).
 * fhe_ct_dot_batch  a, b [groups][count][2][n] -> out [groups][3][n]:
 *   `groups` independent inner products.  FHE_HOST stages chunks of pairs and
 *   folds them with the accumulate flag.  A multi-device context splits the
 *   groups.  Device buffers must be 16-byte aligned.
 * fhe_ct_dot_ptrs   a, b are HOST arrays of `count` DEVICE pointers, each to
 *   one ciphertext (2 n words, 16-byte aligned); pointers may repeat and
 *   a[i] == b[i] gives a square; out is a device buffer.  The tables are
 *   copied before the call returns.  On a multi-device context the call runs
 *   on the device that holds a[0], and every pointer must be memory of that
 *   device. */
int fhe_ct_dot_batch(fhe_ctx *ctx, const uint64_t *a, const uint64_t *b, size_t count, size_t groups, int is_ntt,
                     int accumulate, uint64_t *out, int where);
int fhe_ct_dot_ptrs(fhe_ctx *ctx, const uint64_t *const *a, const uint64_t *const *b, size_t count, int is_ntt,
                    int accumulate, uint64_t *out);

/* ---- public-weight tallies (encryption.cpp:890-902, :809-852, :1327-1460) --
 * The weighted tally whose weights are public (share counts, district
 * multipliers, per-ballot masks): no degree-2 result, no relinearisation key.
 *
 * Integer weights: out[g][w] = sum_i ((cts[g][i][w] mod q) * (scalars[g][i]
 * mod q) mod q) mod q over the polys * n words of a ciphertext, canonical --
 * EncryptionEngine::multiply_scalar (:890-902; PolynomialRing::multiply_scalar,
 * polynomial_ring.cpp:454-473) per ballot folded by add().  The products are
 * canonical residues and mod_add is associative and commutative on them, so
 * the words equal fhe_poly_mul_scalar_batch per ballot followed by
 * fhe_ct_sum_batch bit for bit, in one pass over the ballots instead of
 * three.  Words and scalars may be any u64; any odd q < 2^64 and any n the
 * context takes run the same kernel.  The scalar is reduced and prepared once
 * per ballot, not per word.  The ballots are split into slices as the plain
 * tally's (FHE_TALLY_SPLIT=<S> forces the number, clamped to count).
 * count == 0 fails with "Cannot add empty vector of ciphertexts".
 * accumulate != 0 reads `out` as one more (unscaled) term.  `out` must not
 * overlap an input (checked).
 * fhe_ct_sum_scaled_batch  cts [groups][count][polys][n], polys 1..3, scalars
 *   [groups][count] in the same residence as cts -> out [groups][polys][n].
 *   FHE_HOST stages the ballots chunk by chunk and folds the chunks with the
 *   accumulate flag.  A multi-device context splits the groups.  Device
 *   ciphertext buffers must be 16-byte aligned.
 * fhe_ct_sum_scaled_ptrs   cts is a HOST array of `count` DEVICE pointers
 *   (polys * n words each, 16-byte aligned, may repeat), scalars a HOST array
 *   of `count` u64; out is a device buffer.  Both are copied before the call
 *   returns.  On a multi-device context the call runs on the device that holds
 *   cts[0], and every pointer must be memory of that device.
 *
 * Plaintext-polynomial weights: out[g] = sum_i multiply_plain(cts[g][i],
 * pts[g][i]) folded by add() = (sum_i c0_i (*) p_i, sum_i c1_i (*) p_i), with
 * pts the already-encoded plaintext polynomials (any u64, read as x mod q).
 * The inverse transform is a Z_q-linear map, so on canonical residues
 *   sum_i multiply_plain(ct_i, p_i) = ( inv(sum C0_i P_i), inv(sum C1_i P_i) )
 * holds bit for bit: three forward transforms per pair and two inverse
 * transforms per slice of pairs, no intermediate ciphertext, and the words of
 * fhe_polymul_batch of each component with the plaintext followed by
 * fhe_ct_sum_batch (polys = 2).  is_ntt != 0: the ciphertexts and the result
 * are NTT-domain, pts are still coefficient form and are forward-transformed
 * (:819-821); no inverse runs, and the words are those of fhe_ntt_fwd_batch(pt)
 * and fhe_pointwise_batch followed by fhe_ct_sum_batch.  The pairs are split
 * into slices across the chip and the partial rows folded by the tally kernel;
 * FHE_DOT_SPLIT=<S> forces the number of slices (read per call, clamped to
 * count).  There is no by-component variant: FHE_DOT_COMPONENTS has no effect
 * on these calls.  count == 0 fails with "Cannot tally empty ballot list".
 * accumulate != 0 reads `out` as one more degree-1 term (any u64 words).
 * `out` must not overlap an input.  Shapes outside the fused family
 * (n > 16384, or q >= 2^62) run composed: chunks of batched transforms and
 * pointwise products into a bounded temporary, each folded into `out` by the
 * tally kernel -- bit-exact, not expected to be fast.
 * fhe_ct_dot_plain_batch  cts [groups][count][2][n], pts [groups][count][n] ->
 *   out [groups][2][n].  FHE_HOST stages chunks of pairs and folds them with
 *   the accumulate flag.  A multi-device context splits the groups.  Device
 *   buffers must be 16-byte aligned.
 * fhe_ct_dot_plain_ptrs   cts, pts are HOST arrays of `count` DEVICE pointers
 *   (2 n and n words, 16-byte aligned; pointers may repeat, one plaintext may
 *   weigh several ballots); out is a device buffer.  The tables are copied
 *   before the call returns.  On a multi-device context the call runs on the
 *   device that holds cts[0], and every pointer must be memory of that device. */
int fhe_ct_sum_scaled_batch(fhe_ctx *ctx, const uint64_t *cts, const uint64_t *scalars, uint32_t polys, size_t count,
                            size_t groups, int accumulate, uint64_t *out, int where);
int fhe_ct_sum_scaled_ptrs(fhe_ctx *ctx, const uint64_t *const *cts, const uint64_t *scalars, uint32_t polys,
                           size_t count, int accumulate, uint64_t *out);
int fhe_ct_dot_plain_batch(fhe_ctx *ctx, const uint64_t *cts, const uint64_t *pts, size_t count, size_t groups,
                           int is_ntt, int accumulate, uint64_t *out, int where);
int fhe_ct_dot_plain_ptrs(fhe_ctx *ctx, const uint64_t *const *cts, const uint64_t *const *pts, size_t count,
                          int is_ntt, int accumulate, uint64_t *out);

/* ---- TFHE bootstrapping pieces (bootstrap_engine.cpp) --------------------
 * GLWE [batch][k+1][n] as above; LWE masks [batch][dim], bodies [batch].
 * fhe_glwe_rotate_batch    multiply_glwe_by_monomial (:249-261) by X^rot[c].
 * fhe_cmux_batch           cmux (:520-540): ct0 + ggsw (x) (ct1 - ct0).
 * fhe_blind_rotate_batch   blind_rotate (:547-577) of acc in place, for each
 *   ciphertext c with its own LWE (lwe_a[c], lwe_b[c]) modulo lwe_q; bsk_ntt
 *   = lwe_dim prepared GGSWs ([lwe_dim][(k+1)*level][k+1][n]).
 *   Rotation rule (:560, :568): the amount of a word w is
 *     (int32_t)(uint32_t)((w * 2n + lwe_q / 2) / lwe_q)
 *   in uint64_t arithmetic: the product wraps at 2^64 and so does the sum
 *   (near 2^62 a uniform word gives 0..4), and the quotient is truncated to
 *   its low 32 bits, read as signed.  Mask and body words are used raw, not
 *   reduced modulo lwe_q; lwe_q need not equal the ring modulus.  acc is
 *   first multiplied by X^-amount(lwe_b) (a body whose amount is INT32_MIN
 *   is undefined in the reference); then step i, for amount(lwe_a[i]) = r,
 *   is skipped when r == 0 (the accumulator keeps its words, raw ones
 *   included) and otherwise computes acc <- cmux(bsk[i], acc, X^r acc), also
 *   when r is a non-zero multiple of 2n, where X^r acc = acc and the step
 *   only reduces the accumulator words below q.  k = 1 with
 *   n <= 16384 runs fused: one launch for the whole loop at n = 512..4096
 *   (two CUs per ciphertext while 16 * ceil(batch / 8) <= CUs, else one;
 *   2 * level CUs at level 2 / 3 while 2 * level * ceil(batch / 8) <= the
 *   CUs of one XCD, FHE_BR_MULTI=0 keeps two; FHE_BR_PAIR=0 forces one),
 *   per-step CMux launches above; k = 2..4 run
 *   as one launch where the k + 1 accumulators fit in LDS (n = 512 / 1024
 *   with 64-bit words; n = 2048 for k <= 3 with 32-bit words); other
 *   k <= 16 and n = 32768 / 65536 run composed step by step (one digit
 *   buffer for the whole loop, stream-ordered, no host synchronisation).  The multi-CU
 *   launch needs the workgroups of a ciphertext co-resident.  It is never
 *   assumed: multi-CU launches of one process are serialised per device,
 *   and a workgroup whose partners do not answer within
 *   FHE_BR_PAIR_TIMEOUT_US (default 20000 us; 0 simulates a partner that
 *   never answers, for tests) gives its
 *   ciphertext up: a repair pass enqueued behind the launch recomputes every
 *   given-up ciphertext on one CU from a saved copy of its input, so the
 *   result is exact in every case (no host synchronisation either way).
 *   fhe_br_repair_count reports how many ciphertexts took the repair pass.
 *   fhe_bootstrap_batch takes the same shapes.
 * fhe_sample_extract_batch sample_extract (:594-624): lwe_a [batch][k*n].
 * fhe_key_switch_batch     key_switch (:626-674): ksk_a [in_dim*level][out_dim]
 *   (the `first` polynomials of ksk.keys, entry i*level + l), ksk_b
 *   [in_dim*level] (coefficient 0 of each `second` polynomial).  Any q >= 2.
 *   The result is the reference's, word for word: its running update
 *   r = (r + q - (digit * key) % q) % q in u64 arithmetic.  Below 2^63 that
 *   is -sum of the terms (nothing wraps after the raw body's first update);
 *   at q >= 2^63 the sum r + q - term wraps at 2^64 and the kernels make the
 *   update entry by entry, in the reference's order, wrap included.  A
 *   ciphertext without a non-zero digit keeps its body raw.
 * fhe_slot_extract_batch   the LWE ciphertext at ANY coefficient of an RLWE
 *   difference, the input of the encrypted comparisons (encryption.cpp
 *   :1112-1303 stop at "the difference, ready for PBS").  ct [batch][2][n] =
 *   (c0, c1); ref / ref_count as fhe_ct_square_batch (NULL / 0, one ciphertext
 *   for the whole batch, or one per ciphertext).  D = mod_sub(ct mod q, ref
 *   mod q) per word, or ct mod q without a reference; negate != 0: D =
 *   mod_sub(ref, ct), or -ct.  (D0, D1) is read as the GLWE with mask D1 and
 *   body D0.  For slot h = slots[s] (each below n; slots may repeat and nslots
 *   may exceed n): lwe_a [batch][nslots][n], lwe_a[j] = D1[h - j] for j <= h
 *   and (q - D1[n + h - j]) % q for j > h; lwe_b [batch][nslots] =
 *   (D0[h] + offsets[s] mod q) mod q.  Every output word is canonical.  These
 *   are, word for word, fhe_poly_sub_batch (or fhe_poly_neg_batch) on the
 *   reduced words, fhe_glwe_rotate_batch by -h, fhe_sample_extract_batch and a
 *   modular add on the body, in one launch that reads ct and ref once.  slots
 *   and offsets (any u64; NULL = zeros) are HOST arrays in both residences,
 *   copied before the call returns.  Every context: any n, any odd q < 2^64,
 *   either mode (no transform runs).  FHE_ERR_INVALID_ARG: a null ct, slots,
 *   lwe_a or lwe_b, nslots == 0, batch == 0, a ref_count other than 0, 1 or
 *   batch, "slot index out of range" for a slot >= n, an output that overlaps
 *   ct or ref.  A multi-device context splits the batch.
 * fhe_lwe_sum_batch        the sum of LWE ciphertexts of any dimension (no
 *   context): lwe_a [terms][batch][dim], lwe_b [terms][batch] -> out_a[c][j] =
 *   sum_t (a mod q) mod q, out_b[c] = (sum_t (b mod q) + body_offset mod q)
 *   mod q.  Any q >= 2 (nothing wraps at q >= 2^63), dim >= 0; terms == 0 or
 *   batch == 0: FHE_ERR_INVALID_ARG.  With the sign bootstrap (the constant
 *   test polynomial q / t / 2) it turns differences into encrypted bits:
 *   SIGN(x) + SIGN(-x) is [x == 0], SIGN(x) + q / t / 2 is [x >= 0].
 * fhe_lwe_pack_batch       the packing key switch, the way back from the TFHE
 *   side: nslots LWE ciphertexts per output ciphertext and nslots slot indices
 *   become ONE BFV ciphertext (c0, c1) whose phase c0 - c1 (*) sk has LWE s's
 *   message at coefficient slots[s].  (No reference counterpart: its compare_*
 *   never return from the LWE side.)  pack_key [in_dim*level][2][n], row
 *   e = i*level + l a pair (c0, c1); lwe_a [batch][nslots][in_dim]; lwe_b
 *   [batch][nslots]; slots a HOST array [nslots] in both residences, each
 *   below n, repeats allowed, copied before the call returns; out
 *   [batch][2][n].  With
 *     d(s,e)       = (lwe_a[c][s][i] >> ((level-1-l)*base_log)) & (2^base_log - 1)
 *                    on the raw mask word (key_switch's digit),
 *     term(s,e,p,j) = ((d * pack_key[e][p][j]) mod 2^64) mod q   (key_switch's
 *                    product),
 *     W_s[p][j]    = (-(sum_e term) + [p == 0 and j == 0] * (lwe_b[c][s] mod q))
 *                    mod q,   h = slots[s],
 *   out[c][p][j] = sum_s ( j >= h ? W_s[p][j-h] : (q - W_s[p][n+j-h]) % q )
 *                  (+ out[c][p][j] mod q when accumulate != 0)   mod q.
 *   The sum is the mathematical sum of canonical terms (no running update that
 *   could wrap); every output word is canonical; key, mask and body words may
 *   be any u64.  For q < 2^63 these are, word for word, per (c, s)
 *   fhe_key_switch_batch with out_dim = 2n (ksk_a = the pack key viewed as
 *   [in_dim*level][2n], ksk_b = zeros, body 0), a modular add of lwe_b mod q at
 *   coefficient 0 of the first half, fhe_glwe_rotate_batch (k = 1, mask = the
 *   second half, body = the first half) by +h, and fhe_ct_sum_batch over the
 *   slots (polys = 2) -- in one launch without the [batch*nslots][2n] rows.
 *   Every context: any n, any odd q < 2^64, either mode (no transform runs);
 *   base_log > 32, q >= 2^63 and moduli without the fast constants take a
 *   per-term kernel, as key switch does.  1 <= base_log <= 63 and
 *   (level-1)*base_log < 64, as for relinearisation; nslots * (in_dim*level
 *   + 1) < 2^31.  FHE_ERR_INVALID_ARG: a null pack_key, lwe_a, lwe_b, slots or
 *   out, nslots == 0, batch == 0, in_dim == 0 or level == 0, "slot index out
 *   of range" for a slot >= n, out overlapping an input.  Arguments are checked
 *   before the context is looked at.  FHE_HOST stages every buffer, the key
 *   included; a multi-device context splits the batch.  With in_dim = n and the
 *   ring key's coefficients as the LWE key the same call re-packs chosen slots
 *   of different ciphertexts (fhe_slot_extract_batch's outputs) into one.
 *   The key comes from fhe_pack_key_generate (below). */
int fhe_lwe_pack_batch(fhe_ctx *ctx, uint32_t base_log, uint32_t level, uint32_t in_dim, const uint64_t *pack_key,
                       const uint64_t *lwe_a, const uint64_t *lwe_b, const uint32_t *slots, size_t nslots,
                       int accumulate, uint64_t *out, size_t batch, int where);
int fhe_glwe_rotate_batch(fhe_ctx *ctx, uint32_t k, const int32_t *rot, const uint64_t *glwe, uint64_t *out,
                          size_t batch, int where);
int fhe_cmux_batch(fhe_ctx *ctx, uint32_t k, uint32_t base_log, uint32_t level, const uint64_t *ggsw_ntt,
                   const uint64_t *ct0, const uint64_t *ct1, uint64_t *out, size_t batch, int where);
int fhe_blind_rotate_batch(fhe_ctx *ctx, uint32_t k, uint32_t base_log, uint32_t level, uint32_t lwe_dim,
                           const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t lwe_q, const uint64_t *bsk_ntt,
                           uint64_t *acc, size_t batch, int where);
int fhe_sample_extract_batch(fhe_ctx *ctx, uint32_t k, const uint64_t *glwe, uint64_t *lwe_a, uint64_t *lwe_b,
                             size_t batch, int where);
/* Ciphertexts of this context's multi-CU blind rotations that were recomputed
 * by the repair pass since the context was created (a partner workgroup that
 * was not co-resident in time; see fhe_blind_rotate_batch).  Waits for the
 * context's stream.  No reference counterpart: blind_rotate
 * (bootstrap_engine.cpp:547-577) is a sequential CPU loop. */
int fhe_br_repair_count(fhe_ctx *ctx, uint64_t *count);
int fhe_key_switch_batch(uint64_t q, uint32_t base_log, uint32_t level, uint32_t in_dim, uint32_t out_dim,
                         const uint64_t *ksk_a, const uint64_t *ksk_b, const uint64_t *lwe_a, const uint64_t *lwe_b,
                         uint64_t *out_a, uint64_t *out_b, size_t batch, int where, int device, void *hip_stream);
int fhe_slot_extract_batch(fhe_ctx *ctx, const uint64_t *ct, const uint64_t *ref, size_t ref_count, int negate,
                           const uint32_t *slots, const uint64_t *offsets, size_t nslots, uint64_t *lwe_a,
                           uint64_t *lwe_b, size_t batch, int where);
int fhe_lwe_sum_batch(uint64_t q, uint32_t dim, const uint64_t *lwe_a, const uint64_t *lwe_b, size_t terms,
                      uint64_t body_offset, uint64_t *out_a, uint64_t *out_b, size_t batch, int where, int device,
                      void *hip_stream);

/* ---- EncryptionEngine encrypt / decrypt / add_plain (encryption.cpp) ----
 * The reference's RLWE encryption with its encoding: t = plaintext modulus
 * (0 selects 4, encryption.cpp:40-46), delta = q / t, a plaintext is n slot
 * values per ciphertext encoded as (v * delta mod 2^64) mod q
 * (encode_packed :117-131; encode_plaintext is the one-slot case).
 * fhe_secret_key_prepare  sk [n] (SecretKey::poly) -> sk_prep [2][n]
 *   (NTT-domain s and s^2; decrypt :256-271).
 * fhe_public_key_prepare  pk [2][n] = (a, b) (PublicKey, key_manager.h:70-76)
 *   -> pk_prep [2][n] (NTT-domain).
 *   Prepared keys are opaque to the caller: Montgomery form for the fused
 *   kernels (q < 2^62, n <= 16384), canonical rows for the composed path
 *   (q >= 2^62 or n > 16384); pass them back to the context that made them.
 * fhe_encrypt_batch  encrypt_internal (:171-205) with the sampled
 *   polynomials supplied (u ternary, e1, e2 error; [batch][n] each, any u64
 *   as x mod q), so the call is deterministic: ct [batch][2][n] =
 *   (pk.b u + e1 + m, pk.a u + e2) under the context's transform product.
 * fhe_decrypt_batch  decrypt / decrypt_packed (:234-348) of ciphertexts
 *   [batch][components][n] (2: (c0, c1); 3: degree-2 (c0, c1, c2)); is_ntt
 *   as Ciphertext::is_ntt.  Outputs (each nullable): values [batch][n] =
 *   round(p t / q) mod t per coefficient of the phase p = c0 - c1 s
 *   (- c2 s^2) (decode_packed :150-163; slot 0 is decode_plaintext),
 *   phase [batch][n], max_noise [batch] = the integer whose double is the
 *   reference's max_noise (compute_noise_budget :364-400); its noise
 *   budget is log2(q / (2 max(max_noise, 1))), negative = the reference's
 *   "Noise budget exhausted" failure.
 * fhe_add_plain_batch  add_plain (:638-665): out = (c0 + m, c1), m
 *   transformed first when is_ntt.
 * Every degree and modulus the context takes: one fused kernel per call for
 * q < 2^62 and n <= 16384, batched transforms plus elementwise passes
 * otherwise (engine_composed.hip). */
int fhe_secret_key_prepare(fhe_ctx *ctx, const uint64_t *sk, uint64_t *sk_prep, int where);
int fhe_public_key_prepare(fhe_ctx *ctx, const uint64_t *pk, uint64_t *pk_prep, int where);
int fhe_encrypt_batch(fhe_ctx *ctx, uint64_t t, const uint64_t *pk_prep, const uint64_t *values, const uint64_t *u,
                      const uint64_t *e1, const uint64_t *e2, uint64_t *ct, size_t batch, int where);
int fhe_decrypt_batch(fhe_ctx *ctx, uint64_t t, const uint64_t *sk_prep, const uint64_t *ct, uint32_t components,
                      int is_ntt, uint64_t *values, uint64_t *phase, uint64_t *max_noise, size_t batch, int where);
int fhe_add_plain_batch(fhe_ctx *ctx, uint64_t t, const uint64_t *ct, const uint64_t *values, int is_ntt,
                        uint64_t *out, size_t batch, int where);

/* ---- threshold decryption (key_manager.cpp:479-636) ----
 * A tally under a threshold key is opened by trustees: each computes a partial
 * decryption with a Shamir share of the secret key, and `threshold` partials
 * are combined and decoded.  Batched over ciphertexts [batch][2][n].
 * fhe_shamir_shares_batch  generate_threshold_keys' evaluation (:511-526):
 *   coeffs [threshold][n] (row 0 the master key, rows 1.. the random
 *   polynomials) -> shares [total][n],
 *   shares[i-1][j] = sum_k ((coeffs[k][j] mod q) (i^k mod q) mod q) mod q,
 *   i = 1..total.  1 <= threshold <= total, else FHE_ERR_INVALID_ARG "Invalid
 *   threshold parameters" (:484-486).
 * fhe_key_share_prepare  shares [count][n] -> shares_prep [count][n], the
 *   NTT-domain form partial decryption multiplies with.  Opaque, like sk_prep:
 *   pass it back to the context that made it.
 * fhe_partial_decrypt_batch  partial_decrypt (:584-601) of every ciphertext
 *   with every given share: partials [nshares][batch][n], partials[s][b] =
 *   c1_b * share_s in the ring -- the words of fhe_polymul_batch(c1, share).
 *   Only c1 is read.  nshares >= 1 and batch >= 1, else FHE_ERR_INVALID_ARG;
 *   partials must not overlap ct.
 * fhe_lagrange_coefficients  lagrange_coefficient (:548-582) on the host (no
 *   GPU): lambdas[i], i < used, for share_ids[i] over ALL `count` ids --
 *   numerator prod_{j != i} j mod q, denominator prod_{j != i} (j - i) mod q
 *   with the reference's signed subtraction, inverted by
 *   NTTProcessor::mod_inverse.  (combine_partial_decryptions interpolates over
 *   every supplied index and sums only the first `threshold` partials.)
 *   count == 0, used == 0 or used > count: FHE_ERR_INVALID_ARG; a zero id or
 *   two equal ids: FHE_ERR_INVALID_ARG "share ids must be distinct and
 *   non-zero" (the reference's denominator is 0 there).
 * fhe_combine_partials_batch  combine_partial_decryptions (:623-635) and the
 *   decryption it serves: partials [count][batch][n], one [batch][n] block per
 *   trustee; lambdas a HOST array of `count` words in both residences, copied
 *   before the call returns.  phase = c0 - sum_i partials[i] lambdas[i]: the
 *   words of fhe_poly_mul_scalar_batch and fhe_poly_add_batch per partial,
 *   then fhe_poly_sub_batch(c0, .).  values [batch][n], phase [batch][n] and
 *   max_noise [batch] (each nullable, at least one given) are what
 *   fhe_decrypt_batch gives for that phase; t == 0 selects 4.  Only c0 is
 *   read.  count == 0: FHE_ERR_INVALID_ARG.
 * On a multi-device context the batch is split into contiguous ranges; every
 * device takes all shares / all partials of its range. */
int fhe_shamir_shares_batch(fhe_ctx *ctx, const uint64_t *coeffs, uint32_t threshold, uint32_t total,
                            uint64_t *shares, int where);
int fhe_key_share_prepare(fhe_ctx *ctx, const uint64_t *shares, uint64_t *shares_prep, size_t count, int where);
int fhe_partial_decrypt_batch(fhe_ctx *ctx, const uint64_t *shares_prep, size_t nshares, const uint64_t *ct,
                              uint64_t *partials, size_t batch, int where);
int fhe_lagrange_coefficients(uint64_t q, const uint32_t *share_ids, size_t count, size_t used, uint64_t *lambdas);
int fhe_combine_partials_batch(fhe_ctx *ctx, uint64_t t, const uint64_t *ct, const uint64_t *partials,
                               const uint64_t *lambdas, size_t count, uint64_t *values, uint64_t *phase,
                               uint64_t *max_noise, size_t batch, int where);

/* ---- BootstrapEngine::bootstrap_with_test_poly (bootstrap_engine.cpp:684-708)
 * For each LWE ciphertext c (lwe_a [batch][lwe_dim], lwe_b [batch] mod
 * lwe_q): acc = (0, .., 0, test_poly), blind_rotate (as
 * fhe_blind_rotate_batch), sample_extract, then key_switch modulo the GLWE
 * modulus with ksk_a [k*n*ks_level][out_dim], ksk_b [k*n*ks_level] (as
 * fhe_key_switch_batch): out_a [batch][out_dim], out_b [batch].
 * bootstrap() is the identity test polynomial; programmable_bootstrap
 * (:716-722) passes a lookup table's polynomial. */
int fhe_bootstrap_batch(fhe_ctx *ctx, uint32_t k, uint32_t base_log, uint32_t level, uint32_t lwe_dim,
                        const uint64_t *lwe_a, const uint64_t *lwe_b, uint64_t lwe_q, const uint64_t *bsk_ntt,
                        const uint64_t *test_poly, uint32_t ks_base_log, uint32_t ks_level, uint32_t out_dim,
                        const uint64_t *ksk_a, const uint64_t *ksk_b, uint64_t *out_a, uint64_t *out_b, size_t batch,
                        int where);

/* ---- device randomness and key material (key_manager.cpp, bootstrap_engine.cpp)
 * SecureRandom's draws (key_manager.cpp:53-115) come from a ChaCha20
 * keystream (RFC 8439 block function) keyed by seed[4] (256 bits, little-
 * endian words), with the 64-bit `stream` as the nonce: element i of a
 * stream of `count` elements draws from blocks i, i + count, i + 2 count, ..
 * (8 u64 words per block, in order).  The same (seed, stream, count) gives
 * the same values on every device and in the CPU oracle (oracle_sample), so
 * keys and encryptions are reproducible; the engine seeds from the OS CSPRNG.
 *   FHE_SAMPLE_UNIFORM   random_u64_range(q): rejection below (2^64 - q) % q, then % q (:60-71)
 *   FHE_SAMPLE_TERNARY   sample_ternary: range(3) -> {q-1, 0, 1} (:73-83)
 *   FHE_SAMPLE_GAUSSIAN  sample_gaussian(std_dev, q): Box-Muller on two 53-bit
 *                        uniforms, std::round, negatives as q + x (:85-110)
 *   FHE_SAMPLE_BINARY    sample_binary: random_u64() & 1
 *   FHE_SAMPLE_RAW       random_u64()
 * q is the context modulus.  Every keygen entry point names the streams it
 * takes; results follow the reference formulas under the context's
 * transform product (*).
 * fhe_encrypt_sampled_batch   encrypt_internal (encryption.cpp:171-205) with
 *   u ternary (stream), e1 (stream + 1), e2 (stream + 2) error, [batch][n]
 *   each; otherwise as fhe_encrypt_batch.
 * fhe_public_key_generate     generate_public_key (key_manager.cpp:218-246):
 *   pk [2][n] = (a, a (*) s + e), a uniform (stream), e error (stream + 1).
 * fhe_eval_key_generate       generate_eval_key (:252-333): rlk [level][2][n],
 *   a_l uniform (stream + 2l), e_l error (stream + 2l + 1),
 *   b_l = a_l (*) s + e_l + (s (*) s) * power_l, power_0 = 1,
 *   power_{l+1} = (power_l * 2^base_log) % q in u64 arithmetic (as the reference).
 * fhe_switch_key_generate     the key of fhe_ct_galois_batch and
 *   fhe_ct_trace_batch: swk [level][2][n] = (a_l, b_l) in the layout, with the
 *   draws (a_l uniform on stream + 2l, e_l Gaussian on stream + 2l + 1) and the
 *   u64 power update of fhe_eval_key_generate;
 *   b_l = a_l (*) sk_to + e_l + m * power_l, m[j] = (q - sigma_g(sk_from)[j]) % q:
 *   the NEGATED source key, so that the unsigned digits of sigma_g(c1) give the
 *   phase c0 - c1 (*) s without negating c1.  The words equal fhe_sample_batch
 *   twice, fhe_polymul_batch against sk_to, fhe_poly_add_batch,
 *   fhe_poly_galois_batch + fhe_poly_neg_batch on sk_from,
 *   fhe_poly_mul_scalar_batch by power_l % q and fhe_poly_add_batch, bit for
 *   bit.  sk_from == sk_to with g != 1 is a Galois key; g = 1 with two
 *   different keys is a re-keying key.  It is prepared with
 *   fhe_relin_key_prepare (same shape, same opaque form).  Errors as
 *   fhe_eval_key_generate, plus "Galois element must be odd" (before the
 *   context is looked at), "Galois element out of range" and swk overlapping
 *   either key; level == 0 returns FHE_OK and writes nothing.
 * fhe_ggsw_encrypt_batch      encrypt_ggsw (bootstrap_engine.cpp:268-306) of
 *   count values (the LWE key of a bootstrapping key, :308-360): out
 *   [count][(k+1)*level][k+1][n] coefficient form, row (row, l) an
 *   encrypt_glwe_zero (:190-227; masks uniform (stream), error (stream + 1),
 *   body = sum_i mask_i (*) s + e) plus (|v| q) >> ((l+1) base_log) (negated
 *   mod q for v < 0) on coefficient 0 of mask `row` (row < k) or the body.
 * fhe_ksk_generate            generate_key_switch_key (:367-420): entry
 *   e = i*level + l (i < n_in, the GLWE key coefficients glwe_sk[i]):
 *   ksk_a [entries][lwe_dim] uniform (stream), error (stream + 1; std_dev 0
 *   selects 3.2), ksk_b[e] = ((u64)((<a_e, lwe_sk> + e) % (int64)q)
 *   + (glwe_sk[i] q) >> ((l+1) base_log)) % q with the reference's int64 /
 *   u64 wrap-around.  Shift counts >= 64 take the count mod 64.
 * fhe_pack_key_generate       the key of fhe_lwe_pack_batch: rows =
 *   lwe_dim*level RLWE encryptions under the ring key sk [n] of the LWE key
 *   lwe_sk [lwe_dim] times the gadget powers; pack_key [rows][2][n], row
 *   e = i*level + l = (c0, c1).  c1 = fhe_sample_batch(UNIFORM, seed, stream,
 *   rows*n) read as [rows][n]; err the same with GAUSSIAN and stream + 1
 *   (std_dev 0 selects 3.2, as fhe_ksk_generate); c0[e] = c1[e] (*) sk +
 *   err[e] under the context's transform product, plus m_e on coefficient 0,
 *   m_e = (|lwe_sk[i]| mod q) * (2^((level-1-l)*base_log) mod q) mod q,
 *   negated mod q for lwe_sk[i] < 0.  That power is the one the pack's digit
 *   (a >> ((level-1-l)*base_log)) & (2^base_log - 1) multiplies -- NOT the
 *   q >> ((l+1) base_log) of fhe_ksk_generate -- so with level*base_log >= the
 *   bit length of q - 1 the digits recompose the mask word exactly and the
 *   packed ciphertext decrypts: c0 - c1 (*) sk = X^h (b - <a, lwe_sk>) plus
 *   the digit-weighted key errors.  The words equal fhe_sample_batch twice,
 *   fhe_polymul_batch against the broadcast key, fhe_poly_add_batch and the
 *   gadget add.  1 <= base_log <= 63, (level-1)*base_log < 64.  Slots other
 *   than 0 decrypt only under FHE_MODE_NEGACYCLIC: compat mode's transform
 *   product does not commute with the monomial X^h.  Slot 0 decrypts in both
 *   modes.
 * fhe_lwe_decrypt_batch      LWE decryption under an integer key s [dim]:
 *   phase = b - sum_j a_j s_j (mod q), values = round(phase t / q) mod t
 *   (decode_plaintext's rounding, encryption.cpp:133-148).  Each output
 *   nullable. */
#define FHE_SAMPLE_UNIFORM 0
#define FHE_SAMPLE_TERNARY 1
#define FHE_SAMPLE_GAUSSIAN 2
#define FHE_SAMPLE_BINARY 3
#define FHE_SAMPLE_RAW 4
int fhe_sample_batch(fhe_ctx *ctx, int kind, const uint64_t seed[4], uint64_t stream, double std_dev, uint64_t *out,
                     size_t count, int where);
int fhe_encrypt_sampled_batch(fhe_ctx *ctx, uint64_t t, const uint64_t *pk_prep, const uint64_t *values,
                              const uint64_t seed[4], uint64_t stream, double std_dev, uint64_t *ct, size_t batch,
                              int where);
int fhe_public_key_generate(fhe_ctx *ctx, const uint64_t *sk, const uint64_t seed[4], uint64_t stream, double std_dev,
                            uint64_t *pk, int where);
int fhe_eval_key_generate(fhe_ctx *ctx, const uint64_t *sk, uint32_t base_log, uint32_t level, const uint64_t seed[4],
                          uint64_t stream, double std_dev, uint64_t *rlk, int where);
int fhe_switch_key_generate(fhe_ctx *ctx, const uint64_t *sk_to, const uint64_t *sk_from, uint32_t g, uint32_t base_log,
                            uint32_t level, const uint64_t seed[4], uint64_t stream, double std_dev, uint64_t *swk,
                            int where);
int fhe_ggsw_encrypt_batch(fhe_ctx *ctx, uint32_t k, uint32_t base_log, uint32_t level, const int64_t *values,
                           size_t count, const uint64_t *sk, const uint64_t seed[4], uint64_t stream, double std_dev,
                           uint64_t *out, int where);
int fhe_ksk_generate(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *glwe_sk, uint32_t n_in,
                     const int64_t *lwe_sk, uint32_t lwe_dim, const uint64_t seed[4], uint64_t stream, double std_dev,
                     uint64_t *ksk_a, uint64_t *ksk_b, int where);
int fhe_pack_key_generate(fhe_ctx *ctx, uint32_t base_log, uint32_t level, const uint64_t *sk, const int64_t *lwe_sk,
                          uint32_t lwe_dim, const uint64_t seed[4], uint64_t stream, double std_dev,
                          uint64_t *pack_key, int where);
int fhe_lwe_decrypt_batch(uint64_t q, uint64_t t, const int64_t *sk, uint32_t dim, const uint64_t *lwe_a,
                          const uint64_t *lwe_b, uint64_t *values, uint64_t *phase, size_t batch, int where,
                          int device, void *hip_stream);

/* ---- context-free modular kernels --------------------------------------- */
/* BarrettReducer::barrett_mul contract (modular_arithmetic.cpp:268-280):
 * c[i] = a[i]*b[i] mod q for any u64 inputs, any q != 0. stream may be NULL. */
int fhe_modmul_batch(uint64_t q, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t count, int where,
                     int device, void *hip_stream);
/* MultiLimbModularArithmetic (2 limbs, modular_arithmetic.cpp:471-625).
 * q[2] little-endian limbs; a, b, c: count elements of 2 limbs each. */
int fhe_ml_constants(const uint64_t q[2], uint64_t out[7]); /* q0,q1,r0,r1,r2_0,r2_1,q_inv */
int fhe_ml_montmul_batch(const uint64_t q[2], const uint64_t *a, const uint64_t *b, uint64_t *c, size_t count,
                         int where, int device, void *hip_stream);

/* ---- N-API ModularArithmetic class (index.d.ts:32-44, lib.rs:42-121) -----
 * Scalar host functions with the reference's exact constants, including
 * q_inv = -(q^-1 mod (2^64-1)) (modular_arithmetic.cpp:69).  consts[4] =
 * {q, R mod q, R^2 mod q, q_inv}.                                            */
int fhe_mont_constants_compat(uint64_t q, uint64_t consts[4]);
uint64_t fhe_compat_montgomery_mul(const uint64_t consts[4], uint64_t a, uint64_t b);
uint64_t fhe_compat_to_montgomery(const uint64_t consts[4], uint64_t a);
uint64_t fhe_compat_from_montgomery(const uint64_t consts[4], uint64_t a);
uint64_t fhe_compat_mod_add(uint64_t q, uint64_t a, uint64_t b);
uint64_t fhe_compat_mod_sub(uint64_t q, uint64_t a, uint64_t b);

/* ---- context-owned device memory (resident ciphertexts and keys) -------
 * fhe_ctx_alloc / fhe_ctx_free: stream-ordered allocations on the context's
 * (first) device: a free is ordered after the work already enqueued on the
 * context stream, and the device pool keeps the memory warm (no device
 * synchronisation per call).  fhe_ctx_memcpy copies on the context stream:
 * FHE_COPY_H2D / FHE_COPY_D2H return when the copy is done (ordered after the
 * context's earlier work), FHE_COPY_D2D is enqueued. */
#define FHE_COPY_H2D 0
#define FHE_COPY_D2H 1
#define FHE_COPY_D2D 2
int fhe_ctx_alloc(fhe_ctx *ctx, size_t bytes, void **out);
int fhe_ctx_free(fhe_ctx *ctx, void *ptr);
int fhe_ctx_memcpy(fhe_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);

/* ---- device memory helpers (for callers without their own allocator) --- */
int fhe_dev_alloc(int device, size_t bytes, void **out);
int fhe_dev_free(void *ptr);
int fhe_memcpy_h2d(void *dst, const void *src, size_t bytes);
int fhe_memcpy_d2h(void *dst, const void *src, size_t bytes);
int fhe_device_synchronize(int device);

/* Event timing on a stream (used by bench.py for HIP-event kernel timing). */
int fhe_event_create(void **ev);
int fhe_event_destroy(void *ev);
int fhe_event_record(void *ev, void *hip_stream);
int fhe_event_elapsed_ms(void *start, void *stop, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* FHE_GPU_H */
