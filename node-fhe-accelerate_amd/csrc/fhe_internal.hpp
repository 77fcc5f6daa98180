// fhe_internal.hpp -- interface between the host C-ABI (fhe_gpu.cpp) and the
// kernel translation units.  Not installed; no torch types anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "ntt_core.hpp"

namespace FHE_NS {

// Orders every use of a context's big-N scratch (Plan::big_scratch): the
// launch sequence of one two-pass transform is enqueued under `mu`, and a
// sequence on another stream first waits for `done`, the completion of the
// previous one.  Host threads and streams (the staging slots, async N-API
// jobs, a caller's own stream) may then share one context.
struct BigSync {
    std::mutex mu;
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
};

// Moduli 2^62 <= q < 2^64 (ntt_wide.hip): canonical arithmetic, twiddles in
// Montgomery form (w 2^64 mod q), stage-major like NttArgs' tables.
struct WideArgs {
    const uint64_t *twf, *twi;
    uint64_t q, qinv, mu;   // qinv = -q^-1 mod 2^64, mu = floor(2^64 / q)
    uint64_t r2;            // 2^128 mod q
    uint64_t ninv_m;        // N^-1 2^64 mod q
    uint64_t ninv_r2;       // N^-1 2^128 mod q (after a Montgomery pointwise product)
};

struct Plan {
    uint32_t logn;
    int word;   // 32 or 64
    int wide;   // q >= 2^62: every transform takes ntt_wide.hip
    int lazy;   // 32-bit path with (4 + 2L) q <= 2^32: forward stages skip reductions
    int compat; // compat-mode tables (unit twiddle in pass 0): hot kernels take gk_compat keys
    int cus;    // compute units of the context's device (persistent grids)
    hipStream_t stream;
    // N > 2^kMaxFusedLogN (ntt_big.hip): two chunk-sized scratch buffers
    uint64_t *big_scratch[2];
    size_t big_chunk;  // polynomials per scratch chunk
    BigSync *big_sync; // owned by the context
    NttArgs<uint32_t> a32;
    NttArgs<uint64_t> a64;
    WideArgs wa;  // wide != 0
};

constexpr int kMinLogN = 2;
constexpr int kMaxFusedLogN = 14;  // one workgroup per polynomial up to here
constexpr int kMaxLogN = 16;       // NTTProcessor's limit (ntt_processor.cpp:146)

// Forward NTT; epi 0: canonical output, 1: output * R mod q (Montgomery
// form, used to prepare GGSW keys).
hipError_t launch_fwd(const Plan &p, const uint64_t *in, uint64_t *out, size_t batch, int epi);
hipError_t launch_inv(const Plan &p, const uint64_t *in, uint64_t *out, size_t batch);
// out = fwd(a) (.) w  (config C3: NTT + modmul)
hipError_t launch_fwd_mul(const Plan &p, const uint64_t *a, const uint64_t *w, uint64_t *out, size_t batch);
// c = inv(fwd(a) (.) fwd(b))  (PolynomialRing::multiply)
hipError_t launch_polymul(const Plan &p, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch);
// RNS ring in one launch (grid.y = limb): `limbs` contiguous [batch][N]
// blocks, limb l with the transform constants tab[l] (a device array of
// NttArgs<uint32_t> or NttArgs<uint64_t> per p.word); every limb shares p's
// degree, word and laziness.  inv_limbs: inverse (b == nullptr) or polymul.
hipError_t launch_fwd_limbs(const Plan &p, const void *tab, int limbs, const uint64_t *in, uint64_t *out,
                            size_t batch);
hipError_t launch_inv_limbs(const Plan &p, const void *tab, int limbs, const uint64_t *a, const uint64_t *b,
                            uint64_t *c, size_t batch);
// q >= 2^62 (Plan::wide), any N: op as launch_big
hipError_t launch_wide(const Plan &p, int op, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch);
// N > 2^kMaxFusedLogN: op 0 fwd, 1 fwd*R, 2 fwd (.) b, 3 inv, 4 polymul
hipError_t launch_big(const Plan &p, int op, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t batch);
// TFHE external product, GGSW already in NTT-Montgomery form.
hipError_t launch_extprod(const Plan &p, int k1, int level, int base_log, const uint64_t *glwe,
                          const uint64_t *ggsw, uint64_t *out, size_t batch);
// Several decomposition levels at N = 16384, 64-bit words, k1 == 2,
// base_log <= 31 (ntt_ext2.hip): accumulators in VGPRs, one HBM pass.
bool extprod_acc_supported(const Plan &p, int k1, int level, int base_log);
hipError_t launch_extprod_acc(const Plan &p, int level, int base_log, const uint64_t *glwe, const uint64_t *ggsw,
                              uint64_t *out, size_t batch);

// Relinearisation (EncryptionEngine::relinearize): ct3 [batch][3][n],
// rlk [level][2][n] (a_l, b_l) in NTT-Montgomery form -> out [batch][2][n].
hipError_t launch_relin(const Plan &p, int level, int base_log, const uint64_t *ct3, const uint64_t *rlk,
                        uint64_t *out, size_t batch);
// Galois key switch of degree-1 ciphertexts (fhe_ct_galois_batch; k_dmac
// MODE 4): ct [batch][2][n], swk [level][2][n] (a_l, b_l) in NTT-Montgomery
// form, ginv = g^-1 mod 2n -> out [batch][2][n]; level >= 1, the fused family
// only (n <= 16384, q < 2^62).
hipError_t launch_ct_galois(const Plan &p, int level, int base_log, uint32_t ginv, int add_input, const uint64_t *ct,
                            const uint64_t *swk, uint64_t *out, size_t batch);
// One blind-rotation CMux step over a batch of GLWE accumulators (ping-pong
// buffers acc_in -> acc_out); step = LWE mask index i, bsk[i] = ggsw.
hipError_t launch_cmux_rotate(const Plan &p, int k1, int level, int base_log, const uint64_t *acc_in,
                              const uint64_t *ggsw, uint64_t *acc_out, size_t batch, const uint64_t *lwe_a,
                              uint32_t lwe_dim, uint32_t step, uint64_t lwe_q);
// The whole blind rotation (initial X^-round(b 2N/q) rotation + lwe_dim
// CMux steps) of a small batch in ONE launch (ntt_br.hip): one workgroup per
// ciphertext, accumulators resident in LDS across all steps.  k1 == 2 and
// 512 <= N <= 2048 only (br_persist_supported); acc is updated in place.
bool br_persist_supported(const Plan &p, int k1);
// k = 1 on two CUs per ciphertext (N = 1024..4096, grid 16 ceil(batch / 8)
// <= CUs); scratch: br_pair_scratch_bytes (flags zeroed by the launch).  A
// workgroup whose partner does not answer within timeout_ticks (100 MHz)
// gives up on its ciphertext; the launch is followed by a repair pass
// (k_br_persist) over the given-up ciphertexts, each counted in *repairs.
// With multi set, levels 2 / 3 at small batches take 2 level CUs per
// ciphertext instead (k_br_multi; br_multi_members), same protocol and repair.
struct BrPairOpts {
    uint64_t timeout_ticks;
    bool coop;                     // hipLaunchCooperativeKernel (grid checked against occupancy)
    unsigned long long *repairs;   // device counter
    bool multi;                    // k_br_multi where br_multi_members > 0
};
bool br_pair_supported(const Plan &p, int k1, size_t batch);
int br_multi_members(const Plan &p, int level, size_t batch);
size_t br_pair_scratch_bytes(const Plan &p, size_t batch, int level, bool multi);
hipError_t launch_br_pair(const Plan &p, int level, int base_log, uint64_t *acc, const uint64_t *bsk,
                          const uint64_t *lwe_a, const uint64_t *lwe_b, uint32_t lwe_dim, uint64_t lwe_q, size_t batch,
                          void *scratch, const BrPairOpts &o);
hipError_t launch_br_persist(const Plan &p, int k1, int level, int base_log, uint64_t *acc, const uint64_t *bsk,
                             const uint64_t *lwe_a, const uint64_t *lwe_b, uint32_t lwe_dim, uint64_t lwe_q,
                             size_t batch);
// CMux(ggsw, ct0, ct1) = ct0 + ggsw (x) (ct1 - ct0)
hipError_t launch_cmux(const Plan &p, int k1, int level, int base_log, const uint64_t *ggsw, const uint64_t *ct0,
                       const uint64_t *ct1, uint64_t *out, size_t batch);
// Ciphertext multiply (coefficient form): x, y [batch][2][n] -> out [batch][3][n]
hipError_t launch_ct_mul(const Plan &p, const uint64_t *x, const uint64_t *y, uint64_t *out, size_t batch);
// Ciphertext square (ct_square.hip, coefficient form, the fused family only):
// out[i] = multiply(d, d) with d = ct[i], or ct[i] - ref[i ref_stride / 2n]
// when ref != nullptr (ref_stride in words: 0 shares one ref, 2 n is one per
// ciphertext).  ct [batch][2][n] -> out [batch][3][n].
hipError_t launch_ct_square(const Plan &p, const uint64_t *ct, const uint64_t *ref, size_t ref_stride, uint64_t *out,
                            size_t batch);

// EncryptionEngine encrypt / decrypt / add_plain (ntt_engine.hip); keys
// prepared NTT x R (Montgomery form): pk_prep (pk.a, pk.b), sk_prep (s, s^2).
// t = plaintext modulus (0 -> 4).  decrypt: phase [batch][n] is required for
// comps == 3 on coefficient-form ciphertexts (the partial phase lives there);
// store_phase selects whether the final phase is written.
hipError_t launch_encrypt(const Plan &p, uint64_t t, const uint64_t *pk_prep, const uint64_t *vals,
                          const uint64_t *u, const uint64_t *e1, const uint64_t *e2, uint64_t *ct, size_t batch);
hipError_t launch_decrypt(const Plan &p, uint64_t t, const uint64_t *sk_prep, const uint64_t *ct, int comps,
                          int is_ntt, uint64_t *phase, int store_phase, uint64_t *dec, uint64_t *noise, size_t batch);
hipError_t launch_add_plain(const Plan &p, uint64_t t, const uint64_t *ct, const uint64_t *vals, int is_ntt,
                            uint64_t *out, size_t batch);
// Composed encrypt / decrypt / add_plain (engine_composed.hip) for q >= 2^62
// and N > 16384: elementwise finishing passes around batched transforms.
hipError_t launch_enc_finish(uint64_t q, uint64_t t, const uint64_t *t0, const uint64_t *t1, const uint64_t *e1,
                             const uint64_t *e2, const uint64_t *vals, uint64_t *ct, uint32_t n, size_t batch,
                             hipStream_t s);
hipError_t launch_sub_row(uint64_t q, const uint64_t *src, uint32_t comps, const uint64_t *x, uint64_t *out, uint32_t n,
                          size_t batch, hipStream_t s);
hipError_t launch_decode(uint64_t q, uint64_t t, const uint64_t *phase, uint64_t *dec, uint64_t *noise, uint32_t n,
                         size_t batch, hipStream_t s);
hipError_t launch_add_plain_fin(uint64_t q, const uint64_t *ct, const uint64_t *f, uint64_t *out, uint32_t n, size_t batch,
                                hipStream_t s);
hipError_t launch_encode(uint64_t q, uint64_t t, const uint64_t *vals, uint64_t *out, size_t count, hipStream_t s);
// acc [batch][k1][n] = (0, .., 0, test_poly): bootstrap's accumulator
hipError_t launch_glwe_init(const uint64_t *test_poly, uint64_t *acc, uint32_t n, uint32_t k1, size_t batch,
                            hipStream_t s);

// Elementwise kernels (elementwise.hip).
struct ModConsts {
    uint64_t q, mu, qinv, r2;  // mu = floor(2^64/q); Montgomery R = 2^64
    int fast;                  // q odd and q < 2^63
};
// Composed TFHE / BFV paths (k > 1, N > 16384): key MAC of NTT-domain
// digits, relinearisation digits, row-wise mod_add.
hipError_t launch_mac_keys(const ModConsts &m, int word, const uint64_t *x, const uint64_t *g, uint64_t *out,
                           uint32_t n, size_t batch, uint32_t rows, uint32_t k1, int swap, hipStream_t s);
hipError_t launch_relin_digits(const uint64_t *ct3, uint64_t *out, uint32_t n, size_t batch, uint32_t base_log,
                               uint32_t level, hipStream_t s);
hipError_t launch_add_rows(const ModConsts &m, uint64_t *out, const uint64_t *src, uint32_t n, size_t batch,
                           uint32_t rows, uint32_t src_rows, hipStream_t s);
hipError_t launch_modmul(const ModConsts &m, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t n,
                         hipStream_t s);
hipError_t launch_addsub(const ModConsts &m, const uint64_t *a, const uint64_t *b, uint64_t *c, size_t n, int sub,
                         hipStream_t s);
hipError_t launch_neg(uint64_t q, const uint64_t *a, uint64_t *c, size_t n, hipStream_t s);
// sigma_g of npoly rows (galois.hip): out + i out_pitch = sigma_g(in + i
// in_pitch) (+ add + i in_pitch, mod q, when add != nullptr); ginv = g^-1 mod
// 2n, n = 2^logn >= 4, pitches in words (even), 16-byte aligned rows.
hipError_t launch_poly_galois(const ModConsts &m, uint32_t logn, uint32_t ginv, const uint64_t *in, const uint64_t *add,
                              uint64_t *out, size_t npoly, size_t in_pitch, size_t out_pitch, hipStream_t s);
// RNS ring: pointwise product (op 0), add (1), sub (2) over [limbs][per] with
// per-limb constants tab[limb] (device array), one launch.
hipError_t launch_ew_limbs(const ModConsts *tab, int limbs, const uint64_t *a, const uint64_t *b, uint64_t *c,
                           size_t per, int op, hipStream_t s);
hipError_t launch_mul_scalar(const ModConsts &m, const uint64_t *a, uint64_t sc, uint64_t sc_shoup, uint64_t *c,
                             size_t n, hipStream_t s);
hipError_t launch_ml_montmul(const uint64_t consts[7], const uint64_t *a, const uint64_t *b, uint64_t *c, size_t n,
                             hipStream_t s);
// Segmented ciphertext sum (tally.hip): one pass of k_ct_sum.  src is
// [groups][count][words] u64, or with ptr_table a device array of `count`
// pointers to `words` u64 each (16-byte aligned, groups == 1).  Slice y of
// `slices` sums ballots [y per, min(count, (y+1) per)) into row y of
// out [groups][slices][words]; accumulate (slices == 1 only) reads out as one
// more term.  words even, q odd.
hipError_t launch_ct_sum(const ModConsts &m, const void *src, bool ptr_table, uint64_t *out, size_t words, size_t count,
                         size_t per, size_t slices, size_t groups, int accumulate, hipStream_t s);
// The slice range every sliced launch (tally, dot, dot_plain) accepts: 1 to
// max_slices slices of `per` units that cover `count` with none empty; a
// pointer table addresses one group.
inline bool slices_ok(size_t count, size_t per, size_t slices, size_t groups, bool ptr_table, size_t max_slices) {
    return per != 0 && slices != 0 && slices <= max_slices && (slices - 1) * per < count && slices * per >= count &&
           !(ptr_table && groups != 1);
}
// Scaled ciphertext sum (tally.hip k_ct_sum_scaled): launch_ct_sum with ballot
// i of group g multiplied by the scalar of table entry tab[g count + i] (16
// bytes each, device memory).  launch_scalar_prep fills `total` entries from
// raw u64 scalars on the device; scalar_entry is the same map on the host.
hipError_t launch_scalar_prep(const ModConsts &m, const uint64_t *raw, void *tab, size_t total, hipStream_t s);
hipError_t launch_ct_sum_scaled(const ModConsts &m, const void *src, bool ptr_table, const void *tab, uint64_t *out,
                                size_t words, size_t count, size_t per, size_t slices, size_t groups, int accumulate,
                                hipStream_t s);
inline void scalar_entry(uint64_t raw, uint64_t q, uint64_t e[2]) {
    const unsigned __int128 s = raw % q;
    e[0] = (q >> 63) ? (uint64_t)((s << 64) % q) : (uint64_t)s;
    e[1] = (q >> 63) ? 0 : (uint64_t)((s << 64) / q);
}
// Threshold decryption (threshold.hip; key_manager.cpp:479-636).
// launch_partial_dec: partials[s][b] = inv(fwd(c1_b) (.) shares_prep[s]) for
// ct [batch][2][n] (c1 read in place) and prepared rows [nshares][n] (NTT x R);
// block s of the output starts at partials + s share_stride.  The fused family
// only (n <= 16384, q < 2^62).
hipError_t launch_partial_dec(const Plan &p, const uint64_t *shares_prep, size_t nshares, const uint64_t *ct,
                              uint64_t *partials, size_t share_stride, size_t batch);
// launch_combine_partials: phase = c0 - sum_i partials[i] lambda_i, decoded as
// k_decode does; block i of the partials starts at partials + i share_stride.
// Up to kCombineInlineLambdas partials take `lambdas`, the raw HOST words
// (they travel as kernel arguments, lam unused); more take lam, a device table
// of `count` scalar_entry pairs (launch_scalar_table).  values, phase and
// max_noise are each nullable (max_noise is zeroed by the launch).  Any n >=
// 2 that is a power of two, any odd q.
constexpr int kCombineInlineLambdas = 16;
hipError_t launch_combine_partials(const ModConsts &m, uint64_t t, const uint64_t *ct, const uint64_t *partials,
                                   size_t share_stride, const uint64_t *lambdas, const void *lam, size_t count,
                                   uint64_t *values, uint64_t *phase, uint64_t *max_noise, uint32_t n, size_t batch,
                                   hipStream_t s);
// launch_scalar_table: `count` HOST scalars to a device table of scalar_entry
// pairs.  The entries travel as kernel arguments, so the host array is free
// when the call returns and nothing is synchronised.
hipError_t launch_scalar_table(uint64_t q, const uint64_t *raw, size_t count, void *tab, hipStream_t s);
// launch_shamir_shares: shares[i - 1] = sum_k coeffs[k] i^k, i = 1..total;
// pts is a device table of `total` scalar_entry pairs of the points 1..total.
hipError_t launch_shamir_shares(const ModConsts &m, const uint64_t *coeffs, uint32_t threshold, uint32_t total,
                                const void *pts, uint64_t *shares, size_t n, hipStream_t s);
// Ciphertext inner product with public plaintext polynomials (dot_plain.hip):
// cts [groups][count][2][n], pts [groups][count][n], or with ptr_table device
// arrays of `count` pointers each (groups == 1); slices as launch_ct_dot, rows
// dst [groups][slices][2][n], canonical.  The fused family only (n <= 16384,
// q < 2^62).  is_ntt: the ciphertexts and the rows are NTT-domain, no
// workspace.  Otherwise a workspace of ct_dot_plain_ws_bytes.
size_t ct_dot_plain_resident(const Plan &p, int is_ntt);
size_t ct_dot_plain_ws_bytes(const Plan &p, size_t slices, size_t groups);
hipError_t launch_ct_dot_plain(const Plan &p, const void *cts, const void *pts, bool ptr_table, void *ws, uint64_t *dst,
                               size_t count, size_t per, size_t slices, size_t groups, int is_ntt);
// Ciphertext inner product (dot.hip).  a, b are [groups][count][2][n] u64, or
// with ptr_table device arrays of `count` pointers to 2 n u64 each (groups ==
// 1).  Slice y of `slices` covers pairs [y per, min(count, (y+1) per)) and
// writes row y of dst [groups][slices][3][n], canonical; launch_ct_sum folds
// the rows.  launch_ct_dot: coefficient form, the fused family only (n <=
// 16384, q < 2^62), with a workspace of ct_dot_ws_bytes; ct_dot_resident is
// the number of slices one launch keeps resident; by_component runs three
// workgroups per slice, one per component of the sum.  launch_ct_dot_ntt:
// NTT-domain inputs, any n and odd q, 16-byte aligned buffers.
size_t ct_dot_resident(const Plan &p);
size_t ct_dot_ws_bytes(const Plan &p, size_t slices, size_t groups);
hipError_t launch_ct_dot(const Plan &p, const void *a, const void *b, bool ptr_table, void *ws, uint64_t *dst,
                         size_t count, size_t per, size_t slices, size_t groups, bool by_component);
hipError_t launch_ct_dot_ntt(const ModConsts &m, const void *a, const void *b, bool ptr_table, uint64_t *dst, uint32_t n,
                             size_t count, size_t per, size_t slices, size_t groups, hipStream_t s);
// Tensor product of NTT-form ciphertexts: x, y [batch][2][n] -> [batch][3][n]
hipError_t launch_tensor_ntt(const ModConsts &m, const uint64_t *x, const uint64_t *y, uint64_t *out, uint32_t n,
                             size_t batch, hipStream_t s);
// Square of NTT-form ciphertexts, of x - ref when ref != nullptr (ref_stride
// in words, 0 shares one ref): x [batch][2][n] -> [batch][3][n]; n even and
// 16-byte aligned buffers, hipErrorInvalidValue otherwise.
hipError_t launch_square_ntt(const ModConsts &m, const uint64_t *x, const uint64_t *ref, size_t ref_stride,
                             uint64_t *out, uint32_t n, size_t batch, hipStream_t s);
// GLWE rotation by X^r (multiply_glwe_by_monomial): polys per ciphertext =
// k1; r = rot[c], or when rot == nullptr r = -(int32)((b[c]*2N + q/2)/q)
// (blind_rotate's initial rotation by the LWE body).
hipError_t launch_rotate(const ModConsts &m, const uint64_t *in, uint64_t *out, uint32_t n, uint32_t k1, size_t batch,
                         const int32_t *rot, const uint64_t *lwe_b, uint64_t lwe_q, hipStream_t s);
// Composed blind-rotation step (lwe.hip k_br_diff / k_br_add)
hipError_t launch_br_diff(const ModConsts &m, const uint64_t *cur, uint64_t *d, uint32_t n, uint32_t k1, size_t batch,
                          const uint64_t *lwe_a, uint32_t dim, uint32_t step, uint64_t lwe_q, hipStream_t s);
hipError_t launch_br_add(const ModConsts &m, const uint64_t *cur, const uint64_t *ep, uint64_t *nxt, uint32_t n,
                         uint32_t k1, size_t batch, const uint64_t *lwe_a, uint32_t dim, uint32_t step, uint64_t lwe_q,
                         hipStream_t s);
// sample_extract: glwe [batch][k+1][n] -> lwe_a [batch][k*n], lwe_b [batch]
hipError_t launch_sample_extract(const ModConsts &m, const uint64_t *glwe, uint64_t *lwe_a, uint64_t *lwe_b,
                                 uint32_t n, uint32_t k, size_t batch, hipStream_t s);
// Slot extraction (lwe.hip k_slot_extract): the LWE ciphertexts at the
// coefficients slots[s] of ct - ref (negate: ref - ct; ref nullable, ref_stride
// in words, 0 shares one ref), bodies plus offsets[s] mod q: ct [batch][2][n]
// -> lwe_a [batch][nslots][n], lwe_b [batch][nslots].  slots (each below n)
// and offsets (nullable) are HOST arrays, read before the call returns; beyond
// kSlotInline slots they go through the device table `tab` of
// slot_table_bytes(nslots) bytes.
constexpr int kSlotInline = 16;
size_t slot_table_bytes(size_t nslots);
hipError_t launch_slot_extract(const ModConsts &m, const uint64_t *ct, const uint64_t *ref, size_t ref_stride, int negate,
                               const uint32_t *slots, const uint64_t *offsets, size_t nslots, void *tab,
                               uint64_t *lwe_a, uint64_t *lwe_b, uint32_t n, size_t batch, hipStream_t s);
// Sum of LWE ciphertexts: lwe_a [terms][batch][dim], lwe_b [terms][batch] ->
// out_a [batch][dim], out_b [batch] = sum + body_offset, all mod q (any q >= 2).
hipError_t launch_lwe_sum(const ModConsts &m, const uint64_t *lwe_a, const uint64_t *lwe_b, size_t terms,
                          uint64_t body_offset, uint64_t *out_a, uint64_t *out_b, uint32_t dim, size_t batch,
                          hipStream_t s);
// LWE key switch (BootstrapEngine::key_switch); scratch of
// key_switch_scratch_bytes (0: none needed) for the split partial sums.
size_t key_switch_scratch_bytes(const ModConsts &m, uint32_t base_log, uint32_t level, uint32_t in_dim,
                                uint32_t out_dim, size_t batch);
hipError_t launch_key_switch(const ModConsts &m, uint32_t base_log, uint32_t level, uint32_t in_dim, uint32_t out_dim,
                             const uint64_t *ksk_a, const uint64_t *ksk_b, const uint64_t *lwe_a,
                             const uint64_t *lwe_b, uint64_t *out_a, uint64_t *out_b, size_t batch, void *scratch,
                             hipStream_t s);
// LWE-to-RLWE packing (lwe_pack.hip k_lwe_pack): lwe_a [batch][nslots][in_dim],
// lwe_b [batch][nslots] and the pack key [in_dim * level][2][n] -> out
// [batch][2][n] (+ out mod q with accumulate), LWE s at coefficient slots[s].
// slots (each below n) is a HOST array, read before the call returns; beyond
// kPackInline slots it goes through the device table `tab` of
// lwe_pack_table_bytes(nslots) bytes.  nslots * (in_dim * level + 1) < 2^31.
constexpr int kPackInline = 32;
size_t lwe_pack_table_bytes(size_t nslots);
hipError_t launch_lwe_pack(const ModConsts &m, uint32_t base_log, uint32_t level, uint32_t in_dim,
                           const uint64_t *pack_key, const uint64_t *lwe_a, const uint64_t *lwe_b,
                           const uint32_t *slots, size_t nslots, int accumulate, void *tab, uint64_t *out, uint32_t n,
                           size_t batch, hipStream_t s);
hipError_t launch_decompose(const ModConsts &m, const uint64_t *poly, uint64_t *out, uint32_t n, size_t npoly,
                            uint32_t base_log, uint32_t level, hipStream_t s);

// Scale-invariant BFV product (bfv_scale.hip).  Constants per (q, t) and the
// two auxiliary primes p[0], p[1] (odd, below 2^62); "R" is 2^64 and every
// *_q / *_p product constant is in Montgomery form for wmont.
struct ScaleConsts {
    uint64_t q, half_q, mu_q, qinv_q;  // (q - 1) / 2, floor(2^64 / q), -q^-1 mod 2^64
    uint64_t t_q, p1_q, pp_q;          // t R mod q, p1 R mod q, p1 p2 mod q (plain)
    uint64_t p[2], mu_p[2], qinv_p[2]; // p_j, floor(2^64 / p_j), -p_j^-1 mod 2^64
    uint64_t t_p[2], qi_p[2];          // t R mod p_j, q^-1 R mod p_j
    uint64_t p1inv_p2;                 // p1^-1 R mod p2
    uint64_t half_hi, half_lo;         // (p1 p2 - 1) / 2
};
// lift((in - ref) mod q) mod p1 / p2 over `words` words (even; 16-byte aligned
// buffers): ref nullable; word w belongs to ciphertext w / ct_words, whose
// reference starts at ref + (w / ct_words) ref_stride (0 shares one).
hipError_t launch_center_lift(const ScaleConsts &k, const uint64_t *in, const uint64_t *ref, size_t ref_stride,
                              size_t ct_words, uint64_t *out1, uint64_t *out2, size_t words, hipStream_t s);
// out = round(t X / q) mod q from X mod q, X mod p1, X mod p2; out may be xq.
hipError_t launch_scale_round(const ScaleConsts &k, const uint64_t *xq, const uint64_t *x1, const uint64_t *x2,
                              uint64_t *out, size_t words, hipStream_t s);

// SIMD (CRT batching) codec (simd_codec.hip).  tp is the plan of the negacyclic
// context (n, t); slot_at [n] (device) maps transform index k to the slot s
// with k(s) = k.  The fused family only (n <= 16384, t < 2^62).
//   encode: out = inv(X), X[k] = values[slot_at[k]] mod t; a word above `half`
//     comes back plus lift_add (q - t for the centred lift mod q, 0 for none).
//   decode: out[slot_at[k]] = fwd(in)[k].
hipError_t launch_simd_encode(const Plan &tp, const uint32_t *slot_at, const uint64_t *values, uint64_t half,
                              uint64_t lift_add, uint64_t *out, size_t batch);
hipError_t launch_simd_decode(const Plan &tp, const uint32_t *slot_at, const uint64_t *in, uint64_t *out, size_t batch);
// Composed path, any n = 2^logn and odd t: out[i] = in[tab[i]] mod t per row
// (tab [n], device), and the centred lift of canonical words in place.
hipError_t launch_simd_permute(const ModConsts &m, uint32_t logn, const uint32_t *tab, const uint64_t *in, uint64_t *out,
                               size_t npoly, hipStream_t s);
hipError_t launch_simd_lift(uint64_t half, uint64_t lift_add, uint64_t *x, size_t words, hipStream_t s);

// Hoisted Galois key switching (hoist.hip).  hoisted [batch][1 + level][n]:
// row 0 = fwd(c0), row 1 + l = fwd(d_l), d_l the unsigned digits of c1 mod q.
// tab [count][2] (device) = (g, key index) per rotation, filled from HOST
// arrays by launch_hoist_table (key_idx nullable: the identity; the entries
// travel as kernel arguments, nothing is synchronised).  key [nkeys][level][2][n]
// prepared (a_l, b_l).  launch_hoist_fwd / launch_hoist_apply: the fused family
// only (n <= 16384, q < 2^62), level >= 1, count <= kHoistMaxCount.  apply with
// pts == nullptr: out [batch][count][2][n], rotation r of ciphertext b; with
// pts [count][n] (canonical spectra): out [batch][2][n] = sum_r p_r (*)
// rotation r (+ out mod q with accumulate).
constexpr uint32_t kHoistMaxCount = 4096;
hipError_t launch_hoist_table(const uint32_t *gs, const uint32_t *key_idx, size_t count, uint32_t *tab, hipStream_t s);
hipError_t launch_hoist_fwd(const Plan &p, int level, int base_log, const uint64_t *ct, uint64_t *hoisted, size_t batch);
hipError_t launch_hoist_apply(const Plan &p, int level, const uint32_t *tab, uint32_t count, const uint64_t *key,
                              const uint64_t *pts, const uint64_t *hoisted, int accumulate, uint64_t *out, size_t batch);
// Composed path, any n = 2^logn and odd q: the digit rows (row 0 = c0's raw
// words) for the batched forward transform, and the gathered key MAC into
// spectra spec [batch][count][2][n] (pts != nullptr: [batch][2][n], summed over
// the terms) for the batched inverse.  word = the Montgomery word of the
// prepared keys (32, 64, or 65 for q >= 2^62).
hipError_t launch_hoist_digits(const ModConsts &m, uint32_t logn, uint32_t base_log, uint32_t level, const uint64_t *ct,
                               uint64_t *rows, size_t batch, hipStream_t s);
hipError_t launch_hoist_mac(const ModConsts &m, uint32_t logn, int word, int level, const uint32_t *tab, uint32_t count,
                            const uint64_t *key, const uint64_t *pts, const uint64_t *hoisted, uint64_t *spec, size_t batch,
                            hipStream_t s);

}  // namespace FHE_NS
