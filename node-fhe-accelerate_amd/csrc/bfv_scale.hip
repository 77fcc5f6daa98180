// bfv_scale.hip -- the two streaming kernels of the scale-invariant BFV
// product round(t/q (ct1 (x) ct2)) (fhe_ct_multiply_scaled_batch and its dot
// and square forms; include/fhe_gpu.h).
//
// The tensor product over the integers is taken in three channels: mod q by
// the context's own kernels, and mod two auxiliary NTT primes p1, p2 by the
// same kernels on two auxiliary contexts.  |t X| stays below p1 p2 / 2, so the
// two auxiliary residues determine y = round(t X / q) exactly.
//
//   k_center_lift   x -> lift(x) mod p1, lift(x) mod p2 with lift(x) the
//                   centred residue of x mod q in [-(q-1)/2, (q-1)/2]; with a
//                   reference row, lift((x - ref) mod q).  One read of every
//                   input word, two 16-byte stores per lane.
//   k_scale_round   (X mod q, X mod p1, X mod p2) -> round(t X / q) mod q:
//                     c   = centred(t X mod q)
//                     y_j = (t X - c) q^-1 mod p_j
//                     v   = (y_2 - y_1) p1^-1 mod p2,  y = y_1 + p1 v in [0, p1 p2)
//                     out = y_1 + (p1 mod q) v - [y > (p1 p2 - 1)/2] (p1 p2 mod q)  (mod q)
//                   three 16-byte reads and one 16-byte store per lane.
//
// When t count n q < p1 the first auxiliary prime alone determines y (the
// host decides per call): the lift then skips its second output (out2 ==
// nullptr) and k_scale_round<true> centres y_1 against p1 / 2.  The words are
// the same by definition.
//
// Every product is a canonical Montgomery product with the 65th bit (wmont),
// so one code path serves every odd q < 2^64 and both p_j < 2^62; constants in
// Montgomery form are prepared on the host per (q, t) (ScaleConsts).  Words
// are two per lane, rows 16-byte aligned; neither kernel uses LDS or scratch.
#include "fhe_internal.hpp"

namespace FHE_NS {

static constexpr int kScaleBlock = 256;
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// x mod q for any u64 x and any q >= 2
__device__ __forceinline__ uint64_t sc_red(uint64_t x, uint64_t q, uint64_t mu) {
    return x < q ? x : mod64_slow(x, q, mu);
}
// the signed value (neg ? -mag : mag), mag < 2^63, as a canonical residue mod p
__device__ __forceinline__ uint64_t sc_signed(uint64_t mag, bool neg, uint64_t p, uint64_t mu) {
    const uint64_t r = sc_red(mag, p, mu);
    return (neg && r != 0) ? p - r : r;
}

__device__ __forceinline__ void lift_word(uint64_t x, const ScaleConsts &k, uint64_t &o1, uint64_t &o2) {
    const bool neg = x > k.half_q;           // x canonical mod q
    const uint64_t mag = neg ? k.q - x : x;  // <= (q - 1) / 2
    o1 = sc_signed(mag, neg, k.p[0], k.mu_p[0]);
    o2 = sc_signed(mag, neg, k.p[1], k.mu_p[1]);
}

// in [npoly][n] (ref: [npoly or 1][n], ref_stride words between the rows of
// consecutive ciphertexts of 2 n words; 0 shares one)
__global__ void __launch_bounds__(kScaleBlock)
k_center_lift(const uint64_t *__restrict__ in, const uint64_t *__restrict__ ref, size_t ref_stride, size_t ct_words,
              uint64_t *__restrict__ out1, uint64_t *__restrict__ out2, size_t pairs, ScaleConsts k) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const size_t w = 2 * i;
        const u64x2 x = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(in + w));
        uint64_t a = sc_red(x.x, k.q, k.mu_q), b = sc_red(x.y, k.q, k.mu_q);
        if (ref) {
            const size_t c = w / ct_words, r = c * ref_stride + (w - c * ct_words);
            const u64x2 y = *reinterpret_cast<const u64x2 *>(ref + r);
            a = wsub(a, sc_red(y.x, k.q, k.mu_q), k.q);
            b = wsub(b, sc_red(y.y, k.q, k.mu_q), k.q);
        }
        u64x2 z1, z2;
        uint64_t u, v;
        lift_word(a, k, u, v);
        z1.x = u;
        z2.x = v;
        lift_word(b, k, u, v);
        z1.y = u;
        z2.y = v;
        __builtin_nontemporal_store(z1, reinterpret_cast<u64x2 *>(out1 + w));
        if (out2) __builtin_nontemporal_store(z2, reinterpret_cast<u64x2 *>(out2 + w));
    }
}

// ONE: |rnd(t X)| < p1 / 2, so y_1 alone determines it (x2 unused)
template <bool ONE>
__device__ __forceinline__ uint64_t scale_word(uint64_t xq, uint64_t x1, uint64_t x2, const ScaleConsts &k) {
    // c = centred(t X mod q) as (magnitude, sign)
    const uint64_t u = wmont(sc_red(xq, k.q, k.mu_q), k.t_q, k.q, k.qinv_q);
    const bool cneg = u > k.half_q;
    const uint64_t cmag = cneg ? k.q - u : u;
    // y_j = (t x_j - c) q^-1 mod p_j
    uint64_t y[2];
    const uint64_t xs[2] = {x1, x2};
#pragma unroll
    for (int j = 0; j < (ONE ? 1 : 2); ++j) {
        const uint64_t p = k.p[j];
        const uint64_t tx = wmont(sc_red(xs[j], p, k.mu_p[j]), k.t_p[j], p, k.qinv_p[j]);
        const uint64_t c = sc_signed(cmag, cneg, p, k.mu_p[j]);
        y[j] = wmont(wsub(tx, c, p), k.qi_p[j], p, k.qinv_p[j]);
    }
    if constexpr (ONE) {  // out = y_1 - [y_1 > (p1 - 1) / 2] (p1 mod q)  (mod q)
        uint64_t r = sc_red(y[0], k.q, k.mu_q);
        if (y[0] > (k.p[0] - 1) / 2) r = wsub(r, wmont(k.p1_q, 1, k.q, k.qinv_q), k.q);
        return r;
    }
    // Garner: y = y_1 + p1 v, v = (y_2 - y_1) p1^-1 mod p2
    const uint64_t p2 = k.p[1];
    const uint64_t v = wmont(wsub(y[1], sc_red(y[0], p2, k.mu_p[1]), p2), k.p1inv_p2, p2, k.qinv_p[1]);
    // negative iff y_1 + p1 v > (p1 p2 - 1) / 2  (two-word compare)
    const uint64_t lo0 = k.p[0] * v, lo = lo0 + y[0];
    const uint64_t hi = __umul64hi(k.p[0], v) + (lo < lo0 ? 1 : 0);
    const bool neg = hi > k.half_hi || (hi == k.half_hi && lo > k.half_lo);
    // out = y_1 + (p1 mod q) v - [neg] (p1 p2 mod q)  (mod q)
    const uint64_t pv = wmont(sc_red(v, k.q, k.mu_q), k.p1_q, k.q, k.qinv_q);
    uint64_t r = wadd(sc_red(y[0], k.q, k.mu_q), pv, k.q);
    if (neg) r = wsub(r, k.pp_q, k.q);
    return r;
}

// out may be xq (each lane reads its words before it writes them)
template <bool ONE>
__global__ void __launch_bounds__(kScaleBlock)
k_scale_round(const uint64_t *xq, const uint64_t *__restrict__ x1, const uint64_t *__restrict__ x2, uint64_t *out,
              size_t pairs, ScaleConsts k) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const size_t w = 2 * i;
        const u64x2 a = *reinterpret_cast<const u64x2 *>(xq + w);
        const u64x2 b = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(x1 + w));
        u64x2 c = {0, 0};
        if constexpr (!ONE) c = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(x2 + w));
        u64x2 z;
        z.x = scale_word<ONE>(a.x, b.x, c.x, k);
        z.y = scale_word<ONE>(a.y, b.y, c.y, k);
        __builtin_nontemporal_store(z, reinterpret_cast<u64x2 *>(out + w));
    }
}

static unsigned scale_grid(size_t pairs) {
    const size_t cap = 256 * 16;  // 256 CUs x 16 blocks: grid-stride beyond
    const size_t g = (pairs + kScaleBlock - 1) / kScaleBlock;
    return (unsigned)(g > cap ? cap : g);
}

hipError_t launch_center_lift(const ScaleConsts &k, const uint64_t *in, const uint64_t *ref, size_t ref_stride,
                              size_t ct_words, uint64_t *out1, uint64_t *out2, size_t words, hipStream_t s) {
    if (words == 0) return hipSuccess;
    if ((words & 1) || (ct_words & 1) || (ref_stride & 1) || ct_words == 0 ||
        (((uintptr_t)in | (uintptr_t)ref | (uintptr_t)out1 | (uintptr_t)out2) & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_center_lift, dim3(scale_grid(words / 2)), dim3(kScaleBlock), 0, s, in, ref, ref_stride, ct_words,
                       out1, out2, words / 2, k);
    return hipGetLastError();
}

hipError_t launch_scale_round(const ScaleConsts &k, const uint64_t *xq, const uint64_t *x1, const uint64_t *x2,
                              uint64_t *out, size_t words, hipStream_t s) {
    if (words == 0) return hipSuccess;
    if ((words & 1) || (((uintptr_t)xq | (uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)out) & 15)) return hipErrorInvalidValue;
    if (x2)
        hipLaunchKernelGGL(k_scale_round<false>, dim3(scale_grid(words / 2)), dim3(kScaleBlock), 0, s, xq, x1, x2, out,
                           words / 2, k);
    else  // the single-prime form
        hipLaunchKernelGGL(k_scale_round<true>, dim3(scale_grid(words / 2)), dim3(kScaleBlock), 0, s, xq, x1, x2, out,
                           words / 2, k);
    return hipGetLastError();
}

}  // namespace FHE_NS
