// ct_square.hip -- ciphertext squaring and squared difference
// (EncryptionEngine::square, encryption.cpp:1004-1055; compute_anomaly_score's
// square(subtract(ballot, expected)), :1305-1321) for coefficient-form
// ciphertexts, one kernel per batch:
//
//   d  = ct                       (or (ct mod q) - (ref mod q) mod q, DIFF)
//   X0 = fwd(d.c0)   X1 = fwd(d.c1)
//   c0 = inv(X0 X0)  c1 = inv(2 X0 X1)  c2 = inv(X1 X1)
//
// multiply(d, d) runs 4 forward transforms of data that holds 2 distinct
// polynomials, after a subtraction that writes d to memory.  Here one
// workgroup owns one ciphertext, subtracts while pass 0 loads
// (fwd_poly_diff), and runs 2 forward + 3 inverse transforms back to back.
// Every product is exact over Z_q, so the words equal multiply(d, d)'s.
//
// One schedule for every shape; a thread parks a spectrum as W words at its
// own positions of an output row that is overwritten later, behind a barrier
// (as k_ct_mul2):
//   1. X0 = fwd(d0)      stash canon(X0) in row 1;  inv(X0 X0)   -> row 0
//   2. X1 = fwd(d1)      stash canon(X1) in row 2;  inv(2 X0 X1) -> row 1
//   3. X1 back from row 2;                           inv(X1 X1)   -> row 2
// Products are Montgomery (x R^-1); the R is folded into the inverse's N^-1
// (ninv_r), as in k_ct_mul.
// Unit defines as ntt_cipher.hip (the same transforms at the same shapes).
#ifndef FHE_OPAQUE_TW
#define FHE_OPAQUE_TW 2
#endif
#ifndef FHE_U64_NOVCC
#define FHE_U64_NOVCC 1
#endif
#ifndef FHE_MULHI64
#define FHE_MULHI64 4
#endif
#include "fhe_internal.hpp"

namespace FHE_NS {

// At most 4 waves per SIMD (128 VGPRs), k_ct_mul's budget: with the 64 of 8
// waves the 16-coefficient 32-bit kernels spilled.
template <int LOGN, typename W>
constexpr int ctsq_occ() {
    constexpr int w = Geo<LOGN>::template occ_waves<W>();
    return w > 4 ? 4 : w;
}

template <int LOGN, typename W, bool LAZY, bool DIFF>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, (ctsq_occ<LOGN, W>()))
k_ct_sq(const uint64_t *__restrict__ ct, const uint64_t *__restrict__ ref, size_t ref_stride, uint64_t *out,
        size_t batch, NttArgs<W> A) {
    using G = Geo<LOGN>;
    // u64: a 16-word spectrum and the raw pairs of the loader leave no VGPRs for lookahead
    constexpr int PF = sizeof(W) == 8 ? 0 : (G::LOGE == 5 ? 1 : kPfPolymul);
    constexpr int LAST = G::NP - 1;
    __shared__ W lds_all[G::P * G::LW];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < batch;
    if (G::P == 1 && !valid) return;  // whole workgroup: no barrier is skipped
    const bool live = G::P == 1 || valid;  // stash accesses of a tail ciphertext are skipped
    W *lds = lds_all + pl * G::LW;
    const uint64_t *xr = ct + poly * 2 * G::N;
    const uint64_t *rr = DIFF ? ref + poly * ref_stride : nullptr;
    uint64_t *orow = out + poly * 3 * G::N;
    W *s1 = reinterpret_cast<W *>(orow + G::N), *s2 = reinterpret_cast<W *>(orow + 2 * G::N);
    W v[G::E];
    // a fresh opaque copy of the lane index per phase (as k_ct_mul)
    auto lane = [&]() {
        uint32_t t = tau;
        asm volatile("" : "+v"(t));
        return t;
    };
    auto fwd = [&](uint32_t t, int row) {
        if constexpr (DIFF) fwd_poly_diff<LOGN, LAZY, PF>(lds, v, t, xr + row * G::N, rr + row * G::N, valid, A);
        else fwd_poly<LOGN, LAZY, PF>(lds, v, t, xr + row * G::N, valid, A);
    };
    // 1. X0: stash, c0 = inv(X0 X0)
    uint32_t tp = lane();
    fwd(tp, 0);
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        const W x0 = fwd_to_canon<LAZY>(v[e], A);
        if (live) s1[gidx<LOGN, LAST>(tp, e)] = x0;
        v[e] = A.ar.mont(x0, x0);
    }
    __syncthreads();
    tp = lane();
    inv_poly_from_regs<LOGN, PF>(lds, v, tp, orow, valid, A, A.ninv_r);
    __syncthreads();
    // 2. X1: stash, c1 = inv(2 X0 X1)
    tp = lane();
    fwd(tp, 1);
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        const uint32_t gi = gidx<LOGN, LAST>(tp, e);
        const W x1 = fwd_to_canon<LAZY>(v[e], A);
        const W x0 = live ? s1[gi] : W(0);
        if (live) s2[gi] = x1;
        const W m = A.ar.mont(x0, x1);
        v[e] = A.ar.red2q(m + m);
        // u64: 4 stash words in flight at a time (as k_ct_mul2)
        if (sizeof(W) == 8 && (e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // every stash read of row 1 precedes its final stores
    tp = lane();
    inv_poly_from_regs<LOGN, PF>(lds, v, tp, orow + G::N, valid, A, A.ninv_r);
    __syncthreads();
    // 3. c2 = inv(X1 X1)
    tp = lane();
#pragma unroll
    for (int e = 0; e < G::E; ++e) {
        const W x1 = live ? s2[gidx<LOGN, LAST>(tp, e)] : W(0);
        v[e] = A.ar.mont(x1, x1);
    }
    __syncthreads();  // every stash read of row 2 precedes its final stores
    tp = lane();
    inv_poly_from_regs<LOGN, PF>(lds, v, tp, orow + 2 * G::N, valid, A, A.ninv_r);
}

template <int K, typename W, bool LAZY>
static void ctsq_launch(const Plan &p, const NttArgs<W> &A, const uint64_t *ct, const uint64_t *ref, size_t ref_stride,
                        uint64_t *out, size_t batch) {
    using G = Geo<K>;
    const dim3 grid((batch + G::P - 1) / G::P), block(G::THREADS);
    if (ref)
        hipLaunchKernelGGL((k_ct_sq<K, W, LAZY, true>), grid, block, 0, p.stream, ct, ref, ref_stride, out, batch, A);
    else
        hipLaunchKernelGGL((k_ct_sq<K, W, LAZY, false>), grid, block, 0, p.stream, ct, ref, ref_stride, out, batch, A);
}

template <int LOGN, typename W>
static hipError_t ctsq_one(const Plan &p, const NttArgs<W> &A, const uint64_t *ct, const uint64_t *ref,
                           size_t ref_stride, uint64_t *out, size_t batch) {
    // 32-bit words at N = 8192 / 16384: 32 coefficients per thread (k_ct_mul2's geometry)
    constexpr int K = (sizeof(W) == 4 && (LOGN == 13 || LOGN == 14)) ? gk(LOGN, 5) : LOGN;
    if constexpr (sizeof(W) == 4) {
        if (p.lazy) {
            ctsq_launch<K, W, true>(p, A, ct, ref, ref_stride, out, batch);
            return hipGetLastError();
        }
    }
    ctsq_launch<K, W, false>(p, A, ct, ref, ref_stride, out, batch);
    return hipGetLastError();
}

template <typename W>
static hipError_t ctsq_dispatch(const Plan &p, const NttArgs<W> &A, const uint64_t *ct, const uint64_t *ref,
                                size_t ref_stride, uint64_t *out, size_t batch) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return ctsq_one<L, W>(p, A, ct, ref, ref_stride, out, batch);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ct_square(const Plan &p, const uint64_t *ct, const uint64_t *ref, size_t ref_stride, uint64_t *out,
                            size_t batch) {
    if (batch == 0) return hipSuccess;
    if (p.word == 32) return ctsq_dispatch<uint32_t>(p, p.a32, ct, ref, ref_stride, out, batch);
    return ctsq_dispatch<uint64_t>(p, p.a64, ct, ref, ref_stride, out, batch);
}

}  // namespace FHE_NS
