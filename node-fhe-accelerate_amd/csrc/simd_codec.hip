// simd_codec.hip -- SIMD (CRT batching) codec of BFV plaintexts
// (fhe_simd_encode_batch / fhe_simd_decode_batch).
//
// With t = 1 mod 2N the plaintext ring Z_t[X]/(X^N + 1) splits into N slots:
// the slot values of a message are its evaluations at the odd powers of the
// 2N-th root psi_t, which is what the negacyclic transform of a context
// (N, t) computes (X_k = a(psi^(2k+1)), natural order).  Slot s sits at the
// transform index k(s) = (e(s) - 1) / 2, e(s) = +-3^i mod 2N, so that the
// automorphisms sigma_3 / sigma_-1 rotate the rows / swap them.
//
//   encode: out = inv(X),  X[k(s)] = values[s] mod t   (+ centred lift mod q)
//   decode: out[s] = fwd(in)[k(s)]
//
// Both are the single-transform kernels of ntt_inv.hip / ntt_fwd.hip with the
// slot permutation folded into the side of the transform that is in natural
// order: encode GATHERS its spectrum registers (position gi takes
// values[slot_at[gi]]), decode SCATTERS them (register at gi goes to
// out[slot_at[gi]]).  No separate pass, no temporary row.
//
// The permuted side goes straight to memory as 8-byte accesses.  A row is
// touched by exactly one workgroup and at most 128 KiB, so it stays in L2
// between the first touch of a cache line and the last: HBM sees whole lines
// once, the partial-line cost is L2 transactions only.  Staging the row
// through LDS instead (coalesced HBM access, permutation in LDS) would need a
// second N-word buffer beside the exchange buffer -- at N = 16384 with 64-bit
// words that is 2 x 128 KiB, over the 160 KiB of a CU -- or a pass through the
// exchange buffer with two more barriers per polynomial; the slot index of
// +-3^i has no locality for a pad to exploit (consecutive k land N/2 slots
// apart every other step), so the LDS side would bank-conflict as well.
//
// k_simd_permute is the composed path (n > 16384 or t >= 2^62, and
// FHE_SIMD_FUSED=0): a gather by table with the reduction mod t, around the
// batched transforms of the (N, t) context.
#ifndef FHE_U64_NOVCC
#define FHE_U64_NOVCC 1
#endif
#ifndef FHE_MULHI64
#define FHE_MULHI64 4
#endif
#ifndef FHE_SPLIT_X64
#define FHE_SPLIT_X64 1
#endif
#ifndef FHE_STREAM_DEPTH
#define FHE_STREAM_DEPTH 1
#endif
#include "fhe_internal.hpp"

namespace FHE_NS {

// ---------------------------------------------------------------- encode
template <int LOGN, typename W>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, Geo<LOGN>::template occ_waves<W>())
k_simd_encode(const uint64_t *__restrict__ values, const uint32_t *__restrict__ slot_at, uint64_t *__restrict__ out,
              size_t batch, uint64_t half, uint64_t lift_add, NttArgs<W> A) {
    using G = Geo<LOGN>;
    __shared__ W lds_all[G::P * lds_elems<LOGN, W>()];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < batch;
    W *lds = lds_all + pl * lds_elems<LOGN, W>();
    if (G::P == 1 && !valid) return;
    W v[G::E];
    const uint64_t *src = values + poly * G::N;
    const uint64_t lim = (uint64_t)A.ar.q2;  // GS inputs must be < 2t
    // spectrum position gi of register e takes the value of slot slot_at[gi].  The index is loaded
    // again with a word that needs the slow path: no index stays live beside the raw words.
    // One polynomial per workgroup: the gathers go out in chunks of 4, one chunk ahead (all 16 raw
    // words with their indices do not fit the 64 VGPRs of the 32-bit kernel at N = 8192).
    if constexpr (G::P == 1) {
        const auto r = brsrc(src);
        load_coeffs_chunked<G::E, 4, 1>(v, lim, SlowRed<W>{A}, [&](int e) -> uint64_t {
            return bload<0>(r, slot_at[gidx<LOGN, G::NP - 1>(tau, e)] * 8u, 0);
        });
    } else {
        load_coeffs_r<G::E>(v, lim, SlowRed<W>{A}, [&](int e) -> uint64_t {
            return valid ? src[slot_at[gidx<LOGN, G::NP - 1>(tau, e)]] : 0;
        });
    }
    inv_poly_from_regs<LOGN>(lds, v, tau, out + poly * G::N, valid, A, A.ninv, 0,
                             [&](uint32_t, uint64_t x) -> uint64_t { return x > half ? x + lift_add : x; });
}

// ---------------------------------------------------------------- decode
// Every degree at 16 coefficients per thread.  (k_ntt_fwd's 32 per thread for 64-bit words at
// N = 16384 sits at 128 VGPRs; the slot indices of the scattered store spill there.)
template <int LOGN, typename W, bool LAZY>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, Geo<LOGN>::template occ_waves<W>())
k_simd_decode(const uint64_t *__restrict__ in, const uint32_t *__restrict__ slot_at, uint64_t *__restrict__ out,
              size_t batch, NttArgs<W> A) {
    using G = Geo<LOGN>;
    __shared__ W lds_all[G::P * lds_elems<LOGN, W>()];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < batch;
    W *lds = lds_all + pl * lds_elems<LOGN, W>();
    if (G::P == 1 && !valid) return;  // whole workgroup: no barrier is skipped
    W v[G::E];
    fwd_poly<LOGN, LAZY, kPfSingle, false>(lds, v, tau, in + poly * G::N, valid, A);
    if (!valid) return;
    uint64_t *dst = out + poly * G::N;
    // the register at spectrum position gi is the value of slot slot_at[gi]
    if constexpr (G::P == 1) {
        const auto r = brsrc(dst);
        // 8 slot indices in flight at a time
        constexpr int CH = G::E < 8 ? G::E : 8;
#pragma unroll
        for (int c = 0; c < G::E; c += CH) {
            uint32_t s[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) s[e] = slot_at[gidx<LOGN, G::NP - 1>(tau, c + e)];
#pragma unroll
            for (int e = 0; e < CH; ++e) bstore<0>(r, s[e] * 8u, 0, (uint64_t)fwd_to_canon<LAZY>(v[c + e], A));
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const uint32_t s = slot_at[gidx<LOGN, G::NP - 1>(tau, e)];
            dst[s] = (uint64_t)fwd_to_canon<LAZY>(v[e], A);
        }
    }
}

template <int LOGN, typename W>
static hipError_t encode_one(const Plan &p, const NttArgs<W> &A, const uint32_t *slot_at, const uint64_t *values,
                             uint64_t half, uint64_t lift_add, uint64_t *out, size_t batch) {
    using G = Geo<LOGN>;
    const size_t blocks = (batch + G::P - 1) / G::P;
    hipLaunchKernelGGL((k_simd_encode<LOGN, W>), dim3((unsigned)blocks), dim3(G::THREADS), 0, p.stream, values, slot_at,
                       out, batch, half, lift_add, A);
    return hipGetLastError();
}
template <int LOGN, typename W>
static hipError_t decode_one(const Plan &p, const NttArgs<W> &A, const uint32_t *slot_at, const uint64_t *in,
                             uint64_t *out, size_t batch) {
    using G = Geo<LOGN>;
    const size_t blocks = (batch + G::P - 1) / G::P;
    if constexpr (sizeof(W) == 4) {
        if (p.lazy) {
            hipLaunchKernelGGL((k_simd_decode<LOGN, W, true>), dim3((unsigned)blocks), dim3(G::THREADS), 0, p.stream, in,
                               slot_at, out, batch, A);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_simd_decode<LOGN, W, false>), dim3((unsigned)blocks), dim3(G::THREADS), 0, p.stream, in, slot_at,
                       out, batch, A);
    return hipGetLastError();
}

template <typename W>
static hipError_t codec_dispatch(const Plan &p, const NttArgs<W> &A, bool enc, const uint32_t *slot_at, const uint64_t *in,
                                 uint64_t half, uint64_t lift_add, uint64_t *out, size_t batch) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return enc ? encode_one<L, W>(p, A, slot_at, in, half, lift_add, out, batch) \
                       : decode_one<L, W>(p, A, slot_at, in, out, batch);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

static hipError_t codec_any(const Plan &p, bool enc, const uint32_t *slot_at, const uint64_t *in, uint64_t half,
                            uint64_t lift_add, uint64_t *out, size_t batch) {
    if (p.wide || p.logn > (uint32_t)kMaxFusedLogN || p.logn < (uint32_t)kMinLogN) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    if (p.word == 32) return codec_dispatch<uint32_t>(p, p.a32, enc, slot_at, in, half, lift_add, out, batch);
    return codec_dispatch<uint64_t>(p, p.a64, enc, slot_at, in, half, lift_add, out, batch);
}

hipError_t launch_simd_encode(const Plan &tp, const uint32_t *slot_at, const uint64_t *values, uint64_t half,
                              uint64_t lift_add, uint64_t *out, size_t batch) {
    return codec_any(tp, true, slot_at, values, half, lift_add, out, batch);
}
hipError_t launch_simd_decode(const Plan &tp, const uint32_t *slot_at, const uint64_t *in, uint64_t *out, size_t batch) {
    return codec_any(tp, false, slot_at, in, 0, 0, out, batch);
}

// ---------------------------------------------------------------- composed path
// out[i] = in[tab[i]] mod t, row by row: gather, coalesced 8-byte stores (the
// scattered side is the read side, as in galois.hip).
static constexpr int kPermuteBlock = 256;
__global__ void __launch_bounds__(kPermuteBlock)
k_simd_permute(const uint64_t *__restrict__ in, const uint32_t *__restrict__ tab, uint64_t *__restrict__ out, uint32_t logn,
               size_t npoly, ModConsts m) {
    const uint32_t n = 1u << logn;
    const size_t total = npoly << logn;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t poly = i >> logn;
        const uint32_t k = (uint32_t)i & (n - 1);
        const uint64_t x = in[(poly << logn) + tab[k]];
        out[i] = x < m.q ? x : mod64_slow(x, m.q, m.mu);
    }
}
__global__ void __launch_bounds__(kPermuteBlock)
k_simd_lift(uint64_t *__restrict__ x, size_t words, uint64_t half, uint64_t lift_add) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
        const uint64_t y = x[i];
        if (y > half) x[i] = y + lift_add;
    }
}

static unsigned stream_grid(size_t work) {
    const size_t cap = 256 * 16, g = (work + kPermuteBlock - 1) / kPermuteBlock;
    return (unsigned)(g > cap ? cap : g);
}
hipError_t launch_simd_permute(const ModConsts &m, uint32_t logn, const uint32_t *tab, const uint64_t *in, uint64_t *out,
                               size_t npoly, hipStream_t s) {
    if (npoly == 0) return hipSuccess;
    if (logn < 2 || logn > (uint32_t)kMaxLogN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_simd_permute, dim3(stream_grid(npoly << logn)), dim3(kPermuteBlock), 0, s, in, tab, out, logn,
                       npoly, m);
    return hipGetLastError();
}
hipError_t launch_simd_lift(uint64_t half, uint64_t lift_add, uint64_t *x, size_t words, hipStream_t s) {
    if (words == 0 || lift_add == 0) return hipSuccess;
    hipLaunchKernelGGL(k_simd_lift, dim3(stream_grid(words)), dim3(kPermuteBlock), 0, s, x, words, half, lift_add);
    return hipGetLastError();
}

}  // namespace FHE_NS
