// hoist.hip -- hoisted Galois key switching (fhe_ct_hoist_batch,
// fhe_ct_hoisted_galois_batch, fhe_ct_hoisted_linear_batch).
//
// The negacyclic transform holds X_k = a(psi^(2k+1)) at index k (natural
// order), so sigma_g acts on a spectrum as the index map
//   pi_g(k) = (((2k+1) g mod 2N) - 1) / 2 = g k + (g - 1) / 2 mod N:
// fwd(sigma_g(a))[k] = fwd(a)[pi_g(k)], no sign and no arithmetic.  A
// ciphertext is therefore decomposed and transformed ONCE (k_hoist_fwd: the
// spectra of c0 and of the unsigned digits d_l of c1), and every rotation of
// it is a gathered multiply-accumulate against the key rows followed by two
// inverse transforms (k_hoist_apply, one component per workgroup).  The Galois keys of
// fhe_switch_key_generate serve unchanged: sum_l sigma_g(d_l) 2^(l B) =
// sigma_g(c1) mod q.
//
// Which side is permuted: the READ side.  Position gi of the accumulator
// spectra takes hoisted[row][pi_g(gi)] (8-byte gathers, a stride of g words
// between neighbouring lanes) and meets the key and plaintext rows at gi,
// coalesced; the accumulators stay at the gidx positions inv_poly_from_regs
// wants, so no exchange is added.  A hoisted ciphertext is (1 + level) rows
// that a workgroup reads whole per rotation.  While the hoisted rows of the
// batch fit in L2 the partial lines cost L2 transactions only; with thousands
// of ciphertexts the working set is far beyond L2 and every rotation gathers
// its rows from HBM again, which is where the separate key switches, digits in
// registers, are faster (measured: DESIGN.md section 5).
//
// Linear transform (LIN): out = sum_r p_r (*) rot_r(ct).  The plaintext row is
// multiplied in once per term on the bracket  fwd(sigma_g(c0)) + sum_l ... ,
// the sum over r runs on spectra, and two inverse transforms finish the whole
// sum.  Plaintext rows are canonical transforms without a Montgomery factor:
// mont(bracket, p) carries R^-1, which the inverse's N^-1 R scale removes.
//
// Composed path (N > 16384, q >= 2^62, FHE_HOIST_FUSED=0): k_hoist_digits +
// the batched forward transform; k_hoist_mac (the same gathered MAC, one lane
// per spectrum position, canonical arithmetic for any odd q) + the batched
// inverse, in place in the output.  Same words: every step is exact mod q.
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
#ifndef FHE_OPAQUE_TW
#define FHE_OPAQUE_TW 2  // several transforms per kernel: 32-bit twiddles re-read per transform, not kept in SGPRs
#endif
#include "fhe_internal.hpp"
#include "lwe_ops.hpp"

namespace FHE_NS {

// ---------------------------------------------------------------- hoist
// Row 0 = fwd(c0), row 1 + l = fwd(d_l), d_l = ((c1 mod q) >> l B) & (2^B - 1).
// The digits are extracted on the load of each digit transform.
template <int LOGN, typename W, bool LAZY>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, Geo<LOGN>::template occ_waves<W>())
k_hoist_fwd(const uint64_t *__restrict__ ct, uint64_t *__restrict__ hoisted, size_t batch, int level, int base_log,
            NttArgs<W> A) {
    using G = Geo<LOGN>;
    __shared__ W lds_all[G::P * lds_elems<LOGN, W>()];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < batch;
    W *lds = lds_all + pl * lds_elems<LOGN, W>();
    if (G::P == 1 && !valid) return;  // whole workgroup: no barrier is skipped
    const uint64_t *src = ct + (valid ? poly : 0) * 2 * G::N;
    uint64_t *dst = hoisted + (valid ? poly : 0) * (size_t)(1 + level) * G::N;
    W v[G::E];
    auto store_row = [&](int row) {
        if (!valid) return;
        uint32_t ts = tau;
        asm volatile("" : "+v"(ts));  // the store addresses are formed here, not held across the transforms
        uint64_t *d = dst + (size_t)row * G::N;
        if constexpr (G::P == 1) {  // as k_ntt_fwd: one lane offset, constant slot offsets, no 64-bit address per word
            const auto rs = brsrc(d);
            const uint32_t vo = LastIO<LOGN>::vo(tau);
#pragma unroll
            for (int e = 0; e < G::E; ++e) bstore(rs, vo, LastIO<LOGN>::so(e), (uint64_t)fwd_to_canon<LAZY>(v[e], A));
        } else {
#pragma unroll
            for (int e = 0; e < G::E; ++e)
                __builtin_nontemporal_store((uint64_t)fwd_to_canon<LAZY>(v[e], A), d + gidx<LOGN, G::NP - 1>(ts, e));
        }
    };
    // One loop over the rows: row 0 loads c0 (reduced into the transform's lazy range), row 1 + l
    // the digit l of c1.  c1 is read again for every digit: its row was just touched by this
    // workgroup (an L2 hit); holding its canonical words across the digit transforms instead
    // spilled 4 - 80 VGPRs at the transform's own occupancy.  The transform is run as k_dmac
    // runs it: coefficients narrowed as they arrive, pass 0, then the remaining passes.
    const uint64_t mask = (1ull << base_log) - 1, lim = (uint64_t)(A.ar.q2 * 2);
    for (int row = 0; row <= level; ++row) {
        if (row > 0 && G::NP > 1) __syncthreads();  // the previous transform's last exchange is read
        uint32_t tr = tau;
        asm volatile("" : "+v"(tr));  // per-row copy of the lane index: no address arithmetic hoisted out of the loop
        const uint32_t shift = row ? (uint32_t)(row - 1) * (uint32_t)base_log : 0u;
        const uint64_t *in = src + (row ? G::N : 0);
        const Tw<W> *const twf = opaque_tw(A.twf);
        Tw<W> t0[PassTw<LOGN, 0>::COUNT];
        load_tw<LOGN, 0>(tr, twf, t0);
#pragma unroll
        for (int t = 0; t < G::E; ++t) {
            // P == 1: the workgroup's row through a buffer resource, no 64-bit address per word.
            // Not streamed: c1 is read once per digit.
            uint64_t x;
            if constexpr (G::P == 1) x = bload<0>(brsrc(in), tr * 8u, cbrv(t, G::LOGE) * G::T * 8u);
            else x = valid ? in[tr + cbrv(t, G::LOGE) * G::T] : 0;
            // a digit of a canonical word is below q
            v[t] = row ? W((red_q(x, A.q64, A.mu64) >> shift) & mask) : load_lazy<W>(x, lim, A.q64, A.mu64);
        }
        fwd_pass<LOGN, 0, LAZY>(v, t0, A.ar);
        fwd_rest<LOGN, 1, LAZY, kPfSingle>(lds, v, tr, twf, A.ar);
        store_row(row);
    }
}

// ---------------------------------------------------------------- apply
struct HoistArgs {
    const uint64_t *hoisted;  // [batch][1 + level][n], canonical spectra
    const uint64_t *key;      // [nkeys][level][2][n] prepared (a_l, b_l)
    const uint64_t *pts;      // LIN: [count][n] canonical plaintext spectra
    const uint32_t *tab;      // [count][2] = (g, key index)
    uint64_t *out;            // [batch][count][2][n]; LIN: [batch][2][n]
    size_t batch;
    uint32_t count;
    int level, accumulate;
};

// One workgroup per (ciphertext, rotation, component) -- LIN: per (ciphertext,
// component), looping over the terms -- holds ONE accumulator spectrum at its
// gidx positions; blockIdx.z is the component (0 gathers row 0 too and takes
// the b_l rows, 1 the a_l rows).  Both components in one workgroup issue the
// gathers once but park a second spectrum across the first inverse transform:
// that form spilled 9 - 155 VGPRs in every instantiation (the register budget
// is the transform's own), this one does not.  Positions go in chunks of
// kHoistChunk (2 for 64-bit lanes and for the linear transform) so that only
// the accumulator and one chunk's loads are live; the loop over the terms runs inside a chunk and carries that
// chunk of the accumulator only (terms outside, every chunk's address
// arithmetic live across the loop, spilled 12 - 54 VGPRs).
constexpr int kHoistChunk = 4;
// [0, 4q) -> [0, 2q) by compare and select.  Arith::red2q's flag-free 64-bit form takes its
// constant through an SGPR-constrained asm, which the backend cannot place inside the
// runtime digit loop below ("illegal VGPR to SGPR copy"); the loop is bound by its gathers.
template <typename W>
__device__ __forceinline__ W hoist_red2q(W x, const Arith<W> &ar) { return umin(x, W(x - ar.q2)); }
template <int LOGN, typename W, bool LIN>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, Geo<LOGN>::template occ_waves<W>())
k_hoist_apply(HoistArgs D, NttArgs<W> A) {
    using G = Geo<LOGN>;
    constexpr int CH = (sizeof(W) == 8 || LIN) && G::E > 2 ? 2 : (G::E < kHoistChunk ? G::E : kHoistChunk);
    __shared__ W lds_all[G::P * lds_elems<LOGN, W>()];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < D.batch;
    W *lds = lds_all + pl * lds_elems<LOGN, W>();
    if (G::P == 1 && !valid) return;
    const int level = D.level;
    const uint32_t j = blockIdx.z;
    const uint64_t *hrow = D.hoisted + (valid ? poly : 0) * (size_t)(1 + level) * G::N;
    W acc[G::E];
#pragma unroll
    for (int e = 0; e < G::E; ++e) acc[e] = W(0);
    const uint32_t r0 = LIN ? 0u : blockIdx.y, r1 = LIN ? D.count : r0 + 1;
    // chunk outside, terms inside: the loop over the terms carries one chunk of the accumulator
#pragma unroll
    for (int c = 0; c < G::E; c += CH) {
        for (uint32_t r = r0; r < r1; ++r) {
            uint32_t tr = tau;
            asm volatile("" : "+v"(tr));  // per-term copy of the lane index: no address arithmetic hoisted out of the loop
            const uint32_t g = D.tab[2 * r], off = (g - 1) >> 1;
            // component 0 takes b_l (row 2l + 1 of the key block), component 1 a_l (row 2l)
            const uint64_t *key = D.key + ((size_t)D.tab[2 * r + 1] * level * 2 + (1 - j)) * G::N;
            uint32_t pk[CH];
            W b[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                pk[e] = (g * gidx<LOGN, G::NP - 1>(tr, c + e) + off) & (uint32_t)(G::N - 1);  // pi_g
                b[e] = (valid && j == 0) ? (W)hrow[pk[e]] : W(0);
            }
            for (int l = 0; l < level; ++l) {
                const uint64_t *drow = hrow + (size_t)(1 + l) * G::N, *krow = key + (size_t)2 * l * G::N;
                W d[CH], k[CH];
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    d[e] = valid ? (W)drow[pk[e]] : W(0);
                    k[e] = (W)krow[gidx<LOGN, G::NP - 1>(tr, c + e)];
                }
                // a canonical spectrum word times a canonical prepared key: valid Montgomery pair
#pragma unroll
                for (int e = 0; e < CH; ++e) b[e] = hoist_red2q(W(b[e] + A.ar.mont(d[e], k[e])), A.ar);
            }
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                if constexpr (LIN) {
                    const W p = (W)D.pts[(size_t)r * G::N + gidx<LOGN, G::NP - 1>(tr, c + e)];
                    acc[c + e] = hoist_red2q(W(acc[c + e] + A.ar.mont(b[e], p)), A.ar);  // < 2q times canonical
                } else {
                    acc[c + e] = b[e];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // one chunk's loads in flight, not every chunk's
    }
    uint64_t *row = D.out + (((valid ? poly : 0) * (LIN ? 1 : D.count) + (LIN ? 0 : r0)) * 2 + j) * G::N;
    const uint64_t q = A.q64, mu = A.mu64;
    const bool add = LIN && D.accumulate != 0;
    // the stores are fin's own: with `accumulate` a lane reads the word it then overwrites
    inv_poly_from_regs<LOGN, kPfSingle, false>(lds, acc, tau, nullptr, valid, A, LIN ? A.ninv_r : A.ninv, 0,
                                               [&](uint32_t gi, uint64_t x) -> uint64_t {
                                                   if (valid) {
                                                       if (add) x = addq(x, red_q(row[gi], q, mu), q);
                                                       __builtin_nontemporal_store(x, row + gi);
                                                   }
                                                   return x;
                                               });
}

template <int LOGN, typename W>
static hipError_t hoist_fwd_one(const Plan &p, const NttArgs<W> &A, const uint64_t *ct, uint64_t *hoisted, size_t batch,
                                int level, int base_log) {
    using G = Geo<LOGN>;
    const size_t blocks = (batch + G::P - 1) / G::P;
    if constexpr (sizeof(W) == 4) {
        if (p.lazy) {
            hipLaunchKernelGGL((k_hoist_fwd<LOGN, W, true>), dim3((unsigned)blocks), dim3(G::THREADS), 0, p.stream, ct,
                               hoisted, batch, level, base_log, A);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_hoist_fwd<LOGN, W, false>), dim3((unsigned)blocks), dim3(G::THREADS), 0, p.stream, ct, hoisted,
                       batch, level, base_log, A);
    return hipGetLastError();
}
template <int LOGN, typename W>
static hipError_t hoist_apply_one(const Plan &p, const NttArgs<W> &A, bool lin, const HoistArgs &D) {
    using G = Geo<LOGN>;
    const size_t blocks = (D.batch + G::P - 1) / G::P;
    if (lin)
        hipLaunchKernelGGL((k_hoist_apply<LOGN, W, true>), dim3((unsigned)blocks, 1, 2), dim3(G::THREADS), 0, p.stream, D, A);
    else
        hipLaunchKernelGGL((k_hoist_apply<LOGN, W, false>), dim3((unsigned)blocks, D.count, 2), dim3(G::THREADS), 0,
                           p.stream, D, A);
    return hipGetLastError();
}

template <typename W>
static hipError_t hoist_dispatch(const Plan &p, const NttArgs<W> &A, int op, const HoistArgs &D, const uint64_t *ct,
                                 uint64_t *hoisted, int base_log) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return op == 0 ? hoist_fwd_one<L, W>(p, A, ct, hoisted, D.batch, D.level, base_log) \
                           : hoist_apply_one<L, W>(p, A, op == 2, D);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}
static hipError_t hoist_any(const Plan &p, int op, const HoistArgs &D, const uint64_t *ct, uint64_t *hoisted,
                            int base_log) {
    if (p.wide || p.logn > (uint32_t)kMaxFusedLogN || p.logn < (uint32_t)kMinLogN || D.level < 1) return hipErrorInvalidValue;
    if (D.batch == 0) return hipSuccess;
    if (op != 0 && (D.count == 0 || D.count > kHoistMaxCount)) return hipErrorInvalidValue;
    if (p.word == 32) return hoist_dispatch<uint32_t>(p, p.a32, op, D, ct, hoisted, base_log);
    return hoist_dispatch<uint64_t>(p, p.a64, op, D, ct, hoisted, base_log);
}

hipError_t launch_hoist_fwd(const Plan &p, int level, int base_log, const uint64_t *ct, uint64_t *hoisted, size_t batch) {
    HoistArgs D{};
    D.batch = batch;
    D.level = level;
    return hoist_any(p, 0, D, ct, hoisted, base_log);
}
hipError_t launch_hoist_apply(const Plan &p, int level, const uint32_t *tab, uint32_t count, const uint64_t *key,
                              const uint64_t *pts, const uint64_t *hoisted, int accumulate, uint64_t *out, size_t batch) {
    const HoistArgs D{hoisted, key, pts, tab, out, batch, count, level, accumulate};
    return hoist_any(p, pts ? 2 : 1, D, nullptr, nullptr, 0);
}

// ---------------------------------------------------------------- (g, key index) table
// gs / key_idx are host arrays, a handful per call: they travel as kernel
// arguments, kHoistTabChunk entries per launch, so the host arrays are free
// when the call returns and nothing is synchronised.
static constexpr int kHoistTabChunk = 64;
struct HoistTabChunk {
    uint32_t e[2 * kHoistTabChunk];
};
__global__ void __launch_bounds__(kHoistTabChunk)
k_hoist_table(HoistTabChunk c, uint32_t *__restrict__ tab, uint32_t count) {
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    tab[2 * i] = c.e[2 * i];
    tab[2 * i + 1] = c.e[2 * i + 1];
}
hipError_t launch_hoist_table(const uint32_t *gs, const uint32_t *key_idx, size_t count, uint32_t *tab, hipStream_t s) {
    for (size_t i0 = 0; i0 < count; i0 += kHoistTabChunk) {
        const size_t nb = count - i0 < (size_t)kHoistTabChunk ? count - i0 : (size_t)kHoistTabChunk;
        HoistTabChunk c = {};
        for (size_t i = 0; i < nb; ++i) {
            c.e[2 * i] = gs[i0 + i];
            c.e[2 * i + 1] = key_idx ? key_idx[i0 + i] : (uint32_t)(i0 + i);
        }
        hipLaunchKernelGGL(k_hoist_table, dim3(1), dim3(kHoistTabChunk), 0, s, c, tab + 2 * i0, (uint32_t)nb);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- composed path
static constexpr int kHoistBlock = 256;
static unsigned hoist_grid(size_t work) {
    const size_t cap = 256 * 16, g = (work + kHoistBlock - 1) / kHoistBlock;  // 256 CUs x 16 blocks: grid-stride beyond
    return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}
// ct [batch][2][n] -> rows [batch][1 + level][n]: c0's raw words (the forward
// transform reduces them) and the digits of c1 mod q
__global__ void __launch_bounds__(kHoistBlock)
k_hoist_digits(const uint64_t *__restrict__ ct, uint64_t *__restrict__ rows, uint32_t logn, size_t batch,
               uint32_t base_log, uint32_t level, ModConsts m) {
    const size_t total = batch << logn, n = (size_t)1 << logn;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint64_t mask = (1ull << base_log) - 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i >> logn, k = i & (n - 1);
        const uint64_t *src = ct + ((2 * b) << logn) + k;
        uint64_t *dst = rows + ((b * (1 + level)) << logn) + k;
        dst[0] = src[0];
        const uint64_t w = red_q(src[n], m.q, m.mu);
        for (uint32_t l = 0; l < level; ++l) dst[(size_t)(1 + l) << logn] = (w >> (l * base_log)) & mask;
    }
}
// x * key / R, canonical, for canonical x and a prepared key word (R = 2^32 for
// 32-bit contexts, else 2^64; word 65: q >= 2^62)
__device__ __forceinline__ uint64_t hoist_mul_key(uint64_t x, uint64_t k, const ModConsts &m, int word) {
    if (word == 32) {
        const uint64_t p = x * k;
        const uint32_t t = (uint32_t)p * (uint32_t)m.qinv;
        const uint64_t r = (p + (uint64_t)t * m.q) >> 32;  // [0, 2q)
        return r >= m.q ? r - m.q : r;
    }
    return wmont(x, k, m.q, m.qinv);
}
// x * p mod q, canonical, for canonical x and p
__device__ __forceinline__ uint64_t hoist_mul(uint64_t x, uint64_t p, const ModConsts &m, int word) {
    if (word == 32) return x * p % m.q;  // q < 2^30
    return wmont(wmont(x, p, m.q, m.qinv), m.r2, m.q, m.qinv);
}
// One lane per spectrum position k of one (ciphertext, rotation) -- LIN: of one
// ciphertext, looping over the terms.  spec [batch][count][2][n] (LIN:
// [batch][2][n]), canonical spectra for the batched inverse.
template <bool LIN>
__global__ void __launch_bounds__(kHoistBlock)
k_hoist_mac(HoistArgs D, uint64_t *__restrict__ spec, uint32_t logn, int word, ModConsts m) {
    const uint32_t n = 1u << logn, per = LIN ? 1u : D.count;
    const size_t total = (D.batch * per) << logn;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t level = (uint32_t)D.level;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t k = (uint32_t)i & (n - 1);
        const size_t br = i >> logn, b = br / per;
        const uint64_t *hrow = D.hoisted + ((b * (1 + level)) << logn);
        uint64_t s0 = 0, s1 = 0;
        const uint32_t r0 = LIN ? 0u : (uint32_t)(br % per), r1 = LIN ? D.count : r0 + 1;
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t g = D.tab[2 * r], pk = (g * k + ((g - 1) >> 1)) & (n - 1);  // pi_g
            const uint64_t *key = D.key + (((size_t)D.tab[2 * r + 1] * level * 2) << logn);
            uint64_t b0 = red_q(hrow[pk], m.q, m.mu), b1 = 0;
            for (uint32_t l = 0; l < level; ++l) {
                const uint64_t d = red_q(hrow[((size_t)(1 + l) << logn) + pk], m.q, m.mu);
                const uint64_t *krow = key + ((size_t)(2 * l) << logn);
                b0 = wadd(b0, hoist_mul_key(d, krow[n + k], m, word), m.q);
                b1 = wadd(b1, hoist_mul_key(d, krow[k], m, word), m.q);
            }
            if constexpr (LIN) {
                const uint64_t p = red_q(D.pts[((size_t)r << logn) + k], m.q, m.mu);
                s0 = wadd(s0, hoist_mul(b0, p, m, word), m.q);
                s1 = wadd(s1, hoist_mul(b1, p, m, word), m.q);
            } else {
                s0 = b0;
                s1 = b1;
            }
        }
        uint64_t *o = spec + ((2 * br) << logn) + k;
        o[0] = s0;
        o[n] = s1;
    }
}

hipError_t launch_hoist_digits(const ModConsts &m, uint32_t logn, uint32_t base_log, uint32_t level, const uint64_t *ct,
                               uint64_t *rows, size_t batch, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (logn < 2 || logn > (uint32_t)kMaxLogN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hoist_digits, dim3(hoist_grid(batch << logn)), dim3(kHoistBlock), 0, s, ct, rows, logn, batch,
                       base_log, level, m);
    return hipGetLastError();
}
hipError_t launch_hoist_mac(const ModConsts &m, uint32_t logn, int word, int level, const uint32_t *tab, uint32_t count,
                            const uint64_t *key, const uint64_t *pts, const uint64_t *hoisted, uint64_t *spec, size_t batch,
                            hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (logn < 2 || logn > (uint32_t)kMaxLogN || level < 1 || count == 0 || count > kHoistMaxCount)
        return hipErrorInvalidValue;
    const HoistArgs D{hoisted, key, pts, tab, nullptr, batch, count, level, 0};
    if (pts)
        hipLaunchKernelGGL(k_hoist_mac<true>, dim3(hoist_grid(batch << logn)), dim3(kHoistBlock), 0, s, D, spec, logn, word, m);
    else
        hipLaunchKernelGGL(k_hoist_mac<false>, dim3(hoist_grid((batch * count) << logn)), dim3(kHoistBlock), 0, s, D, spec,
                           logn, word, m);
    return hipGetLastError();
}

}  // namespace FHE_NS
