// dot.hip -- ciphertext inner product: out = sum_i multiply(a_i, b_i), the
// degree-2 sum of EncryptionEngine::tally_weighted_votes
// (encryption.cpp:1069-1110) before its relinearisation, and of any encrypted
// dot product or sum of squares.
//
// The inverse transform is a Z_q-linear map, so on canonical residues
//
//   sum_i multiply(a_i, b_i) = ( inv(sum X0_i Y0_i),
//                                inv(sum (X0_i Y1_i + X1_i Y0_i)),
//                                inv(sum X1_i Y1_i) )
//
// bit for bit (ntt_cipher.hip relies on the same fact for c1): four forward
// transforms per pair, three inverse transforms per slice of pairs, no
// intermediate ciphertexts.
//
//   k_ct_dot     coefficient-form inputs, the fused family (n <= 16384,
//                q < 2^62).  grid = (slices / P, groups): a workgroup owns one
//                slice of one group's pairs (P slices at small n) and loops
//                over them.  Per pair: X0, X1, Y0 are transformed and parked
//                canonical as W words in the slice's workspace row (slots
//                0-2); after the fourth transform (Y1, in registers) the three
//                Montgomery products are added into the NTT-domain
//                accumulators (values in [0, 2q)): VGPRs, or workspace slots
//                3-5 where a lane has no room (ctdot_regacc).  A thread only
//                ever touches its own positions of the slots (the layout of
//                the last forward pass), so they need no synchronisation --
//                the argument of k_ct_mul's slots.  After the last pair the
//                accumulators are inverse-transformed with ninv_r (N^-1 R:
//                removes the Montgomery factor) into the slice's partial row
//                [3][n], canonical.
//                Workspace traffic per coefficient and pair beside the 32 B
//                of input: 3 stash stores + 3 loads = 6 W-words (24 B at
//                32-bit lanes, 48 B at 64-bit); with workspace accumulators 3
//                read-modify-writes more (96 B at 64-bit lanes).
//                Small counts (by_component, gridDim.z == 3): the three sums
//                of a slice on a workgroup each -- 2, 4 and 2 forward
//                transforms per pair and one inverse per workgroup instead of
//                4 and 3 in a row -- so that a few pairs still fill the chip.
//   k_ct_dot_ntt NTT-domain inputs (the reference's multiply with is_ntt runs
//                no transform): a lane owns a 16-byte column and accumulates
//                the three sums of products over its slice, as k_ct_sum does
//                for words.  Products are Montgomery (x 2^-64) and canonical,
//                summed into 128-bit integers, reduced and multiplied by 2^128
//                once per column; exact for any odd q < 2^64.
//
// Both write [groups][slices][3][n] partial rows; launch_ct_sum (tally.hip)
// folds them.
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

// Where the three accumulators live: in VGPRs wherever the workgroup's
// register budget holds them beside a spectrum and its twiddles -- every
// shape but 64-bit lanes at N = 16384 (1024 threads: 128 VGPRs per lane),
// which keeps them in workspace slots 3-5, read-modify-written per pair.
template <int LOGN, typename W>
constexpr bool ctdot_regacc() { return !(sizeof(W) == 8 && Geo<LOGN>::L == 14); }
template <int LOGN, typename W>
constexpr int ctdot_slots() { return ctdot_regacc<LOGN, W>() ? 3 : 6; }

template <int LOGN, typename W, bool LAZY>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS)
k_ct_dot(const void *__restrict__ a, const void *__restrict__ b, int ptr_table, W *__restrict__ ws, uint64_t *dst,
         size_t count, size_t per, size_t slices, size_t groups, NttArgs<W> A) {
    using G = Geo<LOGN>;
    constexpr int LAST = G::NP - 1;
    __shared__ W lds_all[G::P * G::LW];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t slice = (size_t)blockIdx.x * G::P + pl;
    const bool valid = slice < slices;
    if (G::P == 1 && !valid) return;  // whole workgroup: no barrier is skipped
    W *lds = lds_all + pl * G::LW;
    const size_t i0 = slice * per;
    const size_t i1 = i0 + per < count ? i0 + per : count;
    // a fresh opaque copy of the lane index per phase (as k_ct_mul): no
    // phase's address arithmetic stays live across the next transform
    auto lane = [&]() {
        uint32_t t = tau;
        asm volatile("" : "+v"(t));
        return t;
    };
    // gridDim.z == 3: the three components of a slice's sum on a workgroup
    // each (small counts, where whole pairs would leave most of the chip
    // idle): 2, 4 and 2 forward transforms per pair and one inverse instead of
    // 4 and 3 in a row.  Component c parks its spectrum in slot c and
    // accumulates in slot 3 + c: the three workgroups share no word.
    const int comp = gridDim.z == 3 ? (int)blockIdx.z : -1;
    const int nsteps = comp < 0 || comp == 1 ? 4 : 2;
    constexpr bool RA = ctdot_regacc<LOGN, W>();
    W v[G::E];
    // register accumulators, values in [0, 2q); by component only acc0 is used
    W acc0[RA ? G::E : 1], acc1[RA ? G::E : 1], acc2[RA ? G::E : 1];
    for (size_t g = blockIdx.y; g < groups; g += gridDim.y) {
        // slots 0-2: X0, X1, Y0 of the current pair; 3-5: the accumulators
        // (!RA).  Dereferenced only when valid.
        W *slot = ws + (g * slices + slice) * ctdot_slots<LOGN, W>() * G::N;
        if constexpr (RA) {
#pragma unroll
            for (int e = 0; e < G::E; ++e) acc0[e] = acc1[e] = acc2[e] = W(0);
        }
        uint64_t *orow = dst + (g * slices + slice) * 3 * G::N;
        // every polynomial of the workgroup runs `per` rounds (the barriers
        // are workgroup-wide); rounds past a slice's end load zeros and
        // store nothing
        for (size_t k = 0; k < per; ++k) {
            const size_t i = i0 + k;
            const bool ok = valid && i < i1;
            if (G::P == 1 && !ok) break;
            const uint64_t *xr = nullptr, *yr = nullptr;
            if (ok) {
                if (ptr_table) {
                    xr = reinterpret_cast<const uint64_t *const *>(a)[i];
                    yr = reinterpret_cast<const uint64_t *const *>(b)[i];
                } else {
                    xr = reinterpret_cast<const uint64_t *>(a) + (g * count + i) * 2 * G::N;
                    yr = reinterpret_cast<const uint64_t *>(b) + (g * count + i) * 2 * G::N;
                }
            }
            // One forward transform per step (one instance of the transform
            // code for every step), then the step's action on the spectrum
            // in registers.  Source polynomials 0-3 = x0, x1, y0, y1:
            //   whole pair   x0 x1 y0 -> slots 0 1 2,  y1: all three sums
            //   component 0  x0 -> slot 0,  y0: sum 0
            //   component 1  x0 -> slot 1,  y1: sum 1,  x1 -> slot 1,  y0: sum 1
            //   component 2  x1 -> slot 2,  y1: sum 2
#pragma unroll 1
            for (int st = 0; st < nsteps; ++st) {
                const int sp = comp < 0 ? st : comp == 0 ? 2 * st : comp == 2 ? 1 + 2 * st : (0x2130 >> (4 * st)) & 3;
                const uint64_t *src = ((sp & 2) ? yr : xr) + (sp & 1) * G::N;
                const uint32_t tp = lane();
                fwd_poly<LOGN, LAZY, kPfPolymul>(lds, v, tp, src, ok, A);
                if (comp < 0 && st == 3) {
                    if (ok) {
#pragma unroll
                        for (int e = 0; e < G::E; ++e) {
                            W *s = slot + gidx<LOGN, LAST>(tp, e);
                            const W y1 = v[e];
                            const W x0 = s[0], x1 = s[G::N], y0 = s[2 * G::N];
                            W p0 = A.ar.mont(x0, y0);
                            W p1 = A.ar.red2q(A.ar.mont(x0, y1) + A.ar.mont(x1, y0));
                            W p2 = A.ar.mont(x1, y1);
                            if constexpr (RA) {
                                acc0[e] = A.ar.red2q(p0 + acc0[e]);
                                acc1[e] = A.ar.red2q(p1 + acc1[e]);
                                acc2[e] = A.ar.red2q(p2 + acc2[e]);
                            } else {
                                if (k > 0) {
                                    p0 = A.ar.red2q(p0 + s[3 * G::N]);
                                    p1 = A.ar.red2q(p1 + s[4 * G::N]);
                                    p2 = A.ar.red2q(p2 + s[5 * G::N]);
                                }
                                s[3 * G::N] = p0;
                                s[4 * G::N] = p1;
                                s[5 * G::N] = p2;
                                // four coefficients' slot words in flight at a time
                                if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                } else if (comp >= 0 && (st & 1)) {
                    if (ok) {
                        const bool fresh = k == 0 && st == 1;
                        W *acc = slot + (size_t)(3 + comp) * G::N;
#pragma unroll
                        for (int e = 0; e < G::E; ++e) {
                            const uint32_t gi = gidx<LOGN, LAST>(tp, e);
                            W p = A.ar.mont(slot[(size_t)comp * G::N + gi], v[e]);
                            if constexpr (RA) {
                                acc0[e] = A.ar.red2q(p + acc0[e]);
                            } else {
                                if (!fresh) p = A.ar.red2q(p + acc[gi]);
                                acc[gi] = p;
                            }
                        }
                    }
                } else {
                    W *s = slot + (size_t)(comp < 0 ? st : comp) * G::N;
#pragma unroll
                    for (int e = 0; e < G::E; ++e) {
                        const W x = fwd_to_canon<LAZY>(v[e], A);
                        if (ok) s[gidx<LOGN, LAST>(tp, e)] = x;
                    }
                }
                __syncthreads();  // the exchange buffer is free for the next transform
            }
        }
#pragma unroll 1
        for (int r = comp < 0 ? 0 : comp; r <= (comp < 0 ? 2 : comp); ++r) {
            const uint32_t tp = lane();
            if constexpr (RA) {
#pragma unroll
                for (int e = 0; e < G::E; ++e) v[e] = (comp >= 0 || r == 0) ? acc0[e] : r == 1 ? acc1[e] : acc2[e];
            } else {
                const W *s = slot + (size_t)(3 + r) * G::N;
#pragma unroll
                for (int e = 0; e < G::E; ++e) v[e] = valid ? s[gidx<LOGN, LAST>(tp, e)] : W(0);
            }
            inv_poly_from_regs<LOGN, kPfPolymul>(lds, v, tp, orow + (size_t)r * G::N, valid, A, A.ninv_r);
            __syncthreads();
        }
    }
}

// Slices one launch keeps resident: workgroups per CU (occupancy query, once
// per instantiation) x CUs x slices per workgroup.
template <int LOGN, typename W, bool LAZY>
static size_t ctdot_resident(const Plan &p) {
    static int per_cu = 0;
    if (per_cu == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_ct_dot<LOGN, W, LAZY>, Geo<LOGN>::THREADS, 0) !=
                hipSuccess ||
            nb < 1)
            nb = 1;
        per_cu = nb;
    }
    return (size_t)per_cu * (size_t)(p.cus > 0 ? p.cus : 256) * Geo<LOGN>::P;
}

struct DotLaunch {
    const void *a, *b;
    int ptr_table;
    void *ws;
    uint64_t *dst;
    size_t count, per, slices, groups;
    int by_component;  // three workgroups per slice (gridDim.z == 3)
    size_t *resident;  // non-null: query only
    int *ws_slots;     // non-null: query only
};

template <int LOGN, typename W, bool LAZY>
static hipError_t ctdot_go(const Plan &p, const NttArgs<W> &A, const DotLaunch &d) {
    using G = Geo<LOGN>;
    if (d.resident) {
        *d.resident = ctdot_resident<LOGN, W, LAZY>(p);
        return hipSuccess;
    }
    const size_t gx = (d.slices + G::P - 1) / G::P;
    const dim3 grid((unsigned)gx, (unsigned)(d.groups < 65535 ? d.groups : 65535), d.by_component ? 3 : 1);
    hipLaunchKernelGGL((k_ct_dot<LOGN, W, LAZY>), grid, dim3(G::THREADS), 0, p.stream, d.a, d.b, d.ptr_table,
                       reinterpret_cast<W *>(d.ws), d.dst, d.count, d.per, d.slices, d.groups, A);
    return hipGetLastError();
}

template <int LOGN, typename W>
static hipError_t ctdot_one(const Plan &p, const NttArgs<W> &A, const DotLaunch &d) {
    // 32-bit lanes at N = 8192 / 16384: 32 coefficients per thread (as
    // k_ct_mul2), 256 / 512 threads, so that a lane has the VGPRs for the
    // three accumulators
    constexpr int K = sizeof(W) == 4 && (LOGN == 13 || LOGN == 14) ? gk(LOGN, 5) : LOGN;
    if (d.ws_slots) {
        *d.ws_slots = ctdot_slots<K, W>();
        return hipSuccess;
    }
    if constexpr (sizeof(W) == 4) {
        if (p.lazy) return ctdot_go<K, W, true>(p, A, d);
    }
    return ctdot_go<K, W, false>(p, A, d);
}

template <typename W>
static hipError_t ctdot_dispatch(const Plan &p, const NttArgs<W> &A, const DotLaunch &d) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return ctdot_one<L, W>(p, A, d);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

static hipError_t ctdot_any(const Plan &p, const DotLaunch &d) {
    if (p.wide || (int)p.logn > kMaxFusedLogN) return hipErrorInvalidValue;
    if (p.word == 32) return ctdot_dispatch<uint32_t>(p, p.a32, d);
    return ctdot_dispatch<uint64_t>(p, p.a64, d);
}

size_t ct_dot_resident(const Plan &p) {
    size_t r = 0;
    DotLaunch d{};
    d.resident = &r;
    return ctdot_any(p, d) == hipSuccess && r ? r : 1;
}

size_t ct_dot_ws_bytes(const Plan &p, size_t slices, size_t groups) {
    int slots = 6;
    DotLaunch d{};
    d.ws_slots = &slots;
    (void)ctdot_any(p, d);
    return groups * slices * slots * ((size_t)1 << p.logn) * (p.word == 32 ? 4 : 8);
}

hipError_t launch_ct_dot(const Plan &p, const void *a, const void *b, bool ptr_table, void *ws, uint64_t *dst,
                         size_t count, size_t per, size_t slices, size_t groups, bool by_component) {
    if (count == 0 || groups == 0) return hipSuccess;
    if (!slices_ok(count, per, slices, groups, ptr_table, (size_t)1 << 30)) return hipErrorInvalidValue;
    DotLaunch d{a, b, ptr_table ? 1 : 0, ws, dst, count, per, slices, groups, by_component ? 1 : 0, nullptr, nullptr};
    return ctdot_any(p, d);
}

// ---------------------------------------------------------------- NTT domain
static constexpr int kBlock = 256;
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct DotAcc {
    uint64_t lo = 0, hi = 0;
    __device__ __forceinline__ void add(uint64_t x) {
        lo += x;
        hi += lo < x;
    }
    // (hi 2^64 + lo) 2^64 mod q: the sum of Montgomery products back to plain
    __device__ __forceinline__ uint64_t fold(const ModConsts &m) const {
        uint64_t l = mod64_slow(lo, m.q, m.mu);
        if (hi) l = wadd(wmont(mod64_slow(hi, m.q, m.mu), m.r2, m.q, m.qinv), l, m.q);  // hi 2^64 mod q
        return wmont(l, m.r2, m.q, m.qinv);
    }
};

__global__ void __launch_bounds__(kBlock)
k_ct_dot_ntt(const void *__restrict__ a, const void *__restrict__ b, int ptr_table, uint64_t *__restrict__ dst,
             size_t half, size_t count, size_t per, size_t groups, ModConsts m) {
    const size_t i0 = (size_t)blockIdx.y * per;
    const size_t i1 = i0 + per < count ? i0 + per : count;
    const size_t stride = (size_t)gridDim.x * kBlock;
    auto red = [&](uint64_t x) { return x < m.q ? x : mod64_slow(x, m.q, m.mu); };
    for (size_t g = blockIdx.z; g < groups; g += gridDim.z) {
        u64x2 *const row = reinterpret_cast<u64x2 *>(dst) + (g * gridDim.y + blockIdx.y) * 3 * half;
        for (size_t col = (size_t)blockIdx.x * kBlock + threadIdx.x; col < half; col += stride) {
            DotAcc c[3][2];
#pragma unroll 2
            for (size_t i = i0; i < i1; ++i) {
                const u64x2 *x, *y;
                if (ptr_table) {
                    x = reinterpret_cast<const u64x2 *const *>(a)[i];
                    y = reinterpret_cast<const u64x2 *const *>(b)[i];
                } else {
                    x = reinterpret_cast<const u64x2 *>(a) + (g * count + i) * 2 * half;
                    y = reinterpret_cast<const u64x2 *>(b) + (g * count + i) * 2 * half;
                }
                const u64x2 x0 = __builtin_nontemporal_load(x + col), x1 = __builtin_nontemporal_load(x + half + col);
                const u64x2 y0 = __builtin_nontemporal_load(y + col), y1 = __builtin_nontemporal_load(y + half + col);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint64_t p0 = red(j ? x0.y : x0.x), p1 = red(j ? x1.y : x1.x);
                    const uint64_t r0 = red(j ? y0.y : y0.x), r1 = red(j ? y1.y : y1.x);
                    c[0][j].add(wmont(p0, r0, m.q, m.qinv));
                    c[1][j].add(wmont(p0, r1, m.q, m.qinv));
                    c[1][j].add(wmont(p1, r0, m.q, m.qinv));
                    c[2][j].add(wmont(p1, r1, m.q, m.qinv));
                }
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                u64x2 o;
                o.x = c[r][0].fold(m);
                o.y = c[r][1].fold(m);
                row[(size_t)r * half + col] = o;
            }
        }
    }
}

hipError_t launch_ct_dot_ntt(const ModConsts &m, const void *a, const void *b, bool ptr_table, uint64_t *dst, uint32_t n,
                             size_t count, size_t per, size_t slices, size_t groups, hipStream_t s) {
    if (count == 0 || groups == 0) return hipSuccess;
    if ((n & 1) || !(m.q & 1) || !slices_ok(count, per, slices, groups, ptr_table, 65535)) return hipErrorInvalidValue;
    const size_t half = n / 2;
    const dim3 grid((unsigned)((half + kBlock - 1) / kBlock), (unsigned)slices, (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(k_ct_dot_ntt, grid, dim3(kBlock), 0, s, a, b, ptr_table ? 1 : 0, dst, half, count, per, groups, m);
    return hipGetLastError();
}

}  // namespace FHE_NS
