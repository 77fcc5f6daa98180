// dot_plain.hip -- ciphertext inner product with public plaintext weights:
// out = sum_i multiply_plain(ct_i, p_i) folded by add(), the degree-1 sum
//
//   ( sum_i c0_i (*) p_i,  sum_i c1_i (*) p_i )
//
// of EncryptionEngine::multiply_plain (encryption.cpp:809-852) per ballot
// followed by batch_add (:1327-1460).  The inverse transform is a Z_q-linear
// map (the argument of dot.hip and of ntt_cipher.hip's c1), so on canonical
// residues
//
//   sum_i multiply_plain(ct_i, p_i) = ( inv(sum C0_i P_i), inv(sum C1_i P_i) )
//
// bit for bit: three forward transforms per pair, two inverse transforms per
// slice of pairs, no intermediate ciphertext, no relinearisation key.
//
//   k_ct_dot_plain      coefficient-form ciphertexts, the fused family
//                       (n <= 16384, q < 2^62).  grid = (slices / P, groups)
//                       as k_ct_dot.  Per pair: p is transformed and its
//                       spectrum parked canonical in slot 0 of the slice's
//                       workspace row; c0 and c1 are transformed in turn and
//                       their Montgomery products with the parked word are
//                       added into two NTT-domain accumulators (values in
//                       [0, 2q)): VGPRs, or workspace slots 1-2 where a lane
//                       has no room -- 64-bit lanes at N = 16384, as k_ct_dot.
//                       Two accumulators instead of three do not change that:
//                       at 1024 threads (128 VGPRs) the spectrum, its twiddles
//                       and 64 accumulator registers do not fit, and the
//                       32-coefficient geometry (512 threads, 256 VGPRs) as
//                       compiled for gfx950 spilled 228 VGPRs.  A thread only
//                       touches its own positions of the slots, so they need
//                       no synchronisation.  After the last pair both
//                       accumulators are inverse-transformed with ninv_r into
//                       the slice's partial row [2][n], canonical.
//                       Workspace traffic per coefficient and pair beside the
//                       24 B of input: 1 store + 2 loads of a W word; with
//                       workspace accumulators 2 read-modify-writes more.
//   k_ct_dot_plain_ntt  NTT-domain ciphertexts and result (multiply_plain with
//                       is_ntt, encryption.cpp:819-821: the plaintext is still
//                       coefficient form and is forward-transformed).  p is
//                       transformed times R; the ciphertext words are read in
//                       that transform's last-pass layout, reduced, and the
//                       Montgomery products (plain residues, [0, 2q)) added
//                       into the two accumulators, stored canonical (without
//                       register accumulators the sums live in the partial
//                       row itself).  One forward transform per pair, no
//                       inverse, no workspace.
//
// Both write [groups][slices][2][n] partial rows; launch_ct_sum (tally.hip)
// folds them.  There is no by-component variant: FHE_DOT_COMPONENTS has no
// effect on these kernels.
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

// 32 coefficients per thread where a 16-coefficient lane has no room for the
// two accumulators beside a spectrum: 32-bit lanes at N = 8192 / 16384 (as
// k_ct_dot).
template <int LOGN, typename W>
constexpr int ctdp_key() { return sizeof(W) == 4 && (LOGN == 13 || LOGN == 14) ? gk(LOGN, 5) : LOGN; }
// Where the two accumulators live: VGPRs at every shape but 64-bit lanes at
// N = 16384 (see the head of the file).
template <int LOGN, typename W>
constexpr bool ctdp_regacc() { return !(sizeof(W) == 8 && Geo<LOGN>::L == 14); }
template <int LOGN, typename W>
constexpr int ctdp_slots() { return ctdp_regacc<LOGN, W>() ? 1 : 3; }

template <int LOGN, typename W, bool LAZY, bool NTT>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS)
k_ct_dot_plain(const void *__restrict__ cts, const void *__restrict__ pts, int ptr_table, W *__restrict__ ws,
               uint64_t *dst, size_t count, size_t per, size_t slices, size_t groups, NttArgs<W> A) {
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
    // a fresh opaque copy of the lane index per phase (as k_ct_dot)
    auto lane = [&]() {
        uint32_t t = tau;
        asm volatile("" : "+v"(t));
        return t;
    };
    constexpr bool RA = ctdp_regacc<LOGN, W>();
    W v[G::E];
    W acc0[RA ? G::E : 1], acc1[RA ? G::E : 1];  // values in [0, 2q)
    for (size_t g = blockIdx.y; g < groups; g += gridDim.y) {
        // the parked spectrum of the current plaintext; dereferenced only when valid
        // (slot 0), and without register accumulators the two sums (slots 1, 2)
        W *slot = NTT ? nullptr : ws + (g * slices + slice) * ctdp_slots<LOGN, W>() * G::N;
        if constexpr (RA) {
#pragma unroll
            for (int e = 0; e < G::E; ++e) acc0[e] = acc1[e] = W(0);
        }
        uint64_t *orow = dst + (g * slices + slice) * 2 * G::N;
        // every polynomial of the workgroup runs `per` rounds (the barriers
        // are workgroup-wide); rounds past a slice's end load zeros and
        // store nothing
        for (size_t k = 0; k < per; ++k) {
            const size_t i = i0 + k;
            const bool ok = valid && i < i1;
            if (G::P == 1 && !ok) break;
            const uint64_t *cr = nullptr, *pr = nullptr;
            if (ok) {
                if (ptr_table) {
                    cr = reinterpret_cast<const uint64_t *const *>(cts)[i];
                    pr = reinterpret_cast<const uint64_t *const *>(pts)[i];
                } else {
                    cr = reinterpret_cast<const uint64_t *>(cts) + (g * count + i) * 2 * G::N;
                    pr = reinterpret_cast<const uint64_t *>(pts) + (g * count + i) * G::N;
                }
            }
            if constexpr (NTT) {
                const uint32_t tp = lane();
                fwd_poly<LOGN, LAZY, kPfPolymul, true>(lds, v, tp, pr, ok, A);  // P R: mont(P R, c) = P c
                constexpr int CH = G::E >= 4 ? 4 : G::E;
#pragma unroll
                for (int c0 = 0; c0 < G::E; c0 += CH) {
                    W w0[CH], w1[CH];
                    load_coeffs_r<CH>(w0, A.q64, SlowRed<W>{A}, [&](int e) -> uint64_t {
                        return ok ? __builtin_nontemporal_load(cr + gidx<LOGN, LAST>(tp, c0 + e)) : 0;
                    });
                    load_coeffs_r<CH>(w1, A.q64, SlowRed<W>{A}, [&](int e) -> uint64_t {
                        return ok ? __builtin_nontemporal_load(cr + G::N + gidx<LOGN, LAST>(tp, c0 + e)) : 0;
                    });
#pragma unroll
                    for (int e = 0; e < CH; ++e) {
                        W p0 = A.ar.mont(v[c0 + e], w0[e]), p1 = A.ar.mont(v[c0 + e], w1[e]);
                        if constexpr (RA) {
                            acc0[c0 + e] = A.ar.red2q(p0 + acc0[c0 + e]);
                            acc1[c0 + e] = A.ar.red2q(p1 + acc1[c0 + e]);
                        } else if (ok) {  // the sums live in the partial row, canonical
                            uint64_t *o = orow + gidx<LOGN, LAST>(tp, c0 + e);
                            if (k > 0) {
                                p0 = A.ar.red2q(p0 + (W)o[0]);
                                p1 = A.ar.red2q(p1 + (W)o[G::N]);
                            }
                            o[0] = (uint64_t)A.ar.red1q(p0);
                            o[G::N] = (uint64_t)A.ar.red1q(p1);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                __syncthreads();  // the exchange buffer is free for the next transform
            } else {
                // step 0: p -> slot; steps 1, 2: c0, c1 times the parked word
#pragma unroll 1
                for (int st = 0; st < 3; ++st) {
                    const uint64_t *src = st == 0 ? pr : cr + (size_t)(st - 1) * G::N;
                    const uint32_t tp = lane();
                    fwd_poly<LOGN, LAZY, kPfPolymul>(lds, v, tp, src, ok, A);
                    if (st == 0) {
#pragma unroll
                        for (int e = 0; e < G::E; ++e) {
                            const W x = fwd_to_canon<LAZY>(v[e], A);
                            if (ok) slot[gidx<LOGN, LAST>(tp, e)] = x;
                        }
                    } else if (ok) {
#pragma unroll
                        for (int e = 0; e < G::E; ++e) {
                            W *s = slot + gidx<LOGN, LAST>(tp, e);
                            W p = A.ar.mont(s[0], v[e]);
                            if constexpr (RA) {
                                if (st == 1) acc0[e] = A.ar.red2q(p + acc0[e]);
                                else acc1[e] = A.ar.red2q(p + acc1[e]);
                            } else {
                                if (k > 0) p = A.ar.red2q(p + s[(size_t)st * G::N]);
                                s[(size_t)st * G::N] = p;
                                // four coefficients' slot words in flight at a time
                                if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                    __syncthreads();  // the exchange buffer is free for the next transform
                }
            }
        }
        if constexpr (NTT) {
            if (RA && valid) {
                const uint32_t tp = lane();
#pragma unroll
                for (int e = 0; e < G::E; ++e) {
                    const uint32_t gi = gidx<LOGN, LAST>(tp, e);
                    __builtin_nontemporal_store((uint64_t)A.ar.red1q(acc0[e]), orow + gi);
                    __builtin_nontemporal_store((uint64_t)A.ar.red1q(acc1[e]), orow + G::N + gi);
                }
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < 2; ++r) {
                const uint32_t tp = lane();
#pragma unroll
                for (int e = 0; e < G::E; ++e) {
                    if constexpr (RA) v[e] = r == 0 ? acc0[e] : acc1[e];
                    else v[e] = valid ? slot[(size_t)(1 + r) * G::N + gidx<LOGN, LAST>(tp, e)] : W(0);
                }
                inv_poly_from_regs<LOGN, kPfPolymul>(lds, v, tp, orow + (size_t)r * G::N, valid, A, A.ninv_r);
                __syncthreads();
            }
        }
    }
}

struct DotPlainLaunch {
    const void *cts, *pts;
    int ptr_table;
    void *ws;
    uint64_t *dst;
    size_t count, per, slices, groups;
    size_t *resident;  // non-null: query only
    int *ws_slots;     // non-null: query only
};

// Slices one launch keeps resident: workgroups per CU (occupancy query, once
// per instantiation) x CUs x slices per workgroup.
template <int LOGN, typename W, bool LAZY, bool NTT>
static size_t ctdp_resident(const Plan &p) {
    static int per_cu = 0;
    if (per_cu == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_ct_dot_plain<LOGN, W, LAZY, NTT>, Geo<LOGN>::THREADS,
                                                         0) != hipSuccess ||
            nb < 1)
            nb = 1;
        per_cu = nb;
    }
    return (size_t)per_cu * (size_t)(p.cus > 0 ? p.cus : 256) * Geo<LOGN>::P;
}

template <int LOGN, typename W, bool LAZY, bool NTT>
static hipError_t ctdp_go(const Plan &p, const NttArgs<W> &A, const DotPlainLaunch &d) {
    using G = Geo<LOGN>;
    if (d.resident) {
        *d.resident = ctdp_resident<LOGN, W, LAZY, NTT>(p);
        return hipSuccess;
    }
    const size_t gx = (d.slices + G::P - 1) / G::P;
    const dim3 grid((unsigned)gx, (unsigned)(d.groups < 65535 ? d.groups : 65535));
    hipLaunchKernelGGL((k_ct_dot_plain<LOGN, W, LAZY, NTT>), grid, dim3(G::THREADS), 0, p.stream, d.cts, d.pts,
                       d.ptr_table, reinterpret_cast<W *>(d.ws), d.dst, d.count, d.per, d.slices, d.groups, A);
    return hipGetLastError();
}

template <int LOGN, typename W>
static hipError_t ctdp_one(const Plan &p, const NttArgs<W> &A, const DotPlainLaunch &d, int is_ntt) {
    constexpr int K = ctdp_key<LOGN, W>();
    if (d.ws_slots) {
        *d.ws_slots = ctdp_slots<K, W>();
        return hipSuccess;
    }
    if constexpr (sizeof(W) == 4) {
        if (p.lazy) return is_ntt ? ctdp_go<K, W, true, true>(p, A, d) : ctdp_go<K, W, true, false>(p, A, d);
    }
    return is_ntt ? ctdp_go<K, W, false, true>(p, A, d) : ctdp_go<K, W, false, false>(p, A, d);
}

template <typename W>
static hipError_t ctdp_dispatch(const Plan &p, const NttArgs<W> &A, const DotPlainLaunch &d, int is_ntt) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return ctdp_one<L, W>(p, A, d, is_ntt);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

static hipError_t ctdp_any(const Plan &p, const DotPlainLaunch &d, int is_ntt) {
    if (p.wide || (int)p.logn > kMaxFusedLogN) return hipErrorInvalidValue;
    if (p.word == 32) return ctdp_dispatch<uint32_t>(p, p.a32, d, is_ntt);
    return ctdp_dispatch<uint64_t>(p, p.a64, d, is_ntt);
}

size_t ct_dot_plain_resident(const Plan &p, int is_ntt) {
    size_t r = 0;
    DotPlainLaunch d{};
    d.resident = &r;
    return ctdp_any(p, d, is_ntt) == hipSuccess && r ? r : 1;
}

size_t ct_dot_plain_ws_bytes(const Plan &p, size_t slices, size_t groups) {
    int slots = 3;
    DotPlainLaunch d{};
    d.ws_slots = &slots;
    (void)ctdp_any(p, d, 0);
    return groups * slices * slots * ((size_t)1 << p.logn) * (p.word == 32 ? 4 : 8);
}

hipError_t launch_ct_dot_plain(const Plan &p, const void *cts, const void *pts, bool ptr_table, void *ws, uint64_t *dst,
                               size_t count, size_t per, size_t slices, size_t groups, int is_ntt) {
    if (count == 0 || groups == 0) return hipSuccess;
    if (!slices_ok(count, per, slices, groups, ptr_table, (size_t)1 << 30)) return hipErrorInvalidValue;
    DotPlainLaunch d{cts, pts, ptr_table ? 1 : 0, ws, dst, count, per, slices, groups, nullptr, nullptr};
    return ctdp_any(p, d, is_ntt);
}

}  // namespace FHE_NS
