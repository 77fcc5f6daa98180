// threshold.hip -- threshold decryption (KeyManager::generate_threshold_keys,
// partial_decrypt, combine_partial_decryptions; key_manager.cpp:479-636),
// batched over ciphertexts.
//
//   k_partial_dec      partials[s][b] = inv(fwd(c1_b) (.) S_s) for every local
//                      share s: partial_decrypt's polymul (:584-601) with the
//                      share's transform prepared once (S_s = fwd(share) R) and
//                      ONE forward transform per ciphertext for all shares.
//   k_combine_partials phase = c0 - sum_i partials[i] lambda_i (:623-635, then
//                      decrypt's c0 - .), decoded and noise-measured as
//                      fhe_decrypt_batch does, in one streaming pass.
//   k_shamir_shares    share_i = sum_k coeffs[k] i^k, i = 1..total (:511-526).
//
// Every intermediate is a canonical residue and every step is exact over Z_q,
// so the words are the reference chain's bit for bit.
#include "engine_kernels.hpp"
#include "tally_ops.hpp"

namespace FHE_NS {

// ---------------------------------------------------------------- partial decryption
// One workgroup per ciphertext (Geo::P per workgroup at small N), as k_encrypt.
// c1 is read in place from ct [batch][2][N].  The spectrum fwd(c1) has to
// outlive every inverse transform but the last; it waits where k_encrypt's
// second product waits (eng_stash): 0 in VGPRs, 1 in a second LDS region, 2 in
// the output row of the LAST share, W words at this thread's own positions --
// that row is stored last, behind a barrier that follows its reads.  A single
// share needs no stash at all (MULTI = false: the product goes straight from
// the forward transform's registers into the inverse).
struct PdArgs {
    const uint64_t *ct;      // [batch][2][N]
    const uint64_t *shares;  // prepared rows [nshares][N]
    uint64_t *out;           // block s at out + s stride: [batch][N]
    size_t stride, batch;
    uint32_t nshares;
};

// Waves per SIMD: k_encrypt's, except where the spectrum waits in VGPRs
// (N < 32, no LDS at all): two register copies of the polynomial beside the
// transform spill at the 64 VGPRs of 8 waves (32-bit words) and at the 128 of
// 4 (64-bit words).
template <int LOGN, typename W>
constexpr int pd_occ() {
    if (eng_stash<LOGN, W>() == 0) return sizeof(W) == 8 ? 2 : 4;
    return eng_occ<LOGN, W>();
}

template <int LOGN, typename W, bool LAZY, bool MULTI>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, (pd_occ<LOGN, W>()))
k_partial_dec(PdArgs E, NttArgs<W> A) {
    using G = Geo<LOGN>;
    constexpr int STASH = eng_stash<LOGN, W>();
    __shared__ W lds_all[G::P * G::LW + (STASH == 1 ? G::P * G::N : 0)];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < E.batch;
    if (G::P == 1 && !valid) return;
    W *lds = lds_all + pl * G::LW;
    W *st = lds_all + G::P * G::LW + pl * G::N;
    const size_t row = (valid ? poly : 0) * G::N;
    const uint32_t last = MULTI ? E.nshares - 1 : 0;
    W *park = reinterpret_cast<W *>(E.out + (size_t)last * E.stride + row);
    W v[G::E];
    W sp[STASH == 0 ? G::E : 1];
    fwd_poly<LOGN, LAZY>(lds, v, tau, E.ct + 2 * row + G::N, valid, A);
    if constexpr (MULTI) {
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const uint32_t gi = gidx<LOGN, G::NP - 1>(tau, e);
            if constexpr (STASH == 0) sp[e] = v[e];
            else if constexpr (STASH == 1) st[gi] = v[e];
            else if (valid) park[gi] = v[e];
        }
    }
    for (uint32_t s = 0; s <= last; ++s) {
        uint32_t ts = tau;
        asm volatile("" : "+v"(ts));
        const uint64_t *key = E.shares + (size_t)s * G::N;
#pragma unroll
        for (int e = 0; e < G::E; ++e) {
            const uint32_t gi = gidx<LOGN, G::NP - 1>(ts, e);
            W x;
            if constexpr (!MULTI) x = v[e];
            else if constexpr (STASH == 0) x = sp[e];
            else if constexpr (STASH == 1) x = st[gi];
            else x = valid ? park[gi] : W(0);
            v[e] = valid ? A.ar.mont(x, (W)key[gi]) : W(0);  // fwd(c1) . S_s, [0, 2q)
            // u64: 4 stash and key words in flight at a time (as k_ct_sq)
            if (sizeof(W) == 8 && (e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        // exchange buffer reuse; s == last: every parked word is read before the row's stores
        if constexpr (G::NP > 1 || STASH == 2) __syncthreads();
        inv_poly_from_regs<LOGN>(lds, v, ts, E.out + (size_t)s * E.stride + row, valid, A, A.ninv);
        if constexpr (G::NP > 1) __syncthreads();
    }
}

template <int LOGN, typename W, bool LAZY>
static hipError_t pd_one(const NttArgs<W> &A, hipStream_t s, const PdArgs &E) {
    using G = Geo<LOGN>;
    const dim3 grid((E.batch + G::P - 1) / G::P), block(G::THREADS);
    if (E.nshares > 1) hipLaunchKernelGGL((k_partial_dec<LOGN, W, LAZY, true>), grid, block, 0, s, E, A);
    else hipLaunchKernelGGL((k_partial_dec<LOGN, W, LAZY, false>), grid, block, 0, s, E, A);
    return hipGetLastError();
}
template <int LOGN, typename W>
static hipError_t pd_lazy(const Plan &p, const NttArgs<W> &A, const PdArgs &E) {
    if constexpr (sizeof(W) == 4)
        if (p.lazy) return pd_one<LOGN, W, true>(A, p.stream, E);
    return pd_one<LOGN, W, false>(A, p.stream, E);
}
template <typename W>
static hipError_t pd_dispatch(const Plan &p, const NttArgs<W> &A, const PdArgs &E) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return pd_lazy<L, W>(p, A, E);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_partial_dec(const Plan &p, const uint64_t *shares_prep, size_t nshares, const uint64_t *ct,
                              uint64_t *partials, size_t share_stride, size_t batch) {
    if (batch == 0 || nshares == 0) return hipSuccess;
    if (nshares > 0xffffffffull) return hipErrorInvalidValue;
    const PdArgs E{ct, shares_prep, partials, share_stride, batch, (uint32_t)nshares};
    if (p.word == 32) return pd_dispatch<uint32_t>(p, p.a32, E);
    return pd_dispatch<uint64_t>(p, p.a64, E);
}

// ---------------------------------------------------------------- scalar tables
// lambda_i and the evaluation points are host values, a handful per call: they
// are prepared on the host (scalar_entry) and written to the device table by a
// kernel that carries them as arguments, kTabChunk entries per launch.
static constexpr int kTabChunk = 64;
struct TabChunk {
    uint64_t e[2 * kTabChunk];
};
__global__ void __launch_bounds__(kTabChunk)
k_scalar_table(TabChunk c, u64x2 *__restrict__ tab, uint32_t count) {
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    u64x2 x;
    x.x = c.e[2 * i];
    x.y = c.e[2 * i + 1];
    tab[i] = x;
}

hipError_t launch_scalar_table(uint64_t q, const uint64_t *raw, size_t count, void *tab, hipStream_t s) {
    for (size_t i0 = 0; i0 < count; i0 += kTabChunk) {
        const size_t nb = count - i0 < (size_t)kTabChunk ? count - i0 : (size_t)kTabChunk;
        TabChunk c = {};
        for (size_t i = 0; i < nb; ++i) scalar_entry(raw[i0 + i], q, &c.e[2 * i]);
        hipLaunchKernelGGL(k_scalar_table, dim3(1), dim3(kTabChunk), 0, s, c, reinterpret_cast<u64x2 *>(tab) + i0,
                           (uint32_t)nb);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- combination
// A lane owns V consecutive words (V = 2: one 16-byte column; V = 1 for
// buffers that are not 16-byte aligned) of the flat [batch][n] index space and
// walks the partials, kCombUnroll loads in flight.  lambda_i is wave-uniform:
// it is reduced and prepared once per partial on the host (scalar_entry) and
// read as a scalar load -- from the kernel's own arguments for up to
// kCombInline partials (INLINE: a small batch is a handful of microseconds of
// device work, and the table's allocation and fill launch cost more than
// that), from a device table beyond.  The canonical products are summed into a 128-bit
// integer and reduced once (fold128), which is the reference's chain of
// (r + term) % q by associativity of canonical mod_add; then
// phase = (c0 mod q) - acc mod q, and decode_packed + the noise distance as
// k_decode computes them (rounded <= t, so one conditional subtraction is its
// % t).
//
// Noise maximum: the lanes of one ciphertext are n / V consecutive lanes, a
// power of two, aligned -- whole waves, or an aligned group within a wave.  A
// shuffle reduction over min(64, n / V) lanes, then one 64-bit atomicMax per
// group into noise[b], which the launch zeroed: the maximum of a set does not
// depend on the order, so the result is exact and deterministic however many
// workgroups share a ciphertext.
static constexpr int kCombBlock = 256;
static constexpr int kCombUnroll = 4;
static constexpr int kCombInline = kCombineInlineLambdas;

struct CombArgs {
    const uint64_t *ct;        // [batch][2][n], c0 only
    const uint64_t *partials;  // block i at partials + i stride: [batch][n]
    const u64x2 *lam;          // [count] prepared lambda_i (count > kCombInline)
    uint64_t lam_inline[2 * kCombInline];  // the same entries for count <= kCombInline
    uint64_t *values, *phase;  // [batch][n], nullable
    unsigned long long *noise; // [batch], nullable, zeroed
    size_t stride, count, total;  // total = batch n / V lanes of work
    uint32_t logn;
    ModConsts m;
    Decoder D;
};

template <int V>
struct Words {
    uint64_t w[V];
};
template <int V>
__device__ __forceinline__ Words<V> ld_words(const uint64_t *p) {
    Words<V> r;
    if constexpr (V == 2) {
        const u64x2 x = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p));
        r.w[0] = x.x;
        r.w[1] = x.y;
    } else {
        r.w[0] = __builtin_nontemporal_load(p);
    }
    return r;
}
template <int V>
__device__ __forceinline__ void st_words(uint64_t *p, const Words<V> &r) {
    if constexpr (V == 2) {
        u64x2 x;
        x.x = r.w[0];
        x.y = r.w[1];
        __builtin_nontemporal_store(x, reinterpret_cast<u64x2 *>(p));
    } else {
        __builtin_nontemporal_store(r.w[0], p);
    }
}

template <int V, bool WIDE, bool INLINE>
__device__ __forceinline__ void combine_body(const CombArgs &E) {
    const ModConsts &m = E.m;
    const size_t stride = (size_t)gridDim.x * kCombBlock;
    const uint32_t logn = E.logn;
    const uint64_t mask = (1ull << logn) - 1;
    const uint32_t lanes_per_ct = (1u << logn) / V;
    const uint32_t group = lanes_per_ct < 64 ? lanes_per_ct : 64;
    // workgroup-uniform trip count: every lane of a wave takes part in the shuffles
    for (size_t base = (size_t)blockIdx.x * kCombBlock; base < E.total; base += stride) {
        const size_t col = base + threadIdx.x;
        const bool active = col < E.total;
        const size_t w = (active ? col : 0) * V;  // flat word index b n + j
        const uint64_t *pw = E.partials + w;
        uint64_t lo[V] = {}, hi[V] = {};
        auto add = [&](const Words<V> &x, size_t i) {
            u64x2 s;
            if constexpr (INLINE) {
                s.x = E.lam_inline[2 * i];
                s.y = E.lam_inline[2 * i + 1];
            } else {
                s = E.lam[i];
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const uint64_t p = scaled1<WIDE>(x.w[k], s, m);
                lo[k] += p;
                hi[k] += lo[k] < p;
            }
        };
        size_t i = 0;
        for (; i + kCombUnroll <= E.count; i += kCombUnroll) {
            Words<V> x[kCombUnroll];
#pragma unroll
            for (int u = 0; u < kCombUnroll; ++u) x[u] = ld_words<V>(pw + (i + u) * E.stride);
#pragma unroll
            for (int u = 0; u < kCombUnroll; ++u) add(x[u], i + u);
        }
        for (; i < E.count; ++i) add(ld_words<V>(pw + i * E.stride), i);
        const Words<V> c0 = ld_words<V>(E.ct + (((w >> logn) << (logn + 1)) | (w & mask)));
        Words<V> ph, val;
        uint64_t local_max = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const uint64_t p = subq(red_q(c0.w[k], m.q, m.mu), fold128(hi[k], lo[k], m), m.q);
            ph.w[k] = p;
            const uint64_t r = E.D.rounded(p);
            val.w[k] = r >= E.D.t ? r - E.D.t : r;
            if (E.noise) {  // k_decode's distance: the reference's int64 arithmetic, wrapping where q >= 2^63
                uint64_t nz = E.D.noise(p, r);
                nz = (int64_t)nz < 0 ? 0ull - nz : nz;
                local_max = nz > local_max ? nz : local_max;
            }
        }
        if (active && E.phase) st_words<V>(E.phase + w, ph);
        if (active && E.values) st_words<V>(E.values + w, val);
        if (E.noise) {
            if (!active) local_max = 0;
            for (uint32_t o = group >> 1; o >= 1; o >>= 1) {
                const uint64_t x = __shfl_xor(local_max, o, 64);
                local_max = x > local_max ? x : local_max;
            }
            if (active && (threadIdx.x & (group - 1)) == 0)
                atomicMax(E.noise + (w >> logn), (unsigned long long)local_max);
        }
    }
}

template <int V, bool INLINE>
__global__ void __launch_bounds__(kCombBlock)
k_combine_partials(CombArgs E) {
    if (E.m.q >> 63) combine_body<V, true, INLINE>(E);
    else combine_body<V, false, INLINE>(E);
}

hipError_t launch_combine_partials(const ModConsts &m, uint64_t t, const uint64_t *ct, const uint64_t *partials,
                                   size_t share_stride, const uint64_t *lambdas, const void *lam, size_t count,
                                   uint64_t *values, uint64_t *phase, uint64_t *max_noise, uint32_t n, size_t batch,
                                   hipStream_t s) {
    if (batch == 0 || (!values && !phase && !max_noise)) return hipSuccess;
    const bool inl = count <= (size_t)kCombInline;
    if (n < 2 || (n & (n - 1)) || !(m.q & 1) || count == 0 || (inl ? !lambdas : !lam)) return hipErrorInvalidValue;
    if (max_noise) {
        hipError_t e = hipMemsetAsync(max_noise, 0, batch * 8, s);
        if (e != hipSuccess) return e;
    }
    uint32_t logn = 0;
    while ((1u << logn) < n) ++logn;
    CombArgs E;
    E.ct = ct;
    E.partials = partials;
    E.lam = inl ? nullptr : reinterpret_cast<const u64x2 *>(lam);
    for (size_t i = 0; i < (size_t)kCombInline; ++i) {
        E.lam_inline[2 * i] = E.lam_inline[2 * i + 1] = 0;
        if (inl && i < count) scalar_entry(lambdas[i], m.q, &E.lam_inline[2 * i]);
    }
    E.values = values;
    E.phase = phase;
    E.noise = reinterpret_cast<unsigned long long *>(max_noise);
    E.stride = share_stride;
    E.count = count;
    E.logn = logn;
    E.m = m;
    E.D = make_decoder(m.q, t);
    const bool vec = !((((uintptr_t)ct | (uintptr_t)partials | (uintptr_t)values | (uintptr_t)phase) & 15) ||
                       (share_stride & 1));
    E.total = batch * n / (vec ? 2 : 1);
    size_t gx = (E.total + kCombBlock - 1) / kCombBlock;
    if (gx > (1u << 20)) gx = 1u << 20;  // grid-stride beyond
    const dim3 grid((unsigned)gx), block(kCombBlock);
    if (vec && inl) hipLaunchKernelGGL((k_combine_partials<2, true>), grid, block, 0, s, E);
    else if (vec) hipLaunchKernelGGL((k_combine_partials<2, false>), grid, block, 0, s, E);
    else if (inl) hipLaunchKernelGGL((k_combine_partials<1, true>), grid, block, 0, s, E);
    else hipLaunchKernelGGL((k_combine_partials<1, false>), grid, block, 0, s, E);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Shamir shares
// A lane owns one coefficient index j and a tile of kShTile evaluation points
// (blockIdx.y): Horner's rule from the highest coefficient polynomial down,
// acc_i = acc_i i + (coeffs[k][j] mod q).  Each coeffs[k][j] is read and
// reduced once per tile, so once in all for up to kShTile shares.  The product
// with the point is scaled1 with the point's prepared entry; every value is a
// canonical residue, so the result is the reference's sum of terms
// coeffs[k][j] i^k mod q.
static constexpr int kShBlock = 256;
static constexpr int kShTile = 8;

template <bool WIDE>
__device__ __forceinline__ void shamir_body(const uint64_t *__restrict__ coeffs, uint32_t threshold, uint32_t total,
                                            const u64x2 *__restrict__ pts, uint64_t *__restrict__ shares, size_t n,
                                            const ModConsts &m) {
    const uint32_t i0 = blockIdx.y * kShTile;
    const size_t stride = (size_t)gridDim.x * kShBlock;
    for (size_t j = (size_t)blockIdx.x * kShBlock + threadIdx.x; j < n; j += stride) {
        uint64_t acc[kShTile];
        const uint64_t top = mod64_slow(coeffs[(size_t)(threshold - 1) * n + j], m.q, m.mu);
#pragma unroll
        for (int u = 0; u < kShTile; ++u) acc[u] = top;
        for (uint32_t k = threshold - 1; k-- > 0;) {
            const uint64_t c = mod64_slow(coeffs[(size_t)k * n + j], m.q, m.mu);
#pragma unroll
            for (int u = 0; u < kShTile; ++u)
                if (i0 + u < total) acc[u] = wadd(scaled1<WIDE>(acc[u], pts[i0 + u], m), c, m.q);
        }
#pragma unroll
        for (int u = 0; u < kShTile; ++u)
            if (i0 + u < total) shares[(size_t)(i0 + u) * n + j] = acc[u];
    }
}

__global__ void __launch_bounds__(kShBlock)
k_shamir_shares(const uint64_t *__restrict__ coeffs, uint32_t threshold, uint32_t total, const u64x2 *__restrict__ pts,
                uint64_t *__restrict__ shares, size_t n, ModConsts m) {
    if (m.q >> 63) shamir_body<true>(coeffs, threshold, total, pts, shares, n, m);
    else shamir_body<false>(coeffs, threshold, total, pts, shares, n, m);
}

hipError_t launch_shamir_shares(const ModConsts &m, const uint64_t *coeffs, uint32_t threshold, uint32_t total,
                                const void *pts, uint64_t *shares, size_t n, hipStream_t s) {
    if (n == 0 || total == 0) return hipSuccess;
    const size_t tiles = ((size_t)total + kShTile - 1) / kShTile;
    if (threshold == 0 || threshold > total || !(m.q & 1) || tiles > 65535) return hipErrorInvalidValue;
    size_t gx = (n + kShBlock - 1) / kShBlock;
    if (gx > 65535) gx = 65535;  // grid-stride beyond
    hipLaunchKernelGGL(k_shamir_shares, dim3((unsigned)gx, (unsigned)tiles), dim3(kShBlock), 0, s, coeffs, threshold, total,
                       reinterpret_cast<const u64x2 *>(pts), shares, n, m);
    return hipGetLastError();
}

}  // namespace FHE_NS
