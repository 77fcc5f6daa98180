// lwe_pack.hip -- the packing key switch: nslots LWE ciphertexts per output
// become ONE RLWE ciphertext (c0, c1) whose phase carries LWE s's message at
// coefficient slots[s] (include/fhe_gpu.h, fhe_lwe_pack_batch).
//
//   W_s[p][k]    = -(sum_e T(s, e, p, k)) + [p == 0, k == 0] b_s      (mod q)
//   T(s, e, p, k) = (d(s, e) * pack_key[e][p][k]) mod 2^64            (key_switch's digit and product)
//   out[p][j]    = sum_s  X^{h_s} W_s  at j: +W_s[p][j - h_s] for j >= h_s, -W_s[p][n + j - h_s] below
//
// The words of fhe_key_switch_batch with out_dim = 2n, a body add, the
// monomial rotation and fhe_ct_sum_batch, without the [batch * nslots][2n]
// rows in between: a thread owns output word (p, j) of CT ciphertexts, walks
// the slots in groups of kPackSlots and the (i, l) entries in chunks of
// kPackElems / (slots x CT), the digits of (chunk, group, tile) staged in LDS
// as in k_ks_acc.
// For slot s it reads key row e at (j - h_s) mod n: a contiguous window with
// one wrap, so the loads stay coalesced, and the slots of a group read the
// same row back to back (the row comes from HBM once per group and tile).
// The sign of a term depends on (s, j) and is fixed per slot and thread: the
// wrapped products are added to (j < h) or subtracted from (j >= h) one
// deferred 96-bit two's-complement sum, the bodies added, reduced once at the
// end.
// FAST = false (q >= 2^63 or base_log > 32): one 64-bit remainder per term and
// canonical running sums, which do not wrap at any q < 2^64.
#include <type_traits>

#include "fhe_internal.hpp"
#include "lwe_ops.hpp"

namespace FHE_NS {

static constexpr int kPackBlock = 256;
static constexpr int kPackElems = 4096;  // digits staged per LDS round: entries x slots of the group x CT
static constexpr int kPackSlots = 4;     // slots per group

struct PackArgs {
    const uint64_t *key;    // [entries][2][n]
    const uint64_t *lwe_a;  // [batch][nslots][in_dim]
    const uint64_t *lwe_b;  // [batch][nslots]
    const uint32_t *tab;    // [nslots] (nslots > kPackInline)
    uint32_t inl[kPackInline];
    uint64_t *out;  // [batch][2][n]
    size_t batch;
    uint32_t logn, nslots, in_dim, level, base_log;
    int accumulate;
    uint64_t q, mu, qinv, r2;
};

// The signed sum of one output word of one ciphertext of the tile.
template <bool FAST>
struct PackAcc;
// 96 bits in two's complement: fewer than 2^31 words below 2^64 each.
template <>
struct PackAcc<true> {
    uint64_t lo = 0;
    int32_t hi = 0;
    __device__ __forceinline__ void add(uint64_t d, uint64_t key, uint64_t, uint64_t) {
        const uint64_t t = d * key;  // mod 2^64, as key_switch's u64 product
        lo += t;
        hi += lo < t ? 1 : 0;
    }
    __device__ __forceinline__ void sub(uint64_t d, uint64_t key, uint64_t, uint64_t) {
        const uint64_t t = d * key;
        hi -= lo < t ? 1 : 0;
        lo -= t;
    }
    __device__ __forceinline__ void add_word(uint64_t w, uint64_t, uint64_t) {
        lo += w;
        hi += lo < w ? 1 : 0;
    }
    // (hi 2^64 + lo) mod q: hi 2^64 = wmont(hi, 2^128 mod q); a negative sum
    // is negated, reduced and negated mod q
    __device__ __forceinline__ uint64_t value(const PackArgs &E) const {
        const bool minus = hi < 0;
        const uint64_t l = minus ? (uint64_t)0 - lo : lo;
        const uint32_t h32 = minus ? (uint32_t)(~hi) + (lo == 0 ? 1u : 0u) : (uint32_t)hi;
        const uint64_t h = wmont(mod64_slow(h32, E.q, E.mu), E.r2, E.q, E.qinv);
        const uint64_t r = wadd(h, mod64_slow(l, E.q, E.mu), E.q);
        return minus && r ? E.q - r : r;
    }
};
template <>
struct PackAcc<false> {
    uint64_t v = 0;
    __device__ __forceinline__ void add(uint64_t d, uint64_t key, uint64_t q, uint64_t mu) {
        v = addq(v, mod64_slow(d * key, q, mu), q);
    }
    __device__ __forceinline__ void sub(uint64_t d, uint64_t key, uint64_t q, uint64_t mu) {
        v = subq(v, mod64_slow(d * key, q, mu), q);
    }
    __device__ __forceinline__ void add_word(uint64_t w, uint64_t q, uint64_t mu) { v = addq(v, red_q(w, q, mu), q); }
    __device__ __forceinline__ uint64_t value(const PackArgs &) const { return v; }
};

template <int CT, bool FAST, bool INLINE>
__global__ void __launch_bounds__(kPackBlock)
k_lwe_pack(PackArgs E) {
    using Dig = typename std::conditional<FAST, uint32_t, uint64_t>::type;
    __shared__ Dig dig[kPackElems];  // [chunk entries][ns][CT]
    __shared__ uint32_t hs[kPackSlots];
    const uint64_t q = E.q, mu = E.mu;
    const uint32_t n = 1u << E.logn, S = E.nslots;
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;  // output word (p, j) = (w / n, w % n)
    const bool live = w < 2 * n;
    const uint32_t p = w >> E.logn, j = w & (n - 1);
    const size_t c0 = (size_t)blockIdx.y * CT;
    const uint32_t entries = E.in_dim * E.level;
    const uint64_t mask = (1ull << E.base_log) - 1;
    PackAcc<FAST> acc[CT];
    for (uint32_t s0 = 0; s0 < S; s0 += kPackSlots) {
        const uint32_t ns = S - s0 < (uint32_t)kPackSlots ? S - s0 : (uint32_t)kPackSlots;
        const uint32_t chunk = (uint32_t)kPackElems / (ns * CT);  // entries per round: 64 at 4 slots x 16, 256 at one slot
        for (uint32_t e0 = 0; e0 < entries; e0 += chunk) {
            const uint32_t ne = entries - e0 < chunk ? entries - e0 : chunk;
            __syncthreads();
            if (e0 == 0 && threadIdx.x < ns) hs[threadIdx.x] = INLINE ? E.inl[s0 + threadIdx.x] : E.tab[s0 + threadIdx.x];
            for (uint32_t t = threadIdx.x; t < ne * ns * CT; t += blockDim.x) {
                const uint32_t c = t % CT, s = (t / CT) % ns, e = t / (CT * ns);
                const uint32_t idx = e0 + e, i = idx / E.level, l = idx % E.level;
                const uint32_t shift = (E.level - 1 - l) * E.base_log;
                dig[t] = c0 + c < E.batch
                                   ? (Dig)((E.lwe_a[((c0 + c) * S + s0 + s) * E.in_dim + i] >> shift) & mask)
                                   : (Dig)0;
            }
            __syncthreads();
            if (!live) continue;
            // slot by slot over the chunk: the window offset and the sign are
            // fixed per slot, the loads of the entries pipeline as in k_ks_acc
            const uint64_t *krow = E.key + (((size_t)e0 * 2 + p) << E.logn);
            for (uint32_t s = 0; s < ns; ++s) {
                const uint32_t h = hs[s];
                const uint64_t *kcol = krow + ((j - h) & (n - 1));
                const Dig *dg = dig + s * CT;
                const uint32_t dstep = ns * CT;
                if (j >= h) {
#pragma unroll 8
                    for (uint32_t e = 0; e < ne; ++e) {
                        const uint64_t key = kcol[(size_t)e * 2 * n];
#pragma unroll
                        for (int c = 0; c < CT; ++c) acc[c].sub(dg[e * dstep + c], key, q, mu);
                    }
                } else {
#pragma unroll 8
                    for (uint32_t e = 0; e < ne; ++e) {
                        const uint64_t key = kcol[(size_t)e * 2 * n];
#pragma unroll
                        for (int c = 0; c < CT; ++c) acc[c].add(dg[e * dstep + c], key, q, mu);
                    }
                }
            }
        }
        // the bodies: + b_s at (p, j) = (0, h_s)
        if (live && p == 0) {
            for (uint32_t s = 0; s < ns; ++s) {
                if (hs[s] != j) continue;
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c0 + c < E.batch) acc[c].add_word(E.lwe_b[(c0 + c) * S + s0 + s], q, mu);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (c0 + c >= E.batch) break;
        uint64_t *o = E.out + (((c0 + c) * 2 + p) << E.logn) + j;
        uint64_t r = acc[c].value(E);
        if (E.accumulate) r = addq(r, red_q(*o, q, mu), q);
        *o = r;
    }
}

// The slot table from a HOST array: the entries travel as kernel arguments,
// kPackTabChunk per launch (no host buffer outlives the call).
static constexpr int kPackTabChunk = 256;
struct PackTabChunk {
    uint32_t h[kPackTabChunk];
};
__global__ void __launch_bounds__(kPackTabChunk)
k_pack_table(PackTabChunk c, uint32_t *__restrict__ tab, uint32_t count) {
    const uint32_t i = threadIdx.x;
    if (i < count) tab[i] = c.h[i];
}

size_t lwe_pack_table_bytes(size_t nslots) { return nslots > (size_t)kPackInline ? nslots * 4 : 0; }

template <int CT, bool FAST>
static hipError_t pack_launch(const PackArgs &E, bool inl, uint32_t n, size_t nb, hipStream_t s) {
    // small grids take 64-thread workgroups: more of them to stream the key
    const size_t tiles = (nb + CT - 1) / CT;
    const unsigned block = (size_t)((2 * n + kPackBlock - 1) / kPackBlock) * tiles >= 256 ? kPackBlock : 64;
    const dim3 grid((2 * n + block - 1) / block, (unsigned)tiles);
    if (inl) hipLaunchKernelGGL((k_lwe_pack<CT, FAST, true>), grid, dim3(block), 0, s, E);
    else hipLaunchKernelGGL((k_lwe_pack<CT, FAST, false>), grid, dim3(block), 0, s, E);
    return hipGetLastError();
}

hipError_t launch_lwe_pack(const ModConsts &m, uint32_t base_log, uint32_t level, uint32_t in_dim,
                           const uint64_t *pack_key, const uint64_t *lwe_a, const uint64_t *lwe_b,
                           const uint32_t *slots, size_t nslots, int accumulate, void *tab, uint64_t *out, uint32_t n,
                           size_t batch, hipStream_t s) {
    if (batch == 0 || nslots == 0) return hipSuccess;
    if (nslots > 0xffffffffull || n == 0 || (n & (n - 1)) || n > (1u << 30)) return hipErrorInvalidValue;
    const bool inl = nslots <= (size_t)kPackInline;
    if (!inl && !tab) return hipErrorInvalidValue;
    PackArgs E;
    E.key = pack_key;
    E.tab = inl ? nullptr : (const uint32_t *)tab;
    for (int i = 0; i < kPackInline; ++i) E.inl[i] = inl && (size_t)i < nslots ? slots[i] : 0;
    if (!inl) {
        for (size_t i0 = 0; i0 < nslots; i0 += kPackTabChunk) {
            const size_t nt = nslots - i0 < (size_t)kPackTabChunk ? nslots - i0 : (size_t)kPackTabChunk;
            PackTabChunk c = {};
            for (size_t i = 0; i < nt; ++i) c.h[i] = slots[i0 + i];
            hipLaunchKernelGGL(k_pack_table, dim3(1), dim3(kPackTabChunk), 0, s, c, (uint32_t *)tab + i0, (uint32_t)nt);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    E.logn = (uint32_t)__builtin_ctz(n);
    E.nslots = (uint32_t)nslots;
    E.in_dim = in_dim;
    E.level = level;
    E.base_log = base_log;
    E.accumulate = accumulate ? 1 : 0;
    E.q = m.q;
    E.mu = m.mu;
    E.qinv = m.qinv;
    E.r2 = m.r2;
    const bool fast = m.fast && base_log <= 32;
    const int ct = !fast ? 4 : batch >= 16 ? 16 : batch >= 4 ? 4 : 1;
    // grid.y <= 65535 tiles per launch
    const size_t per_launch = (size_t)65535 * ct;
    for (size_t b0 = 0; b0 < batch; b0 += per_launch) {
        const size_t nb = batch - b0 < per_launch ? batch - b0 : per_launch;
        E.lwe_a = lwe_a + b0 * nslots * in_dim;
        E.lwe_b = lwe_b + b0 * nslots;
        E.out = out + b0 * 2 * n;
        E.batch = nb;
        const hipError_t e = !fast      ? pack_launch<4, false>(E, inl, n, nb, s)
                             : ct == 16 ? pack_launch<16, true>(E, inl, n, nb, s)
                             : ct == 4  ? pack_launch<4, true>(E, inl, n, nb, s)
                                        : pack_launch<1, true>(E, inl, n, nb, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace FHE_NS
