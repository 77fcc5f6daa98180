// tally.hip -- segmented sum of ciphertexts in one HBM pass.
//
//   k_ct_sum : out[g][w] = sum_{i<count} (in[g][i][w] mod q) mod q, canonical,
//              w < words = polys N.  EncryptionEngine::batch_add /
//              batch_add_tree (encryption.cpp:1327-1460), tally_votes
//              (:1061-1067) and tally_multi_candidate (:1153-1168): a fold of
//              add() (:700-730), whose coefficients are mod_add
//              (modular_arithmetic.cpp:122-135).  mod_add of canonical residues
//              is associative and commutative, so any order of summation gives
//              the reference's words bit for bit.
//
// Layout: a lane owns one 16-byte column (two u64) of one group's output and
// walks the ballots of its slice, kUnroll non-temporal 16-byte loads in
// flight.  grid = (column blocks, slices, groups): slice blockIdx.y sums
// ballots [y per, (y+1) per) and writes row y of the group's [slices][words]
// partials; a second launch of the same kernel over those rows (contiguous
// form, count = slices) folds them.  Two addressing forms: contiguous
// [groups][count][words], or a device table of `count` pointers (one group),
// read as wave-uniform scalar loads.
//
// Accumulation: the raw words are summed into a 128-bit (hi:lo) integer and
// reduced once per column.  Statically that is 4 VALU per word in the loop as
// compiled for gfx950 (v_lshl_add_u64, v_cmp_lt_u64, v_cndmask, v_lshl_add_u64
// into hi) against about 10 for the reduce-then-mod_add form (compare with q,
// 64-bit add, carry compare, compare with q, 64-bit subtract, two selects, on
// 32-bit halves) plus its divergent slow path for words >= q; either is far
// below what the 16 bytes per lane and ballot cost in HBM time.  The single
// reduction at the end,
// hi 2^64 + lo = wmont(hi, 2^128 mod q) + lo (mod q), is exact for any odd
// q < 2^64 and any count < 2^64 (as lwe.hip's split key-switch sum).
#include "tally_ops.hpp"

namespace FHE_NS {

static constexpr int kBlock = 256;
static constexpr int kUnroll = 8;

// PTR = false: src is [groups][count][words] u64.  PTR = true: src is a table
// of `count` pointers to `words` u64 each (gridDim.z == 1).
template <bool PTR>
__global__ void __launch_bounds__(kBlock)
k_ct_sum(const void *__restrict__ src, uint64_t *__restrict__ out, size_t cols, size_t count, size_t per,
         size_t groups, int accumulate, ModConsts m) {
    const size_t i0 = (size_t)blockIdx.y * per;
    const size_t i1 = i0 + per < count ? i0 + per : count;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t g = blockIdx.z; g < groups; g += gridDim.z) {
        u64x2 *const dst = reinterpret_cast<u64x2 *>(out) + (g * gridDim.y + blockIdx.y) * cols;
        for (size_t col = (size_t)blockIdx.x * kBlock + threadIdx.x; col < cols; col += stride) {
            auto row = [&](size_t i) -> const u64x2 * {
                if (PTR) return reinterpret_cast<const u64x2 *const *>(src)[i] + col;
                return reinterpret_cast<const u64x2 *>(src) + (g * count + i) * cols + col;
            };
            TallyAcc a;
            if (accumulate) a.add(dst[col]);
            size_t i = i0;
            for (; i + kUnroll <= i1; i += kUnroll) {
                u64x2 v[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(row(i + u));
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) a.add(v[u]);
            }
            for (; i < i1; ++i) a.add(__builtin_nontemporal_load(row(i)));
            u64x2 r;
            r.x = fold128(a.hi0, a.lo0, m);
            r.y = fold128(a.hi1, a.lo1, m);
            dst[col] = r;
        }
    }
}

// One pass: `slices` rows per group into out ([groups][slices][cols 2] u64).
hipError_t launch_ct_sum(const ModConsts &m, const void *src, bool ptr_table, uint64_t *out, size_t words, size_t count,
                         size_t per, size_t slices, size_t groups, int accumulate, hipStream_t s) {
    if (words == 0 || count == 0 || groups == 0) return hipSuccess;
    if ((words & 1) || !(m.q & 1) || !slices_ok(count, per, slices, groups, ptr_table, 65535) ||
        (accumulate && slices != 1))
        return hipErrorInvalidValue;
    const size_t cols = words / 2;
    size_t gx = (cols + kBlock - 1) / kBlock;
    if (gx > 65535) gx = 65535;  // grid-stride beyond
    const dim3 grid((unsigned)gx, (unsigned)slices, (unsigned)(groups < 65535 ? groups : 65535));
    if (ptr_table)
        hipLaunchKernelGGL(k_ct_sum<true>, grid, dim3(kBlock), 0, s, src, out, cols, count, per, groups, accumulate, m);
    else
        hipLaunchKernelGGL(k_ct_sum<false>, grid, dim3(kBlock), 0, s, src, out, cols, count, per, groups, accumulate, m);
    return hipGetLastError();
}

// ---------------------------------------------------------------- public integer weights
// k_ct_sum_scaled: out[g][w] = sum_i ((in[g][i][w] mod q) (s[g][i] mod q) mod q)
// mod q -- multiply_scalar per ballot (encryption.cpp:890-902,
// polynomial_ring.cpp:454-473) folded by add(): k_ct_sum with one product per
// word.  The scalar is wave-uniform, so it is reduced and prepared once per
// ballot (k_scalar_prep, or the host for pointer tables and host-resident
// ballots) into a table of 16-byte entries that the kernel reads as scalar
// loads:
//   q < 2^63   {s mod q, floor((s mod q) 2^64 / q)}: mul_scalar's Shoup product
//              (shoup64), exact for raw u64 words;
//   q >= 2^63  {(s mod q) 2^64 mod q, 0}: the word, one conditional subtraction
//              from canonical, times the Montgomery-form scalar by wmont --
//              the canonical product with the carry bit, in place of
//              mul_scalar's 128-step shift-subtract.
// Products are canonical; they are summed and folded as k_ct_sum's words.  A
// prior `out` (accumulate) is one more unscaled term.  The product is scaled1
// (tally_ops.hpp); the choice between its two forms is made once per kernel
// (WIDE), outside every loop: as a branch per word the compiler ran the wmont
// product unconditionally beside the Shoup one.
__global__ void __launch_bounds__(kBlock)
k_scalar_prep(const uint64_t *__restrict__ raw, u64x2 *__restrict__ tab, size_t total, ModConsts m) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const uint64_t s = mod64_slow(raw[i], m.q, m.mu);
    u64x2 e;
    if (m.q >> 63) {
        e.x = wmont(s, m.r2, m.q, m.qinv);
        e.y = 0;
    } else {  // floor(s 2^64 / q) by restoring division (s < q < 2^63: no carry)
        uint64_t r = s, quo = 0;
        for (int b = 0; b < 64; ++b) {
            r <<= 1;
            quo <<= 1;
            if (r >= m.q) {
                r -= m.q;
                quo |= 1;
            }
        }
        e.x = s;
        e.y = quo;
    }
    tab[i] = e;
}

template <bool PTR, bool WIDE>
__device__ __forceinline__ void ct_sum_scaled_body(const void *__restrict__ src, const u64x2 *__restrict__ tab,
                                                   uint64_t *__restrict__ out, size_t cols, size_t count, size_t per,
                                                   size_t groups, int accumulate, const ModConsts &m) {
    const size_t i0 = (size_t)blockIdx.y * per;
    const size_t i1 = i0 + per < count ? i0 + per : count;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t g = blockIdx.z; g < groups; g += gridDim.z) {
        u64x2 *const dst = reinterpret_cast<u64x2 *>(out) + (g * gridDim.y + blockIdx.y) * cols;
        const u64x2 *const sc = tab + g * count;
        for (size_t col = (size_t)blockIdx.x * kBlock + threadIdx.x; col < cols; col += stride) {
            auto row = [&](size_t i) -> const u64x2 * {
                if (PTR) return reinterpret_cast<const u64x2 *const *>(src)[i] + col;
                return reinterpret_cast<const u64x2 *>(src) + (g * count + i) * cols + col;
            };
            auto mul = [&](u64x2 v, size_t i) {
                const u64x2 s = sc[i];
                u64x2 p;
                p.x = scaled1<WIDE>(v.x, s, m);
                p.y = scaled1<WIDE>(v.y, s, m);
                return p;
            };
            TallyAcc a;
            if (accumulate) a.add(dst[col]);
            size_t i = i0;
            for (; i + kUnroll <= i1; i += kUnroll) {
                u64x2 v[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(row(i + u));
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) a.add(mul(v[u], i + u));
            }
            for (; i < i1; ++i) a.add(mul(__builtin_nontemporal_load(row(i)), i));
            u64x2 r;
            r.x = fold128(a.hi0, a.lo0, m);
            r.y = fold128(a.hi1, a.lo1, m);
            dst[col] = r;
        }
    }
}

template <bool PTR>
__global__ void __launch_bounds__(kBlock)
k_ct_sum_scaled(const void *__restrict__ src, const u64x2 *__restrict__ tab, uint64_t *__restrict__ out, size_t cols,
                size_t count, size_t per, size_t groups, int accumulate, ModConsts m) {
    if (m.q >> 63) ct_sum_scaled_body<PTR, true>(src, tab, out, cols, count, per, groups, accumulate, m);
    else ct_sum_scaled_body<PTR, false>(src, tab, out, cols, count, per, groups, accumulate, m);
}

hipError_t launch_scalar_prep(const ModConsts &m, const uint64_t *raw, void *tab, size_t total, hipStream_t s) {
    if (total == 0) return hipSuccess;
    if (!(m.q & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scalar_prep, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, raw,
                       reinterpret_cast<u64x2 *>(tab), total, m);
    return hipGetLastError();
}

hipError_t launch_ct_sum_scaled(const ModConsts &m, const void *src, bool ptr_table, const void *tab, uint64_t *out,
                                size_t words, size_t count, size_t per, size_t slices, size_t groups, int accumulate,
                                hipStream_t s) {
    if (words == 0 || count == 0 || groups == 0) return hipSuccess;
    if ((words & 1) || !(m.q & 1) || !slices_ok(count, per, slices, groups, ptr_table, 65535) ||
        (accumulate && slices != 1))
        return hipErrorInvalidValue;
    const size_t cols = words / 2;
    size_t gx = (cols + kBlock - 1) / kBlock;
    if (gx > 65535) gx = 65535;  // grid-stride beyond
    const dim3 grid((unsigned)gx, (unsigned)slices, (unsigned)(groups < 65535 ? groups : 65535));
    const u64x2 *t = reinterpret_cast<const u64x2 *>(tab);
    if (ptr_table)
        hipLaunchKernelGGL(k_ct_sum_scaled<true>, grid, dim3(kBlock), 0, s, src, t, out, cols, count, per, groups,
                           accumulate, m);
    else
        hipLaunchKernelGGL(k_ct_sum_scaled<false>, grid, dim3(kBlock), 0, s, src, t, out, cols, count, per, groups,
                           accumulate, m);
    return hipGetLastError();
}

}  // namespace FHE_NS
