// tally_ops.hpp -- the word arithmetic shared by the streaming sums
// (tally.hip, threshold.hip): a 128-bit accumulator of raw or canonical words,
// its single reduction, and the product with a prepared scalar_entry.
#pragma once
#include "fhe_internal.hpp"

namespace FHE_NS {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct TallyAcc {
    uint64_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    __device__ __forceinline__ void add(u64x2 v) {
        lo0 += v.x;
        hi0 += lo0 < v.x;
        lo1 += v.y;
        hi1 += lo1 < v.y;
    }
};

__device__ __forceinline__ uint64_t fold128(uint64_t hi, uint64_t lo, const ModConsts &m) {
    const uint64_t l = mod64_slow(lo, m.q, m.mu);
    if (hi == 0) return l;
    const uint64_t h = wmont(mod64_slow(hi, m.q, m.mu), m.r2, m.q, m.qinv);  // hi 2^64 mod q
    return wadd(h, l, m.q);
}

// (x mod q) (s mod q) mod q, canonical, for a raw word x and the table entry
// of s (scalar_entry / k_scalar_prep):
//   q < 2^63   {s mod q, floor((s mod q) 2^64 / q)}: mul_scalar's Shoup product
//              (shoup64), exact for raw u64 words;
//   q >= 2^63  {(s mod q) 2^64 mod q, 0}: the word, one conditional subtraction
//              from canonical, times the Montgomery-form scalar by wmont.
template <bool WIDE>
__device__ __forceinline__ uint64_t scaled1(uint64_t x, u64x2 s, const ModConsts &m) {
    if constexpr (WIDE) return wmont(x >= m.q ? x - m.q : x, s.x, m.q, m.qinv);
    else return shoup64(x, s.x, s.y, m.q);
}

}  // namespace FHE_NS
