// galois.hip -- the Galois automorphism sigma_g : X -> X^g (g odd) of
// negacyclic rows as a streaming signed permutation (fhe_poly_galois_batch,
// the source key of fhe_switch_key_generate, and the sigma_g rows of the
// composed fhe_ct_galois_batch for N > 16384 or q >= 2^62).
//
//   out[j g mod 2N]     = in[j] mod q             when j g mod 2N < N
//   out[j g mod 2N - N] = (q - in[j] mod q) % q   otherwise
//
// Direction: GATHER with g^-1 and write coalesced.  Output word k is
// +-in[k g^-1 mod 2N], so a lane owns two adjacent output words and stores
// them as one 16-byte non-temporal store, the access the other streaming
// kernels use; the two 8-byte reads are strided by g^-1 words.  The scattered
// side is then the read side, where a partial cache line costs a refetch from
// L2 at worst: every word of a row is consumed within one pass of the
// workgroups that share the row.  Scattering the writes instead would leave
// 8-byte partial lines to be merged in L2 before they reach HBM, and a line
// evicted early becomes a read-modify-write there.
//
// `add` (nullable) adds a second row mod q on the way out (the trace step's
// sigma_g(c0) + c0).  Polynomial i is at in + i in_pitch (and add + i
// in_pitch) and goes to out + i out_pitch, so a ciphertext component can be
// moved between [batch][2][N] and [batch][3][N] layouts.  Any N >= 4 (power
// of two), any odd q < 2^64; 16-byte aligned rows.
#include "fhe_internal.hpp"

namespace FHE_NS {

static constexpr int kGaloisBlock = 256;
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t galois_red(uint64_t x, const ModConsts &m) {
    return x < m.q ? x : mod64_slow(x, m.q, m.mu);
}
__device__ __forceinline__ uint64_t galois_word(const uint64_t *__restrict__ row, uint32_t k, uint32_t ginv, uint32_t n,
                                                const ModConsts &m) {
    const uint32_t j = (k * ginv) & (2 * n - 1);  // the u32 product wraps at a multiple of 2N
    const uint64_t x = galois_red(row[j & (n - 1)], m);
    return (j < n || x == 0) ? x : m.q - x;
}
__device__ __forceinline__ uint64_t galois_add(uint64_t x, uint64_t y, const ModConsts &m) {
    const uint64_t s = x + y;
    return (s < x || s >= m.q) ? s - m.q : s;
}

__global__ void __launch_bounds__(kGaloisBlock)
k_poly_galois(const uint64_t *__restrict__ in, const uint64_t *__restrict__ add, uint64_t *__restrict__ out,
              uint32_t logn, size_t npoly, uint32_t ginv, size_t in_pitch, size_t out_pitch, ModConsts m) {
    const uint32_t n = 1u << logn, half = n / 2;
    const size_t total = npoly << (logn - 1);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t poly = i >> (logn - 1);
        const uint32_t k = 2 * ((uint32_t)i & (half - 1));
        const uint64_t *row = in + poly * in_pitch;
        u64x2 z;
        z.x = galois_word(row, k, ginv, n, m);
        z.y = galois_word(row, k + 1, ginv, n, m);
        if (add) {
            const u64x2 a = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(add + poly * in_pitch + k));
            z.x = galois_add(z.x, galois_red(a.x, m), m);
            z.y = galois_add(z.y, galois_red(a.y, m), m);
        }
        __builtin_nontemporal_store(z, reinterpret_cast<u64x2 *>(out + poly * out_pitch + k));
    }
}

hipError_t launch_poly_galois(const ModConsts &m, uint32_t logn, uint32_t ginv, const uint64_t *in, const uint64_t *add,
                              uint64_t *out, size_t npoly, size_t in_pitch, size_t out_pitch, hipStream_t s) {
    if (npoly == 0) return hipSuccess;
    if (logn < 2 || ((in_pitch | out_pitch) & 1) || (((uintptr_t)add | (uintptr_t)out) & 15)) return hipErrorInvalidValue;
    const size_t work = npoly << (logn - 1), cap = 256 * 16;  // 256 CUs x 16 blocks: grid-stride beyond
    const size_t g = (work + kGaloisBlock - 1) / kGaloisBlock;
    hipLaunchKernelGGL(k_poly_galois, dim3((unsigned)(g > cap ? cap : g)), dim3(kGaloisBlock), 0, s, in, add, out, logn,
                       npoly, ginv, in_pitch, out_pitch, m);
    return hipGetLastError();
}

}  // namespace FHE_NS
