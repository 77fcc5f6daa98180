// ntt_ext.hip -- decompose / NTT / key-MAC / inverse kernels: the TFHE
// external product, BFV-style relinearisation and the blind-rotation CMux
// step share one kernel body (k_dmac) and differ only in where the digit
// polynomials come from and what the store epilogue adds.
//
// MODE 0  external product (BootstrapEngine::external_product,
//         bootstrap_engine.cpp:431-518): for each decomposition row r (mask
//         polynomials first, then the body; digit level inner, digits of
//         decompose_polynomial :152-185) and each output component j:
//           res_j = mod_add(res_j, inv( fwd(decomp_r) (.) fwd(ggsw[r][j]) )).
// MODE 1  relinearisation (EncryptionEngine::relinearize, encryption.cpp:
//         904-980): digit l of c2 is (c2 >> l*B) & (2^B - 1) (unsigned, LSB
//         first); c0' = c0 + sum_l inv(fwd(d_l) (.) fwd(b_l)),
//         c1' = c1 + sum_l inv(fwd(d_l) (.) fwd(a_l)), keys given as (a_l, b_l)
//         pairs (KeySwitchKey, key_manager.h:85-95; key_manager.cpp:296-324).
// MODE 2  one blind-rotation step (BootstrapEngine::blind_rotate :547-577 ->
//         cmux :520-540 -> multiply_glwe_by_monomial :249-261 ->
//         rotate_polynomial :122-145) for a batch of accumulators, each with
//         its own LWE mask coefficient a_i:
//           rot = (int32)((a_i * 2N + q/2) / q)   (u64 arithmetic)
//           rot == 0 : acc unchanged (the reference `continue`s)
//           else     : acc' = acc + ExtProd(X^rot * acc - acc, bsk[i])
//         The rotation and the subtraction are folded into the digit load.
// MODE 3  CMux with explicit inputs (cmux :520-540): out = ct0 +
//         ExtProd(ct1 - ct0, ggsw).
// MODE 4  Galois key switch of a degree-1 ciphertext (fhe_ct_galois_batch):
//         MODE 1 with the digits taken from sigma_g(c1) instead of c2 and the
//         addends sigma_g(c0) (+ c0) and (c1 | 0) instead of c0, c1.  No
//         sigma_g(c) row is ever stored: coefficient p of sigma_g(c) is
//         +-c[p g^-1 mod 2N] (lwe_ops.hpp galois_at), gathered straight from
//         the ciphertext's own rows on the digit load and in the store
//         epilogue.  Every word of a row is read once per pass by the one
//         workgroup that owns the ciphertext, so HBM traffic is that of a
//         coalesced read; what the gather costs is cache-line fan-out between
//         L2 and the CU: g = 3 (a line per lane) measures 0.9-2.3 % over
//         g = N + 1 (coalesced), DESIGN.md section 5.  That is all a coalesced
//         load scattered through the transform LDS region, the alternative,
//         could win back before paying for its barrier; it was not built.
//
// Every intermediate is a canonical residue and the inverse transform is
// linear over Z_q, so  sum_r inv(X_r) == inv(sum_r X_r)  bit-exactly: keys are
// transformed once (fhe_ggsw_prepare / fhe_relin_key_prepare: NTT x R,
// Montgomery form), every digit polynomial is produced on its HBM load,
// transformed in registers/LDS, multiplied into K1 NTT-domain accumulators,
// and only K1 inverse transforms run at the end -- one kernel, one HBM pass
// over the ciphertext.
// Flag-free 64-bit arithmetic with the carry-free mulhi in this unit (as in
// ntt_inv.hip; fhe_arith.hpp FHE_U64_NOVCC, FHE_MULHI64=4): fewer static VALU
// issue cycles in its 64-bit kernels and fewer of them with scratch (round 6,
// DESIGN.md section 5).
#ifndef FHE_U64_NOVCC
#define FHE_U64_NOVCC 1
#endif
#ifndef FHE_MULHI64
#define FHE_MULHI64 4
#endif
#include "fhe_internal.hpp"
#include "lwe_ops.hpp"

namespace FHE_NS {

// Where the K1 NTT-domain accumulators live between rows: 1 = a second LDS
// region, 2 = the ciphertext's own output rows in HBM (read-modify-write of
// the thread's own positions; no synchronisation needed).  Holding them in
// VGPRs spilled 300-800 B/lane.
// LDS accumulators are used only while they leave at least kExtMinWaves
// waves per CU resident: at N = 1024 with u64 words they would cut the CU to
// one 4-wave workgroup (99 KB of LDS), and the HBM/L2 round trip of the
// output-row stash is cheaper than that loss of latency hiding.
constexpr int kExtMinWaves = 8;
template <int LOGN, typename W, int K1, int MODE = 0>
constexpr int ext_stash() {
    using G = Geo<LOGN>;
    constexpr int bytes = G::P * (G::LW + K1 * G::N) * (int)sizeof(W);
    if (bytes <= 160 * 1024) {
        const int wg = (160 * 1024) / bytes < 2048 / G::THREADS ? (160 * 1024) / bytes : 2048 / G::THREADS;
        if (wg * G::THREADS / 64 >= kExtMinWaves) return 1;
    }
    // relinearisation (MODE 1): accumulator 0 in LDS, accumulator 1 and the
    // c2 words in VGPRs (one workgroup per CU); c2 is then read once instead
    // of once per digit level
    if ((MODE == 1 || MODE == 4) && K1 == 2 && G::P == 1 && (G::LW + G::N) * (int)sizeof(W) <= 160 * 1024)
        return 3;
    return 2;
}
template <int LOGN, typename W, int K1, int MODE = 0>
constexpr int ext_extra_words() {
    constexpr int st = ext_stash<LOGN, W, K1, MODE>();
    return st == 1 ? Geo<LOGN>::P * K1 * Geo<LOGN>::N : (st == 3 ? Geo<LOGN>::N : 0);
}

template <int LOGN, typename W, int K1, int MODE = 0>
constexpr int ext_occ() {
    constexpr int extra = ext_extra_words<LOGN, W, K1, MODE>();
    return Geo<LOGN>::template occ_waves<W, extra>();
}

struct DmArgs {
    const uint64_t *src;    // MODE 0: glwe [batch][K1][N]; 1: ct [batch][3][N]; 2: acc [batch][K1][N]; 4: ct [batch][2][N]
    const uint64_t *key;    // prepared key rows (NTT x R): 0/2: [K1*L][K1][N]; 1: [L][2][N] (a_l, b_l)
    uint64_t *out;          // [batch][K1][N]
    size_t batch;
    int level, base_log;
    const uint64_t *lwe_a;  // MODE 2: LWE masks [batch][lwe_dim]
    uint64_t lwe_q;
    uint32_t lwe_dim, step;
    const uint64_t *src2;   // MODE 3: ct1 [batch][K1][N] (src = ct0)
    uint32_t ginv;          // MODE 4: g^-1 mod 2N
    int add_input;          // MODE 4: out += ct
};

// Relinearisation with 32-bit words loads the row's whole key (low words of
// the prepared u64 rows; canonical residues < q < 2^32) after the digit
// transform in one batch instead of two coefficients at a time: 8.14 vs 8.30 ms
// per 16,384 ciphertexts (round 5).  Issued before the transform (kept in
// flight across it) it spills 28 VGPRs and takes 10.4 ms.
template <int LOGN, typename W, int K1, bool LAZY, int MODE>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, (ext_occ<LOGN, W, K1, MODE>()))
k_dmac(DmArgs D, NttArgs<W> A) {
    using G = Geo<LOGN>;
    constexpr int STASH = ext_stash<LOGN, W, K1, MODE>();
    constexpr bool RELIN = MODE == 1 || MODE == 4;  // unsigned LSB-first digits of one row, (a_l, b_l) keys
    constexpr bool KPF = RELIN && STASH == 3 && sizeof(W) == 4;
    constexpr int NIN = MODE == 1 ? 3 : K1;  // source polynomials per ciphertext
    __shared__ W lds_all[G::P * G::LW + ext_extra_words<LOGN, W, K1, MODE>()];
    const uint32_t tau = threadIdx.x & (G::T - 1), pl = wg_poly<G>();
    const size_t poly = (size_t)blockIdx.x * G::P + pl;
    const bool valid = poly < D.batch;
    if (G::P == 1 && !valid) return;  // whole workgroup: no barrier is skipped
    W *lds = lds_all + pl * G::LW;
    uint64_t *orow = D.out + poly * K1 * G::N;
    const uint64_t *srow = D.src + (valid ? poly : 0) * NIN * G::N;
    // accumulator j of this ciphertext: LDS, or row j of the output
    // (STASH 3: j = 0 only; accumulator 1 is racc)
    auto acc = [&](int j) -> W * {
        if constexpr (STASH == 1) return lds_all + G::P * G::LW + (pl * K1 + j) * G::N;
        else if constexpr (STASH == 3) return lds_all + G::LW;
        else return reinterpret_cast<W *>(orow + (size_t)j * G::N);
    };
    W racc[STASH == 3 ? G::E : 1];
    uint64_t craw[STASH == 3 ? G::E : 1];  // c2 (MODE 4: sigma_g(c1)) words at this lane's pass-0 positions

    const int level = D.level;
    const uint64_t base = 1ull << D.base_log, mask = base - 1, half = base / 2;
    const uint64_t q = A.q64, mu = A.mu64, lim = (uint64_t)A.ar.q2 * 2;
    if constexpr (STASH == 3) {
#pragma unroll
        for (int t = 0; t < G::E; ++t) {
            const uint32_t p = tau + cbrv(t, G::LOGE) * G::T;
            if constexpr (MODE == 4) craw[t] = valid ? galois_at(srow + G::N, p, D.ginv, G::N, q, mu) : 0;
            else craw[t] = valid ? srow[2 * G::N + p] : 0;
        }
    }
    bool skip = false;   // MODE 2, rot == 0: output = input accumulator
    uint32_t rot = 0;
    if constexpr (MODE == 2) {
        const int32_t r = valid ? rot_amount(D.lwe_a[poly * D.lwe_dim + D.step], G::N, D.lwe_q) : 0;
        skip = r == 0;
        rot = rot_norm(r, G::N);
        if (G::P == 1 && skip) {  // workgroup-uniform: copy and leave
            for (uint32_t i = threadIdx.x; i < (uint32_t)(K1 * G::N); i += G::THREADS) orow[i] = srow[i];
            return;
        }
    }
    const int rows = RELIN ? level : K1 * level;
    for (int r = 0; r < rows; ++r) {
        // opaque per-row copy of the lane index: keeps the (loop-invariant)
        // address arithmetic inside the loop instead of 100+ hoisted VGPRs
        uint32_t tr = tau;
        asm volatile("" : "+v"(tr));
        const int i = MODE == 1 ? 2 : MODE == 4 ? 1 : r / level, l = RELIN ? r : r % level;
        const uint32_t shift = RELIN ? uint32_t(l) * uint32_t(D.base_log)
                                         : uint32_t(level - 1 - l) * uint32_t(D.base_log);
        const uint64_t *src = srow + (size_t)i * G::N;
        const uint64_t *src2 = MODE == 3 ? D.src2 + ((valid ? poly : 0) * K1 + i) * G::N : nullptr;
        if (r > 0 && G::NP > 1) __syncthreads();
        W v[G::E];
        Tw<W> t0[PassTw<LOGN, 0>::COUNT];
        load_tw<LOGN, 0>(tr, A.twf, t0);
        load_coeffs<G::E>(v, lim, q, mu, [&](int t) -> uint64_t {
            const uint32_t p = tr + cbrv(t, G::LOGE) * G::T;
            if (!valid || skip) return 0;
            uint64_t c;
            if constexpr (STASH == 3) c = craw[STASH == 3 ? t : 0];
            else if constexpr (MODE == 2) c = subq(red_q(rotated_at(src, p, rot, G::N, q, mu), q, mu), red_q(src[p], q, mu), q);
            else if constexpr (MODE == 3) c = subq(red_q(src2[p], q, mu), red_q(src[p], q, mu), q);
            else if constexpr (MODE == 4) c = galois_at(src, p, D.ginv, G::N, q, mu);
            else c = src[p];
            uint64_t d = (c >> shift) & mask;
            if constexpr (!RELIN) {
                if (d > half) d = red_q(q - (base - d), q, mu);
            }
            return d;
        });
        // KPF: the row's key words loaded at once, after the digit transform
        uint32_t kw[KPF ? G::E : 1][2];
        auto load_keys = [&]() {
            const uint32_t *g32 = reinterpret_cast<const uint32_t *>(D.key + (size_t)r * K1 * G::N);
#pragma unroll
            for (int e = 0; e < (KPF ? G::E : 1); ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    kw[e][j] = g32[2 * ((size_t)(1 - j) * G::N + gidx<LOGN, G::NP - 1>(tr, e))];
        };
        fwd_pass<LOGN, 0, LAZY>(v, t0, A.ar);
        fwd_rest<LOGN, 1, LAZY, kPfSingle>(lds, v, tr, A.twf, A.ar);
        if constexpr (KPF) load_keys();
        if (!valid) continue;
        if constexpr (KPF) {
#pragma unroll
            for (int e = 0; e < G::E; ++e) {
                const uint32_t gi = gidx<LOGN, G::NP - 1>(tr, e);
                const W p0 = r == 0 ? W(0) : acc(0)[gi];
                const W p1 = r == 0 ? W(0) : racc[STASH == 3 ? e : 0];
                acc(0)[gi] = A.ar.red2q(p0 + A.ar.mont(v[e], (W)kw[e][0]));
                racc[STASH == 3 ? e : 0] = A.ar.red2q(p1 + A.ar.mont(v[e], (W)kw[e][1]));
            }
            continue;
        }
        const uint64_t *g = D.key + (size_t)r * K1 * G::N;
        // chunks of 2 coefficients: all key + accumulator loads of the row in
        // flight at once would not fit the register budget
#pragma unroll
        for (int c0 = 0; c0 < G::E; c0 += 2) {
            uint64_t kv[2][K1];
            W pv[2][K1];
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < K1; ++j) {
                    const uint32_t gi = gidx<LOGN, G::NP - 1>(tr, c0 + e);
                    const int kj = RELIN ? 1 - j : j;  // relin: c0' uses b_l, c1' uses a_l
                    kv[e][j] = g[(size_t)kj * G::N + gi];
                    if (STASH == 3 && j > 0) pv[e][j] = r == 0 ? W(0) : racc[STASH == 3 ? c0 + e : 0];
                    else pv[e][j] = r == 0 ? W(0) : acc(j)[gi];
                }
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < K1; ++j) {
                    // raw output (< R) times a canonical key: valid Montgomery pair
                    const W m = A.ar.mont(v[c0 + e], (W)kv[e][j]);
                    if (STASH == 3 && j > 0) racc[STASH == 3 ? c0 + e : 0] = A.ar.red2q(pv[e][j] + m);
                    else acc(j)[gidx<LOGN, G::NP - 1>(tr, c0 + e)] = A.ar.red2q(pv[e][j] + m);
                }
        }
    }
    auto out_row = [&](int j) {
        if (G::NP > 1) __syncthreads();
        uint32_t tr = tau;
        asm volatile("" : "+v"(tr));
        W v[G::E];
        if (STASH == 3 && j > 0) {
#pragma unroll
            for (int e = 0; e < G::E; ++e) v[e] = valid ? racc[STASH == 3 ? e : 0] : W(0);
        } else {
#pragma unroll
            for (int e = 0; e < G::E; ++e) v[e] = valid ? acc(j)[gidx<LOGN, G::NP - 1>(tr, e)] : W(0);
        }
        if constexpr (STASH == 2) {
            if (G::NP > 1) __syncthreads();  // every stash read of row j precedes its final stores
        }
        // MODE 1: + c_j (mod_add of encryption.cpp:953/958); MODE 2: + acc_j
        // (cmux's add_glwe_inplace, :537), or acc_j itself when skipped;
        // MODE 4: row 0 + sigma_g(c0) (+ c0), row 1 (+ c1).
        const uint64_t *addend = srow + (size_t)j * G::N;
        auto fin = [&](uint32_t gi, uint64_t x) -> uint64_t {
            if constexpr (MODE == 0) return x;
            else if constexpr (MODE == 4) {
                if (!valid) return 0;
                uint64_t a = D.add_input ? red_q(addend[gi], q, mu) : 0;
                if (j == 0) a = addq(galois_at(srow, gi, D.ginv, G::N, q, mu), a, q);
                return addq(x, a, q);
            } else {
                if (!valid) return 0;
                const uint64_t a = addend[gi];
                if (MODE == 2 && skip) return a;
                return addq(x, red_q(a, q, mu), q);
            }
        };
        inv_poly_from_regs<LOGN>(lds, v, tr, orow + (size_t)j * G::N, valid, A, A.ninv, 0, fin);
    };
    if constexpr (STASH == 3) {  // unrolled: racc is indexed by the row
#pragma unroll
        for (int j = 0; j < K1; ++j) out_row(j);
    } else {
#pragma nounroll
        for (int j = 0; j < K1; ++j) out_row(j);
    }
}

// External product with one decomposition level (level == 1, K1 == 2) for
// one polynomial per workgroup: the two digit polynomials are transformed in
// lockstep (shared twiddles), the key MAC turns (X0, X1) into the two
// NTT-domain outputs in place, and both inverses run in lockstep -- nothing
// is parked in HBM (k_dmac's output-row stash read and wrote every
// accumulator once per row: 2.2x the algorithmic traffic at N = 16384).
template <int LOGN, typename W>
__global__ void __launch_bounds__(Geo<LOGN>::THREADS, Geo<LOGN>::template occ_waves<W>())
k_extprod2(DmArgs D, NttArgs<W> A) {
    using G = Geo<LOGN>;
    static_assert(G::P == 1, "one ciphertext per workgroup");
    constexpr int PF = 0;  // no twiddle stage ahead of the exchanges: two 16-word spectra are live
    __shared__ W lds[G::LW];
    const TidSource tid;  // lane index per phase, not held across phases
    const uint32_t tau = tid();
    const size_t poly = blockIdx.x;
    if (poly >= D.batch) return;
    const uint64_t *srow = D.src + poly * 2 * G::N;
    uint64_t *orow = D.out + poly * 2 * G::N;
    const uint64_t base = 1ull << D.base_log, mask = base - 1, half = base / 2;
    const uint64_t q = A.q64, mu = A.mu64, lim = (uint64_t)A.ar.q2 * 2;
    W v0[G::E], v1[G::E];
    Tw<W> t0[PassTw<LOGN, 0>::COUNT];
    load_tw<LOGN, 0>(tau, A.twf, t0);
    // digit (level 0 of 1: shift 0) of glwe row i, signed (decompose_polynomial)
    auto digit = [&](const uint64_t *src, int t) -> uint64_t {
        uint64_t d = src[tau + cbrv(t, G::LOGE) * G::T] & mask;
        if (d > half) d = red_q(q - (base - d), q, mu);
        return d;
    };
    load_coeffs<G::E>(v0, lim, q, mu, [&](int t) { return digit(srow, t); });
    load_coeffs<G::E>(v1, lim, q, mu, [&](int t) { return digit(srow + G::N, t); });
    fwd_pass<LOGN, 0, false>(v0, t0, A.ar);
    fwd_pass<LOGN, 0, false>(v1, t0, A.ar);
    fwd_rest2<LOGN, 1, false, PF>(lds, v0, v1, tau, A.twf, A.ar);
    // (o0, o1) = (X0 G00 + X1 G10, X0 G01 + X1 G11); raw outputs (< 4q) times
    // canonical prepared keys: valid Montgomery pairs
    const uint64_t *g = D.key;
    const uint32_t tm = tid();
#pragma unroll
    for (int e0 = 0; e0 < G::E; e0 += 2) {
        uint64_t k[2][4];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) k[e][j] = g[(size_t)j * G::N + gidx<LOGN, G::NP - 1>(tm, e0 + e)];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const W x0 = v0[e0 + e], x1 = v1[e0 + e];
            v0[e0 + e] = A.ar.red2q(A.ar.mont(x0, (W)k[e][0]) + A.ar.mont(x1, (W)k[e][2]));
            v1[e0 + e] = A.ar.red2q(A.ar.mont(x0, (W)k[e][1]) + A.ar.mont(x1, (W)k[e][3]));
        }
    }
    __syncthreads();
    const uint32_t ti = tid();
    inv_poly2<LOGN, PF>(lds, v0, v1, ti, orow, orow + G::N, A, A.ninv);
}

// Relinearisation takes k_dmac MODE 1.  Two 32-coefficient-per-thread
// kernels (c2 low words and accumulator 1 in VGPRs, accumulator 0 in LDS; 8
// waves per CU) measured slower on MI355X: single digit transforms 9.03 vs
// 8.29 ms per 16,384 ciphertexts (round 4), digit levels in lockstep pairs
// 4.67 vs 4.27 ms per 8,192 (round 5) -- the 16 waves of MODE 1 hide more of
// the exchange barriers than the shorter transforms save.  One 512-thread
// workgroup per ciphertext with accumulator 0 in the output row (two
// workgroups per CU) measured 9.11 ms against 8.19 ms (profiles/r6d).

template <int LOGN, typename W, int MODE>
static hipError_t dmac_one(const NttArgs<W> &A, hipStream_t s, int k1, const DmArgs &D) {
    using G = Geo<LOGN>;
    const size_t blocks = (D.batch + G::P - 1) / G::P;
    if (k1 != 2) return hipErrorInvalidValue;
    if constexpr (MODE == 0 && G::P == 1 && sizeof(W) == 8 && LOGN >= 12) {
        if (D.level == 1) {
            if constexpr (LOGN == 14) {
                // a sparse prime (ntt_core.hpp gk_sparse): C5 (23, 1) 8.1 -> 7.7 ms
                // per 16,384 (round 5)
                if (A.ar.sp == 1 || A.ar.sp == 2) {
                    if (A.ar.sp == 1)
                        hipLaunchKernelGGL((k_extprod2<gk_sparse(LOGN, 1), W>), dim3((unsigned)D.batch),
                                           dim3(G::THREADS), 0, s, D, A);
                    else
                        hipLaunchKernelGGL((k_extprod2<gk_sparse(LOGN, 2), W>), dim3((unsigned)D.batch),
                                           dim3(G::THREADS), 0, s, D, A);
                    return hipGetLastError();
                }
            }
            hipLaunchKernelGGL((k_extprod2<LOGN, W>), dim3((unsigned)D.batch), dim3(G::THREADS), 0, s, D, A);
            return hipGetLastError();
        }
    }
    // (unit twiddles, ntt_core.hpp gk_compat, measured 0 to +0.4 % here and in
    // the external-product kernels, round 5: not instantiated)
    hipLaunchKernelGGL((k_dmac<LOGN, W, 2, false, MODE>), dim3(blocks), dim3(G::THREADS), 0, s, D, A);
    return hipGetLastError();
}

template <typename W, int MODE>
static hipError_t dmac_dispatch(const Plan &p, const NttArgs<W> &A, int k1, const DmArgs &D) {
    switch (p.logn) {
#define FHE_CASE(L) \
    case L: return dmac_one<L, W, MODE>(A, p.stream, k1, D);
        FHE_CASE(2) FHE_CASE(3) FHE_CASE(4) FHE_CASE(5) FHE_CASE(6) FHE_CASE(7) FHE_CASE(8)
        FHE_CASE(9) FHE_CASE(10) FHE_CASE(11) FHE_CASE(12) FHE_CASE(13) FHE_CASE(14)
#undef FHE_CASE
    default: return hipErrorInvalidValue;
    }
}

template <int MODE>
static hipError_t dmac(const Plan &p, int k1, const DmArgs &D) {
    if (D.batch == 0) return hipSuccess;
    if (p.word == 32)
        return dmac_dispatch<uint32_t, MODE>(p, p.a32, k1, D);
    return dmac_dispatch<uint64_t, MODE>(p, p.a64, k1, D);
}

hipError_t launch_extprod(const Plan &p, int k1, int level, int base_log, const uint64_t *glwe,
                          const uint64_t *ggsw, uint64_t *out, size_t batch) {
    if (extprod_acc_supported(p, k1, level, base_log))
        return launch_extprod_acc(p, level, base_log, glwe, ggsw, out, batch);
    DmArgs D{glwe, ggsw, out, batch, level, base_log, nullptr, 0, 0, 0, nullptr};
    return dmac<0>(p, k1, D);
}

hipError_t launch_relin(const Plan &p, int level, int base_log, const uint64_t *ct3, const uint64_t *rlk,
                        uint64_t *out, size_t batch) {
    DmArgs D{ct3, rlk, out, batch, level, base_log, nullptr, 0, 0, 0, nullptr};
    return dmac<1>(p, 2, D);
}

hipError_t launch_ct_galois(const Plan &p, int level, int base_log, uint32_t ginv, int add_input, const uint64_t *ct,
                            const uint64_t *swk, uint64_t *out, size_t batch) {
    DmArgs D{ct, swk, out, batch, level, base_log, nullptr, 0, 0, 0, nullptr, ginv, add_input};
    return dmac<4>(p, 2, D);
}

hipError_t launch_cmux_rotate(const Plan &p, int k1, int level, int base_log, const uint64_t *acc_in,
                              const uint64_t *ggsw, uint64_t *acc_out, size_t batch, const uint64_t *lwe_a,
                              uint32_t lwe_dim, uint32_t step, uint64_t lwe_q) {
    DmArgs D{acc_in, ggsw, acc_out, batch, level, base_log, lwe_a, lwe_q, lwe_dim, step, nullptr};
    return dmac<2>(p, k1, D);
}

hipError_t launch_cmux(const Plan &p, int k1, int level, int base_log, const uint64_t *ggsw, const uint64_t *ct0,
                       const uint64_t *ct1, uint64_t *out, size_t batch) {
    DmArgs D{ct0, ggsw, out, batch, level, base_log, nullptr, 0, 0, 0, ct1};
    return dmac<3>(p, k1, D);
}

}  // namespace FHE_NS
