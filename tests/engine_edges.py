"""Moduli, plaintext moduli and planted inputs for the decode epilogue of the
BFV decryptions and for the encoders (helpers of test_engine_edges.py,
test_gpu_engine_edges.py and test_gpu_keygen_edges.py; plain Python and
numpy, no GPU).

Every decryption ends in Decoder of node-fhe-accelerate_amd/csrc/
engine_kernels.hpp: rounded(p) = (p t + q / 2) / q through a corrected double
estimate, the fold of t to 0, the int64 noise distance and a per-ciphertext
maximum.  It is compiled into k_decrypt (one instance per degree, word size
and laziness; several polynomials per workgroup below N = 4096), k_decode
(engine_composed.hip: q >= 2^62 and N > 16384) and combine_body
(threshold.hip).  A uniformly random phase meets a rounding step with
probability t / q, so the phases here are planted: lwe_edges.edge_phases puts
one on either side of the steps, :func:`plant` builds ciphertexts that decrypt
to them under a non-zero key, and :func:`noise_rows` puts the maximum noise
at a chosen coefficient.
"""
from __future__ import annotations

import functools

import numpy as np

import lwe_edges as E
import ntt_primes as P
import oracle

M64 = P.M64
SEED = [0x0123456789ABCDEF, 0x0F1E2D3C4B5A6978, 42, 7]

# Every degree of the fused engine kernels (eng_dispatch, logN 2..14), and
# one two-pass degree (composed by degree).
FUSED_DEGREES = tuple(1 << l for l in range(2, 15))
FULL_DEGREES = (16, 256, 1024, 4096)  # the whole modulus list
BIG = 32768
DEGREES = FUSED_DEGREES + (BIG,)


def polys_per_workgroup(n: int) -> int:
    """Geo<L>::P of node-fhe-accelerate_amd/csrc/ntt_core.hpp (P = 256 / T
    for T = N / E < 256 threads per polynomial, else 1) with the default
    words per thread E of gk_loge, which the engine kernels use: one thread
    per polynomial below 16, 16 words per thread from there on.  (A kernel
    key that overrides E changes T only where T >= 256 either way.)"""
    return 256 if n < 16 else max(1, 4096 // n)


@functools.lru_cache(maxsize=None)
def moduli(n: int) -> dict:
    """name -> q.  The full degrees take stream_primes (both word sizes, the
    wide family from 2^62 and both sides of 2^63: k_decode) and the largest
    lazy prime; the others the largest lazy and the largest 62-bit prime; the
    two-pass degree one 32-bit and one 62-bit prime."""
    if n == BIG:
        b = P.boundary_primes(n)
        return {"u32_top": b["u32_top"], "u64_top": b["u64_top"]}
    s = P.sweep_primes(n)
    if n in FULL_DEGREES:
        return dict(P.stream_primes(n), lazy_top=s["lazy_top"])
    return {"lazy_top": s["lazy_top"], "u64_top": s["u64_top"]}


def cases(degrees=DEGREES) -> list:
    return [(n, name) for n in degrees for name in moduli(n)]


def word_pair(n: int) -> tuple:
    """One 32-bit and one 64-bit modulus name of the degree."""
    return ("u32_top", "u64_top") if n == BIG else ("lazy_top", "u64_top")


def plaintext_moduli(q: int) -> list:
    """lwe_edges.plaintext_moduli, an odd t that is no power of two, and
    2^40 (t = 0 selects 4)."""
    return P._distinct(E.plaintext_moduli(q) + [3, 1 << 40])


def rng(*seed):
    return np.random.default_rng([int(s) % (1 << 32) for s in seed])


def below(r, q: int, shape) -> np.ndarray:
    return r.integers(0, q - 1, size=shape, dtype=np.uint64, endpoint=True)


# ---------------------------------------------------------------- planted phases
def phase_list(q: int, t: int) -> list:
    """edge_phases(q, t) interleaved with the exact encodings v delta of
    v = 0, 1, t - 1 (noise 0)."""
    te = t or 4
    delta = q // te
    exact = [(v * delta) % q for v in (0, 1, te - 1)]
    out = []
    for i, p in enumerate(E.edge_phases(q, t)):
        out += [p, exact[i % 3]]
    return out


def phase_rows(n: int, q: int, t: int, rows: int) -> np.ndarray:
    """[rows, n]: phase_list tiled along a row, row i rotated by i, so that
    each phase visits different lanes and register slots."""
    L = np.array(phase_list(q, t), dtype=np.uint64)
    idx = (np.arange(n)[None, :] + np.arange(rows)[:, None]) % len(L)
    return np.ascontiguousarray(L[idx])


def rows_for(n: int) -> int:
    """One workgroup full of polynomials and one more in the next."""
    return polys_per_workgroup(n) + 1


def ternary_key(n: int, q: int, seed: int = 0) -> np.ndarray:
    """-1, 0, 1 coefficients, the first three -1, 1, -1 (never zero)."""
    s = rng(n, q, q >> 32, 3, seed).integers(0, 3, size=n)
    s[:3] = [0, 2, 0]
    return np.where(s == 0, np.uint64(q - 1), (s - 1).astype(np.uint64)).astype(np.uint64)


def plant(o, want: np.ndarray, s: np.ndarray, c1: np.ndarray, c2: np.ndarray = None) -> np.ndarray:
    """[rows, 2 or 3, n] ciphertexts in coefficient form whose phase
    c0 - c1 s [- c2 s^2] under the oracle's own product is `want`."""
    q = o.q
    tile = lambda p: np.ascontiguousarray(np.broadcast_to(p, c1.shape))
    flat = lambda a: np.ascontiguousarray(a.reshape(-1))
    acc = oracle.poly_add(q, flat(want), flat(o.polymul(c1, tile(s))))
    comps = [c1]
    if c2 is not None:
        s2 = o.polymul(s[None, :], s[None, :])[0]
        acc = oracle.poly_add(q, acc, flat(o.polymul(c2, tile(s2))))
        comps.append(c2)
    return np.ascontiguousarray(np.stack([acc.reshape(c1.shape)] + comps, axis=1))


def forms(q: int) -> tuple:
    """The values of is_ntt a phase can be planted for.  From q = 2^63 on the
    reference's N^-1 is 0 (its signed extended Euclid reads the modulus as a
    negative int64), so the phase of an NTT-form ciphertext is 0 whatever it
    holds: only the coefficient form, whose phase is then c0, carries planted
    phases there (test_engine_edges.py asserts both)."""
    return (False, True) if q < 1 << 63 else (False,)


def to_ntt(o, ct: np.ndarray) -> np.ndarray:
    """Every component transformed forward with the oracle."""
    return np.ascontiguousarray(o.forward(ct.reshape(-1, ct.shape[-1])).reshape(ct.shape))


def planted_cts(o, n: int, q: int, t: int, comps: int, rows: int = None):
    """(want [rows, n], sk [n], ct [rows, comps, n]) for the decode sweeps."""
    rows = rows or rows_for(n)
    want = phase_rows(n, q, t, rows)
    r = rng(n, q, q >> 32, t, t >> 32, comps)
    s = ternary_key(n, q)
    c1 = below(r, q, (rows, n))
    c2 = below(r, q, (rows, n)) if comps == 3 else None
    return want, s, plant(o, want, s, c1, c2)


def partials_for(q: int, c0: np.ndarray, want: np.ndarray, lambdas, seed: int = 0) -> np.ndarray:
    """[count, rows, n] canonical partial decryptions with
    sum_i partials[i] lambdas[i] = c0 - want (mod q): all seeded but the one
    of the last non-zero lambda, which is solved for.  (From q = 2^63 on the
    reference's Lagrange coefficients of the ids 1, 2, 3 are 0, 3, 0: its
    signed modular inverse again.)"""
    r = rng(q, q >> 32, len(lambdas), seed)
    lam = [int(x) % q for x in lambdas]
    solve = max(i for i, l in enumerate(lam) if l)
    flat = lambda a: np.ascontiguousarray(a.reshape(-1))
    rest = oracle.poly_sub(q, flat(c0), flat(want))
    blocks = [below(r, q, c0.shape) for _ in lam]
    for i, l in enumerate(lam):
        if i != solve:
            rest = oracle.poly_sub(q, rest, oracle.poly_mul_scalar(q, flat(blocks[i]), l))
    blocks[solve] = oracle.poly_mul_scalar(q, rest, pow(lam[solve], -1, q)).reshape(c0.shape)
    return np.ascontiguousarray(np.stack(blocks))


# ---------------------------------------------------------------- encoders
def encode_values(q: int, t: int) -> list:
    """Slot values at the edges of encode_packed's u64 product v delta:
    0, 1, t - 1, t, t + 1, 2^32, 2^63, 2^64 - 1 and the smallest v whose
    product wraps."""
    te = t or 4
    delta = q // te
    v = [0, 1, te - 1, te, te + 1, 1 << 32, 1 << 63, M64]
    if delta:
        v.append(-(-(1 << 64) // delta))  # past the word for delta = 1: dropped
    return P._distinct(v)


def value_rows(n: int, q: int, t: int, rows: int) -> np.ndarray:
    V = np.array(encode_values(q, t), dtype=np.uint64)
    return np.ascontiguousarray(V[(np.arange(n)[None, :] + np.arange(rows)[:, None]) % len(V)])


def raw_ciphertexts(n: int, q: int, rows: int, seed: int = 0) -> np.ndarray:
    """[rows, 2, n] canonical words with the raw words 2^64 - 1, q and q + 1
    in c0 (the first three coefficients of row 0, the last three of the last
    row) and 2^64 - 1 in c1 (copied as it is)."""
    ct = below(rng(n, q, q >> 32, rows, 11, seed), q, (rows, 2, n))
    ct[0, 0, :3] = [M64, q, q + 1]
    ct[-1, 0, -3:] = [q + 1, q, M64]
    ct[0, 1, 0] = M64
    return ct


ENCODE_DEGREES = (4, 64, 512, 2048, 16384, BIG)  # the degrees test_gpu_engine.py leaves out


# ---------------------------------------------------------------- noise placement
NOISE_T = 65537


def noise_positions(n: int) -> list:
    """Every coefficient up to n = 256; beyond, 0, n - 1, every 2^k and
    2^k - 1 and 61 seeded positions."""
    if n <= 256:
        return list(range(n))
    pos = [0, n - 1]
    for k in range(n.bit_length() - 1):
        pos += [1 << k, (1 << k) - 1]
    pos += [int(x) for x in rng(n, 61).integers(0, n, size=61)]
    return P._distinct(pos)


def noise_rows(n: int, q: int, t: int = NOISE_T):
    """(phase [batch, n], values [batch, n], noise [batch]): every coefficient
    an exact encoding v delta of a value 1 <= v <= vmax (so that the noisy
    one stays clear of 0 and q), except position noise_positions(n)[i] of row
    i, which is off by d_i = i + 1 -- above in even rows, below in odd ones.
    p t = v q - v (q mod t) +- d t rounds to v when v (q mod t) + d t < q / 2:
    vmax is the largest value (up to t - 2) for which that holds with
    d = batch.  The values then decode unchanged and max_noise[i] = d_i."""
    pos = noise_positions(n)
    batch = len(pos)
    delta = q // t
    vmax = min(t - 2, (q // 2 - batch * t - 1) // max(q % t, 1))
    assert delta // 2 > batch and vmax >= 3, (n, q, t)
    i = np.arange(batch)[:, None]
    vals = (1 + (np.arange(n)[None, :] * 31 + i) % vmax).astype(np.uint64)
    phase = vals * np.uint64(delta)
    d = np.arange(1, batch + 1, dtype=np.uint64)
    for r, p in enumerate(pos):
        phase[r, p] = phase[r, p] + d[r] if r % 2 == 0 else phase[r, p] - d[r]
    return np.ascontiguousarray(phase), np.ascontiguousarray(vals), d


# ---------------------------------------------------------------- key material
INT64_MIN, INT64_MAX = E.INT64_MIN, E.INT64_MAX
GGSW_VALUES = [0, 1, -1, 3, INT64_MIN, INT64_MAX, -(1 << 62), 1 << 40]
# (k, base_log, level): (l + 1) base_log reaches 64 at (32, 2) and passes it at
# (33, 2) and (16, 5); (63, 1) is the largest single shift
GGSW_DECOMPS = ((1, 32, 2), (2, 33, 2), (1, 63, 1), (3, 16, 5), (1, 7, 1))
GGSW_DEGREES = (16, 256)

KSK_DIMS = (1, 63, 64, 65, 130)  # around the 64-lane stride of k_ksk_body, and a third trip
KSK_DECOMPS = ((32, 2), (7, 3), (63, 1))
KSK_STD = (3.2, 1e6)
KSK_DEGREE = 16


def ksk_moduli() -> dict:
    """P27, the prime below 2^63 and QG = 2^64 - 2^32 + 1, at the degree of the
    context that carries them.  2^64 - 59 = 5 (mod 8) is the modulus of no
    context of degree 4 or more (q = 1 mod 2N), so the word's last prime that
    is one stands in for it."""
    s = P.stream_primes(KSK_DEGREE)
    return {"P27": E.P27, "shoup_top": s["shoup_top"], "QG": P.QG, "u64_max": s["u64_max"]}


def glwe_key_words(q: int) -> np.ndarray:
    return np.array([0, 1, q - 1, q, 1 << 63, M64, 5, 7], dtype=np.uint64)
