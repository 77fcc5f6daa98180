"""Moduli at the edges of the kernel families, and rows that fill the
unreduced input windows (helpers of test_ntt_primes.py, test_gpu_ranges.py,
test_gpu_ranges_big.py, test_gpu_ranges_stream.py, test_gpu_negacyclic.py and
test_gpu_rns_limbs.py; plain Python and numpy, no GPU).

The library picks its kernels from the modulus
(node-fhe-accelerate_amd/csrc/fhe_gpu.cpp, fhe_ctx_create):

  word = q < 2^30 ? 32 : 64                        (line 917)
  wide = q >= 2^62                                 (line 918)
  lazy = word == 32 && (4 + 2 log2 N) q <= 2^32    (line 980, plan.lazy)

The lazy flag is not part of fhe_ctx_info, so :func:`is_lazy` restates the
inequality.  :func:`boundary_primes` gives, for one degree, the NTT-friendly
primes (q = 1 mod 2N) on either side of each of those thresholds, and
:func:`wrap_prime` the first one at which the lazy forward provably wraps.
The streaming kernels change arithmetic at q = 2^63 instead:
:func:`stream_primes` and the word and scalar lists at the end of the file.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
QG = (1 << 64) - (1 << 32) + 1  # the wide family's usual prime

_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def is_prime(n: int) -> bool:
    """Miller-Rabin with the first twelve primes (2..37) as bases:
    deterministic for n < 318665857834031151167461 (about 3.18e23), which
    covers every u64."""
    if n < 2:
        return False
    for p in _MR_BASES:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in _MR_BASES:
        x = pow(a, d, n)
        if x == 1 or x == n - 1:
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_below(limit: int, n: int) -> int:
    """The largest prime q <= limit with q = 1 (mod 2n)."""
    step = 2 * n
    q = (limit - 1) // step * step + 1
    while q > 1:
        if is_prime(q):
            return q
        q -= step
    raise ValueError(f"no prime = 1 mod {step} up to {limit}")


def prime_above(limit: int, n: int) -> int:
    """The smallest prime q > limit with q = 1 (mod 2n)."""
    step = 2 * n
    q = limit // step * step + 1
    if q <= limit:
        q += step
    while not is_prime(q):
        q += step
    return q


def log2(n: int) -> int:
    assert n > 0 and n & (n - 1) == 0
    return n.bit_length() - 1


def lazy_bound(n: int) -> int:
    """floor(2^32 / (4 + 2 log2 n)): the largest q the lazy forward takes."""
    return (1 << 32) // (4 + 2 * log2(n))


def is_lazy(n: int, q: int) -> bool:
    """plan.lazy of fhe_ctx_create (node-fhe-accelerate_amd/csrc/fhe_gpu.cpp:980), restated."""
    return q < (1 << 30) and (4 + 2 * log2(n)) * q <= (1 << 32)


def word_bits(q: int) -> int:
    return 32 if q < (1 << 30) else 64


BOUNDARY_NAMES = ("lazy_top", "nonlazy_bottom", "u32_top", "u64_bottom", "u64_top")


def boundary_primes(n: int) -> dict:
    lb = lazy_bound(n)
    return {
        "lazy_top": prime_below(lb, n),
        "nonlazy_bottom": prime_above(lb, n),
        "u32_top": prime_below((1 << 30) - 1, n),
        "u64_bottom": prime_above(1 << 30, n),
        "u64_top": prime_below((1 << 62) - 1, n),
    }


def wrap_prime(n: int) -> int:
    """The smallest prime above 2^32 / (3 + log2 n): a modulus the lazy
    forward must not take, with a row that proves it.

    The bound (4 + 2L) q of the lazy butterflies (fhe_arith.hpp ct_lazy:
    x' = a + b, y' = a - b + 2q with the Shoup product b in [0, 2q)) is not
    attained: b = 0 needs a lower input that is literally 0, and a lower
    input that is a nonzero multiple k q of q gives b = q exactly (the Shoup
    quotient is k w - 1).  For the row with 4q-1 in word 0 and 0 elsewhere
    the largest word therefore moves along indices 0, 1, 3, .., n-1 and gains
    q per stage: it ends at (3 + L) q - 1 in compat mode, whose stage 0 is
    the reducing unit butterfly, and at (5 + L) q - 1 in negacyclic mode.
    Both pass 2^32 at this modulus, so a lazy inequality loosened far enough
    to take it fails on that row (measured on a library built with
    (2 + L) q <= 2^32: the sweeps fail at this prime at every degree, in
    both modes, on the sparse, the 3q and the lim-1 rows first).  An
    inequality between the two, such as (2 + 2L) q <= 2^32, makes
    nonlazy_bottom lazy without any row reaching 2^32: measured as well, the
    sweeps pass on such a library, so they cannot tell it from the real one."""
    return prime_above((1 << 32) // (3 + log2(n)), n)


SWEEP_NAMES = BOUNDARY_NAMES + ("wrap",)


def sweep_primes(n: int) -> dict:
    """boundary_primes and the wrap prime: the moduli of the GPU sweeps."""
    return dict(boundary_primes(n), wrap=wrap_prime(n))


LIMB_FAMILIES = ("lazy", "nonlazy32", "u64")


def limb_families(n: int) -> dict:
    """Three uniform RNS rings of three distinct primes each, one per kernel
    shape of the one-launch limb kernels (fhe_rns_ctx_create: every limb of
    the same word and laziness):

    lazy       lazy_top, the next prime below it and the smallest prime
               = 1 mod 2n: two neighbours at the bound and one whose constants
               differ from theirs by orders of magnitude
    nonlazy32  nonlazy_bottom, wrap, u32_top: 32-bit lanes, none lazy
    u64        u64_bottom, the first prime above 2^45, u64_top"""
    s = sweep_primes(n)
    return {
        "lazy": [s["lazy_top"], prime_below(s["lazy_top"] - 1, n), prime_above(1, n)],
        "nonlazy32": [s["nonlazy_bottom"], s["wrap"], s["u32_top"]],
        "u64": [s["u64_bottom"], prime_above(1 << 45, n), s["u64_top"]],
    }


# ---------------------------------------------------------------- adversarial rows
def window_limit(q: int, inverse: bool = False) -> int:
    """Words below this enter the butterflies as they are (4q: forward-type
    loads, ntt_core.hpp fwd_poly; 2q: inverse loads, ntt_inv.hip); words at
    or above it take the exact reduction first."""
    if q >> 62:  # wide family (ntt_wide.hip): every word is reduced at the load
        return q
    return (2 if inverse else 4) * q


def base_rows(n: int, q: int, inverse: bool = False, seed: int = 0, reduced: bool = False):
    """The rows that sit at the edges of the input window [0, lim), as
    (names, uint64 array [rows, n]).

    constant  every word 0, q-1, q, 2q, 3q (forward; the inverse's 2q is
              its lim), lim-1, lim, lim+1, 2^64-1, and in 32-bit lanes 2^32-2,
              2^32-1, 2^32; for q >= 2^62 (lim = q) without the repeats and
              the values past the word
    sparse    lim-1 at index 0 / at index n-1 and 0 elsewhere; 0 and lim-1
              alternating
    mixed     uniform in [0, lim); the same row with one word of every group
              of 16 (one word of the row below n = 16) replaced by a word
              >= lim, which takes the slow path among in-window neighbours
    canon     uniform in [0, q)

    reduced: without the canonical row (the callers with a slow reference)."""
    lim = window_limit(q, inverse)
    rng = np.random.default_rng([n, q % (1 << 32), q >> 32, int(inverse), seed])
    names, rows = [], []

    def put(name, row):
        names.append(name)
        rows.append(np.asarray(row, dtype=np.uint64))

    consts = [("0", 0), ("q-1", q - 1), ("q", q)]
    if not inverse:  # the inverse window ends at 2q: that row is "lim"
        consts += [("2q", 2 * q), ("3q", 3 * q)]
    consts += [("lim-1", lim - 1), ("lim", lim), ("lim+1", lim + 1), ("2^64-1", M64)]
    if word_bits(q) == 32:
        consts += [("2^32-2", (1 << 32) - 2), ("2^32-1", (1 << 32) - 1), ("2^32", 1 << 32)]
    seen = set()
    for name, v in consts:
        if v > M64 or v in seen:  # q >= 2^62: multiples of q past the word, lim = q
            continue
        seen.add(v)
        put("const " + name, np.full(n, v, dtype=np.uint64))

    top = np.uint64(lim - 1)
    first = np.zeros(n, dtype=np.uint64)
    first[0] = top
    put("sparse first", first)
    last = np.zeros(n, dtype=np.uint64)
    last[n - 1] = top
    put("sparse last", last)
    alt = np.zeros(n, dtype=np.uint64)
    alt[1::2] = top
    put("sparse alternating", alt)

    mixed = rng.integers(0, lim, size=n, dtype=np.uint64)
    put("mixed in-window", mixed)
    slow = mixed.copy()
    group = min(n, 16)
    at = np.arange(0, n, group) + rng.integers(0, group, size=n // group)
    slow[at] = rng.integers(lim, M64, size=at.size, dtype=np.uint64, endpoint=True)
    slow[at[0]] = lim  # the first word that leaves the window
    put("mixed one slow word per 16", slow)

    if not reduced:
        put("canonical", rng.integers(0, q, size=n, dtype=np.uint64))
    return names, np.stack(rows)


def tile_rows(rows: np.ndarray, at_least: int, ragged_for: int = 1) -> np.ndarray:
    """The rows repeated cyclically to at_least rows (and at least once), one
    more where the count would be a multiple of ragged_for > 1."""
    total = max(at_least, rows.shape[0])
    if ragged_for > 1 and total % ragged_for == 0:
        total += 1
    return np.ascontiguousarray(rows[np.arange(total) % rows.shape[0]])


def multiply_partners(x: np.ndarray, names, q: int) -> dict:
    """Second operands for multiply(x, y) over the tiled rows x (row i is base
    row names[i % len(names)]), by name:

    rolled     x rolled by 5 rows (by 1 below six rows): extreme rows
               against other extreme rows
    squares    x itself: lim-1 against lim-1 and the sparse rows against
               themselves, both operands at the top of the window
    canonical  one nonzero canonical row (the in-window mixed row mod q)
               against every row, so that no extreme row is checked only
               against an all-zero product"""
    names = list(names)
    mixed = "mixed in-window" if "mixed in-window" in names else "mixed one slow word per 16"
    canon = x[names.index(mixed)] % np.uint64(q)
    assert canon.any()
    return {
        "rolled": np.ascontiguousarray(np.roll(x, 5 if x.shape[0] > 5 else 1, axis=0)),
        "squares": x,
        "canonical": np.ascontiguousarray(np.broadcast_to(canon, x.shape)),
    }


def weight_rows(n: int, q: int, count: int, period: int, seed: int = 1) -> np.ndarray:
    """Second operands for forward_ntt_mul / pointwise_multiply, count rows:
    canonical random, all q-1, raw all q, raw all 2^64-1, the kind changing
    every `period` rows (so with operands tiled from `period` base rows every
    base row meets every kind within 4 * period rows)."""
    rng = np.random.default_rng([n, q % (1 << 32), q >> 32, 77, seed])
    w = rng.integers(0, q, size=(count, n), dtype=np.uint64)
    kind = (np.arange(count) // max(period, 1)) % 4
    w[kind == 1] = np.uint64(q - 1)
    w[kind == 2] = np.uint64(q)
    w[kind == 3] = np.uint64(M64)
    return w


# ---------------------------------------------------------------- streaming kernels: the 2^63 edge
# The streaming sums (tally.hip, threshold.hip, elementwise.hip) take any
# degree and switch their word arithmetic at q = 2^63: the Shoup product and
# the Barrett reduction below, the Montgomery product and one conditional
# subtraction above (tally_ops.hpp scaled1, fhe_arith.hpp mod64_slow).
STREAM_NAMES = ("u32_top", "u64_bottom", "u64_top", "wide_bottom", "shoup_top", "wmont_bottom", "u64_max")


def stream_primes(n: int) -> dict:
    """The word-size pair and the top of the 64-bit lanes (as boundary_primes),
    the bottom of the wide family (q >= 2^62: wide transforms, Shoup scalar
    product), the primes on either side of 2^63 (shoup_top: the Shoup
    remainder x s - hi(x s') q reaches up to 2q ~ 2^64; wmont_bottom: the first
    Montgomery one) and the last prime of the word."""
    b = boundary_primes(n)
    return {
        "u32_top": b["u32_top"],
        "u64_bottom": b["u64_bottom"],
        "u64_top": b["u64_top"],
        "wide_bottom": prime_above(1 << 62, n),
        "shoup_top": prime_below((1 << 63) - 1, n),
        "wmont_bottom": prime_above(1 << 63, n),
        "u64_max": prime_below(M64, n),
    }


def _distinct(values):
    out = []
    for v in values:
        if 0 <= v <= M64 and v not in out:
            out.append(v)
    return out


def stream_words(q: int) -> list:
    """Raw input words of the streaming kernels: the residues 0, 1, q-1 and
    their first and second unreduced copies, the middle of the range, the
    32-bit and 63-bit carries, and the top of the word (-q, -2, -1 mod 2^64)."""
    return _distinct([0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, q // 2, (1 << 32) - 1, 1 << 32,
                      (1 << 63) - 1, 1 << 63, (1 << 64) - q, M64 - 1, M64])


def stream_scalars(q: int) -> list:
    """Scalars (weights, lambdas) of the streaming kernels, any u64 read
    mod q: the residues at both ends, unreduced q and q+1, the middle, the
    Shoup/Montgomery threshold 2^63, the top of the word and two seeded
    random words."""
    rng = np.random.default_rng([q % (1 << 32), q >> 32, 63])
    return _distinct([0, 1, 2, q - 1, q, q + 1, q // 2, 1 << 63, M64] + [int(v) for v in rng.integers(
        0, M64, size=2, dtype=np.uint64, endpoint=True)])


def cross_ballots(q: int, n: int, polys: int):
    """(ballots [count, polys, n], scalars [count]), count = |S| |W|, in which
    every pair of stream_words(q) x stream_scalars(q) meets in every column:
    ballot i carries scalar S[i % |S|], and word j of its polys * n words is
    W[(j + i // |S|) % |W|]."""
    W, S = stream_words(q), stream_scalars(q)
    count = len(S) * len(W)
    i = np.arange(count)
    j = np.arange(polys * n)
    words = np.array(W, dtype=np.uint64)[(j[None, :] + i[:, None] // len(S)) % len(W)]
    scalars = np.array(S, dtype=np.uint64)[i % len(S)]
    return np.ascontiguousarray(words.reshape(count, polys, n)), scalars


# Ballot counts of the streaming sums: one, the unroll of 8 and its
# remainders, two rounds and one (None: the whole of cross_ballots).
STREAM_COUNTS = (1, 2, 7, 8, 9, 17, None)
# q = 97: this many terms of 2^64 - 1 leave 98 >= q (residue 1) in the
# accumulator's high word, which fold128 (tally_ops.hpp) then has to reduce.
HIGH_WORD_COUNT = 99
