"""Designed inputs for the range sweeps of the three newest kernel families
(helpers of test_range_inputs.py, test_gpu_scaled_bound.py,
test_gpu_ranges_galois.py and test_gpu_ranges_pack.py; plain Python and numpy,
no GPU).  Random words reach none of these states:

  bound_ciphertexts   ciphertext pairs whose tensor reaches the largest
                      coefficient the centred lift allows, 2 n ((q-1)/2)^2, so
                      that |rnd(t X / q)| sits just under the exactness bound
                      of the scale-invariant product
  scaled_bound_cases  the plaintext moduli and counts on either side of the
                      one-prime threshold t count n q < p1 and at the bound
                      t count n q < p1 p2
  pack_planted        keys, masks and bodies that drive the packing kernel's
                      signed 96-bit sum into its carry and sign corners
  pack_window         the same arrays filled cyclically from stream_words
  galois_operands     the adversarial rows of ntt_primes.base_rows as
                      ciphertexts, every row once as c0 and once as c1

test_range_inputs.py asserts on the CPU, with the references alone, that each
state is really reached."""
from __future__ import annotations

import numpy as np

import bfv_ref as R
import ntt_primes as P

M64 = (1 << 64) - 1

# the moduli of the scaled sweeps: (name, table) of ntt_primes
SWEEP_Q = ("lazy_top", "nonlazy_bottom", "wrap", "u32_top", "u64_bottom")
STREAM_Q = ("u64_top", "wide_bottom", "shoup_top", "wmont_bottom", "u64_max")
SCALED_NAMES = SWEEP_Q + STREAM_Q
# (n, modulus name) of the pairs at the bound (test_gpu_scaled_bound.py)
BOUND_SHAPES = [(1024, name) for name in SCALED_NAMES] + [(16, "u64_top"), (16, "u64_max")]

# the packing sweeps (test_gpu_ranges_pack.py): n = 64, in_dim = 8
PACK_N, PACK_IN_DIM = 64, 8
PACK_SLOTS = [0, 63, 5, 5, 1, 32, 9, 20]  # 0, n - 1 and a repeat; 32 is reached by no other slot
PACK_STATES_DECOMP = (16, 4)                                       # test_pack_accumulator_states
PACK_THRESHOLD_DECOMPS = [(1, 4), (31, 2), (32, 2), (33, 1), (63, 1)]  # test_pack_fast_threshold
# test_pack_window_words: (in_dim, level, base_log, batch), slots of degree n
PACK_WINDOW = (6, 4, 16, 5)


def pack_window_slots(n: int) -> list:
    return [0, n - 1, n // 2, n // 2, 1]


def scaled_prime(n: int, name: str) -> int:
    return P.sweep_primes(n)[name] if name in SWEEP_Q else P.stream_primes(n)[name]


# ---------------------------------------------------------------- scaled product
def _u(rows):
    return np.array(rows, dtype=np.uint64)


def bound_ciphertexts(n: int, q: int) -> dict:
    """name -> (ct1, ct2), [2, n] raw words each.  With h = (q - 1) / 2:

    all +h          every word h, paired with itself: X1[n-1] = 2 n h^2 and
                    X1[0] = -2 (n - 2) h^2
    sign-aligned    a all +h; b_0 = +h, b_j = (q + 1) / 2 (lift -h) for j >= 1:
                    the peak 2 n h^2 is at coefficient 0
    negated ...     the first operand negated word by word: the tensor changes
                    sign, the peaks are -2 n h^2
    all +h unreduced  the all +h pair with h + q in place of h in both
                    operands; left out where h + q does not fit the word"""
    h, m = (q - 1) // 2, (q + 1) // 2
    plus = np.full((2, n), h, dtype=np.uint64)
    minus = np.full((2, n), m, dtype=np.uint64)
    aligned = minus.copy()
    aligned[:, 0] = h
    out = {
        "all +h": (plus, plus.copy()),
        "sign-aligned": (plus, aligned),
        "negated all +h": (minus, plus.copy()),
        "negated sign-aligned": (minus, aligned.copy()),
    }
    if h + q <= M64:
        out["all +h unreduced"] = (plus + np.uint64(q), plus + np.uint64(q))
    return out


def one_prime(n: int, q: int, t: int, count: int) -> bool:
    """t count n q < p1: the first auxiliary prime alone determines the result."""
    return t * count * n * q < R.aux_for(q)[0]


def over_one_prime(n: int, q: int) -> int:
    """t1 + t1 // 64 + 1: at t1 + 1 the peak t n (q-1)^2 / (2 q) may still lie
    below p1 / 2 (it misses t n q / 2 by about t n), so a decision that took one
    prime there could go unnoticed; 1.6 % above t1 the peak is past p1 / 2 and
    the one-prime channel cannot hold it (asserted in test_range_inputs.py)."""
    t1 = (R.aux_for(q)[0] - 1) // (n * q)
    return t1 + t1 // 64 + 1


def scaled_bound_cases(n: int, q: int) -> list:
    """(t, count, expect_one_prime) with p1, p2 = aux_for(q):

    t1 = min(q - 1, (p1 - 1) // (n q))   the last single-prime t at count 1,
    t1 + 1                               the first two-prime one,
    over_one_prime(n, q)                 a two-prime one whose peak is past p1 / 2,
    max_t(n, q, p1, p2)                  the largest exact t,
    t7 = t1 // 7 at counts 7 and 8       one prime and two,
    max_t // 3 at max_count              where max_t < q - 1 (the bound binds).
    Values outside 2 <= t < q are left out (t1 = 0 from q ~ 2^52 on)."""
    p1, p2 = R.aux_for(q)
    cases = []

    def put(t, count):
        if 2 <= t < q and not any(c[:2] == (t, count) for c in cases):
            assert count <= R.max_count(n, q, t, p1, p2)
            cases.append((t, count, t * count * n * q < p1))

    t1 = min(q - 1, (p1 - 1) // (n * q))
    put(t1, 1)
    put(t1 + 1, 1)
    if t1 >= 64:
        put(over_one_prime(n, q), 1)
    mt = R.max_t(n, q, p1, p2)
    put(mt, 1)
    put(t1 // 7, 7)
    put(t1 // 7, 8)
    if mt < q - 1:
        put(mt // 3, R.max_count(n, q, mt // 3, p1, p2))
    return cases


def scaled_bound(n: int, q: int, t: int, count: int) -> int:
    """The largest |rnd(t X / q)| the channel in force represents."""
    p1, p2 = R.aux_for(q)
    return (p1 - 1) // 2 if t * count * n * q < p1 else (p1 * p2 - 1) // 2


def window_pairs(n: int, q: int):
    """(names, x, y): the rows of base_rows(n, q) as ciphertexts [b, 2, n], cut
    as Ctx.cts of test_gpu_ranges.py does, and the same rows rolled by 5."""
    from test_gpu_ranges import Ctx

    rows = Rows(n, q)
    b = len(rows.names)
    return rows.names, Ctx.cts(rows, b, 2), Ctx.cts(rows, b, 2, shift=5)


# ---------------------------------------------------------------- packing
def pack_word(digs, base_log: int) -> int:
    """The mask word whose pack_ref.digits are digs (l = 0 is the top digit)."""
    level = len(digs)
    w = sum(int(d) << ((level - 1 - l) * base_log) for l, d in enumerate(digs))
    assert w <= M64 and all(0 <= d < 1 << base_log for d in digs)
    return w


def pack_planted(n: int, q: int, base_log: int, level: int, in_dim: int, slots) -> dict:
    """name -> (key [entries, 2, n], lwe_a [S, in_dim], lwe_b [S]) of ONE output
    ciphertext.  S(p, j) below is the exact signed sum of the kernel's terms
    +-(d key mod 2^64) and bodies at output word (p, j): a term of slot h is
    subtracted at j >= h and added at j < h.  entries = in_dim level is even.

    half       every digit 2^(base_log-1), every key word 2^(64-base_log): all
               terms 2^63, so S = (adds - subs) entries 2^63 = 0 mod 2^64;
               negative at j = n - 1 (the branch lo == 0 of a negative sum),
               positive at word 0
    ones       entry 0 has digit 1, the others 0; key words 1 at columns 0 and
               n - 1 of entry 0, else 0: S = -1 at j = h and +1 at j = h - 1 for
               a slot h that no other slot touches; bodies 2^64 - 1, which at
               (0, h) land on the low word 2^64 - 1
    minus      every digit d = 2^base_log - 1 (odd), every key word -d^-1 mod
               2^64: all terms 2^64 - 1; at j = n - 1 all S entries terms are
               subtracted, the largest magnitude of the shape
    minus added  the same with the masks of slot 0 zero: word 0 holds additions
               only (and a mask whose digits are all 0 beside the all-ones ones)
    q is not used by the sums: the key words are raw u64."""
    S, entries = len(slots), in_dim * level
    assert entries % 2 == 0 and (level - 1) * base_log < 64 and base_log * level <= 64
    top = (1 << base_log) - 1
    shape = (entries, 2, n)
    zeros_b = np.zeros(S, dtype=np.uint64)
    out = {}

    half_word = pack_word([1 << (base_log - 1)] * level, base_log)
    out["half"] = (np.full(shape, 1 << (64 - base_log), dtype=np.uint64),
                   np.full((S, in_dim), half_word, dtype=np.uint64), zeros_b.copy())

    key = np.zeros(shape, dtype=np.uint64)
    key[0, :, 0] = 1
    key[0, :, n - 1] = 1
    lwe_a = np.zeros((S, in_dim), dtype=np.uint64)
    lwe_a[:, 0] = pack_word([1] + [0] * (level - 1), base_log)
    out["ones"] = (key, lwe_a, np.full(S, M64, dtype=np.uint64))

    ones_word = pack_word([top] * level, base_log)
    kw = (-pow(top, -1, 1 << 64)) % (1 << 64)
    assert top * kw % (1 << 64) == M64
    key = np.full(shape, kw, dtype=np.uint64)
    lwe_a = np.full((S, in_dim), ones_word, dtype=np.uint64)
    out["minus"] = (key, lwe_a, zeros_b.copy())
    lwe_a = lwe_a.copy()
    lwe_a[[i for i, h in enumerate(slots) if h == 0]] = 0
    out["minus added"] = (key.copy(), lwe_a, zeros_b.copy())
    return out


def pack_sums(n: int, base_log: int, level: int, key, lwe_a, lwe_b, slots, bodies: bool = True):
    """S(p, j) in Python integers: [2][n].  The signs are the kernel's (a term
    of slot h is subtracted at j >= h, added below; the body is added at
    (0, h)); the value mod q is pack_ref's out without prev."""
    import pack_ref

    S = [[0] * n for _ in range(2)]
    for s, h in enumerate(slots):
        d = [x for word in lwe_a[s] for x in pack_ref.digits(word, base_log, level)]
        for p in range(2):
            for j in range(n):
                k = (j - h) % n
                total = sum((d[e] * int(key[e][p][k])) & M64 for e in range(len(d)) if d[e])
                S[p][j] += -total if j >= h else total
        if bodies:
            S[0][h] += int(lwe_b[s])
    return S


def pack_window(n: int, q: int, in_dim: int, level: int, batch: int, S: int):
    """key [entries, 2, n], lwe_a [batch, S, in_dim], lwe_b [batch, S], prev
    [batch, 2, n] filled cyclically from stream_words(q).  The masks and the
    bodies run through the list in the order of their words in memory, so with
    batch S in_dim >= len(stream_words) every word is a mask (and with S
    in_dim >= len, in every ciphertext); along k every key word follows every
    other at offset (k + e + p), so each mask word meets every key word
    (n >= len; asserted in test_range_inputs.py)."""
    W = _u(P.stream_words(q))
    m = len(W)
    assert n >= m and batch * S * in_dim >= m and batch * S >= m
    e, p, k = np.ogrid[:in_dim * level, :2, :n]
    key = W[(k + e + p) % m]
    lwe_a = W[np.arange(batch * S * in_dim) % m].reshape(batch, S, in_dim)
    lwe_b = W[(np.arange(batch * S) + 1) % m].reshape(batch, S)
    c, p, k = np.ogrid[:batch, :2, :n]
    prev = W[(k + 5 * p + 7 * c + 2) % m]
    return tuple(np.ascontiguousarray(a) for a in (key, lwe_a, lwe_b, prev))


# ---------------------------------------------------------------- Galois
class Rows:
    """The part of test_gpu_ranges.Ctx that cuts operands, without a GPU."""

    def __init__(self, n: int, q: int):
        self.n, self.q = n, q
        self.names, self.base = P.base_rows(n, q)


def galois_operands(ctx, shift: int):
    """Ctx.cts(b, 2, shift) with b = len(ctx.names): over shift 0 and 1 every
    base row is once a c0 and once a c1.  ctx: a Ctx of test_gpu_ranges.py or
    a Rows."""
    from test_gpu_ranges import Ctx

    assert shift in (0, 1)
    return Ctx.cts(ctx, len(ctx.names), 2, shift)


def galois_digit_edges(n: int, q: int, base_log: int):
    """Two ciphertexts [2, 2, n] for the decomposition of sigma_g(c1): c1 all
    2^base_log - 1 (at index 0, which no g negates, the lowest digit is all
    ones and the others 0) against c0 all q - 1, and c1 = 0 against the same."""
    top = min(q - 1, (1 << base_log) - 1)
    ct = np.zeros((2, 2, n), dtype=np.uint64)
    ct[:, 0] = q - 1
    ct[0, 1] = top
    return ct


def operand_rows(ctx, shift: int):
    """[(name of c0's row, name of c1's row)] of galois_operands(ctx, shift)."""
    b = len(ctx.names)
    return [(ctx.names[(2 * i + shift) % b], ctx.names[(2 * i + 1 + shift) % b]) for i in range(b)]


def plant_words(ct, words):
    """A copy of ct [b, 2, n] with `words` planted in c0 and c1 of its last
    ciphertext, each at an even and at an odd index."""
    ct = ct.copy()
    w = _u(list(words) + list(words)[::-1] + list(words)[:1])  # odd length: the second run changes parity
    w = w[:ct.shape[-1]]
    ct[-1, 0, :len(w)] = w
    ct[-1, 1, -len(w):] = w
    return ct
