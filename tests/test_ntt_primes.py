"""CPU checks of tests/ntt_primes.py: the primality test, the boundary primes
of every degree (pinned values), the side of the lazy inequality each one
falls on, that the oracle accepts them, and the adversarial row builder."""
import numpy as np
import pytest

import ntt_primes as P
import oracle

T62 = 1 << 62

# log2 n -> the pinned primes (None: not pinned for that degree)
PINNED = {
    2: dict(lazy_top=536870849, nonlazy_bottom=536871001, u32_top=1073741689, u64_bottom=1073741833,
            u64_top=T62 - 87),
    6: dict(lazy_top=268432897, nonlazy_bottom=268437889, u64_top=T62 - 4991),
    10: dict(lazy_top=178956289, nonlazy_bottom=178997249, u32_top=1073707009, u64_bottom=1073750017,
             u64_top=T62 - 22527),
    12: dict(lazy_top=153231361, nonlazy_bottom=153468929),
    14: dict(lazy_top=133857281, nonlazy_bottom=134250497, u32_top=1073643521, u64_bottom=1073872897,
             u64_top=T62 - 65535),
}


def test_miller_rabin_small_numbers_and_pseudoprimes():
    sieve = [True] * 5000
    sieve[0] = sieve[1] = False
    for i in range(2, 71):
        if sieve[i]:
            for j in range(i * i, 5000, i):
                sieve[j] = False
    assert [P.is_prime(i) for i in range(5000)] == sieve
    # strong pseudoprimes to the small bases, Carmichael numbers, squares of primes
    for c in (2047, 1373653, 25326001, 3215031751, 2152302898747, 3474749660383, 341550071728321,
              3825123056546413051, 561, 41041, 825265, 132120577 ** 2, (2 ** 31 - 1) ** 2):
        assert not P.is_prime(c), c
    for p in (2, 37, 41, 132120577, 4611686018326724609, 2 ** 31 - 1, 2 ** 61 - 1, 18446744069414584321,
              2 ** 64 - 59):
        assert P.is_prime(p), p


@pytest.mark.parametrize("logn", sorted(PINNED))
def test_pinned_boundary_primes(logn):
    got = P.boundary_primes(1 << logn)
    for name, q in PINNED[logn].items():
        assert got[name] == q, (logn, name)


@pytest.mark.parametrize("logn", range(2, 15))
def test_boundary_primes_sides(logn):
    n = 1 << logn
    b = P.boundary_primes(n)
    assert tuple(b) == P.BOUNDARY_NAMES
    for name, q in b.items():
        assert P.is_prime(q) and q % (2 * n) == 1, (logn, name)
    # nearest: no prime of the progression lies between the pair
    for lo, hi in ((b["lazy_top"], b["nonlazy_bottom"]), (b["u32_top"], b["u64_bottom"])):
        assert not any(P.is_prime(c) for c in range(lo + 2 * n, hi, 2 * n)), logn
    assert not any(P.is_prime(c) for c in range(b["u64_top"] + 2 * n, T62, 2 * n)), logn
    # the lazy inequality of fhe_ctx_create, (4 + 2 log2 N) q <= 2^32, and the word size q < 2^30
    k = 4 + 2 * logn
    assert k * b["lazy_top"] <= 1 << 32 < k * b["nonlazy_bottom"]
    assert b["nonlazy_bottom"] < b["u32_top"] < 1 << 30 < b["u64_bottom"] < b["u64_top"] < T62
    assert [P.is_lazy(n, b[x]) for x in P.BOUNDARY_NAMES] == [True, False, False, False, False]
    assert [P.word_bits(b[x]) for x in P.BOUNDARY_NAMES] == [32, 32, 32, 64, 64]
    assert P.prime_below(b["lazy_top"], n) == b["lazy_top"]
    assert P.prime_above(b["lazy_top"], n) == b["nonlazy_bottom"]
    # the benchmark's modulus stays lazy at its degree
    assert P.is_lazy(16384, 132120577)


@pytest.mark.parametrize("logn", range(2, 15))
def test_wrap_prime(logn):
    """A 32-bit, non-lazy modulus between nonlazy_bottom and u32_top at which
    (3 + L) q - 1 >= 2^32, and the two facts its row relies on, on a model of
    the lazy butterfly (fhe_arith.hpp ct_lazy with the Shoup product
    x w - floor(x w' / 2^32) q, w' = floor(w 2^32 / q)): a lower input 0
    gives b = 0, a nonzero multiple of q gives b = q, so the top word of the
    sparse row gains q per stage."""
    n = 1 << logn
    b = P.boundary_primes(n)
    q = P.wrap_prime(n)
    assert P.is_prime(q) and q % (2 * n) == 1
    assert b["nonlazy_bottom"] < q < b["u32_top"] and not P.is_lazy(n, q) and P.word_bits(q) == 32
    assert (3 + logn) * q - 1 >= 1 << 32
    assert not any(P.is_prime(c) for c in range(q - 2 * n, (1 << 32) // (3 + logn), -2 * n))
    assert P.sweep_primes(n) == dict(b, wrap=q) and tuple(P.sweep_primes(n)) == P.SWEEP_NAMES

    def shoup(x, w):
        return (x * w - (x * ((w << 32) // q) >> 32) * q) % (1 << 32)

    psi = oracle.NTT(n, q).psi
    top = 4 * q - 1
    for s in range(1, logn):  # stages above 0: twiddle of the butterfly that holds the top word
        w = pow(psi, ((1 << s) - 1) * (n >> (s + 1)), q)
        lower = (2 + (s - 1)) * q if s > 1 else 2 * q  # a nonzero multiple of q (its value does not matter)
        assert shoup(0, w) == 0 and shoup(lower, w) == q
        top = top - shoup(lower, w) + 2 * q
    assert top == (3 + logn) * q - 1


@pytest.mark.parametrize("logn", range(2, 15))
def test_oracle_accepts_boundary_primes(logn):
    """The oracle's root search succeeds for every boundary prime, and
    forward then inverse is the identity (n <= 1024)."""
    n = 1 << logn
    for name, q in P.sweep_primes(n).items():
        t = oracle.NTT(n, q)
        psi = t.psi
        assert pow(psi, n, q) == q - 1, (logn, name)
        if n <= 1024:
            _, rows = P.base_rows(n, q)
            x = rows % np.uint64(q)
            assert (t.inverse(t.forward(x)) == x).all(), (logn, name)


@pytest.mark.parametrize("logn,bound", [(15, 126322567), (16, 119304647)])
def test_two_pass_degrees_premise(logn, bound):
    """The premise of test_gpu_ranges_big.py: at N = 32768 / 65536 the usual
    27-bit prime is past the lazy bound, so only lazy_top reaches the lazy row
    kernel of ntt_big.hip; the six sweep primes exist, fall on the stated sides
    and have the word sizes test_window_rows_vs_oracle states."""
    n = 1 << logn
    assert P.lazy_bound(n) == bound and (1 << 32) // (4 + 2 * logn) == bound
    s = P.sweep_primes(n)
    assert tuple(s) == P.SWEEP_NAMES and len(set(s.values())) == 6
    for name, q in s.items():
        assert P.is_prime(q) and q % (2 * n) == 1, (logn, name)
        assert P.word_bits(q) == (64 if name in ("u64_bottom", "u64_top") else 32), (logn, name)
        assert P.is_lazy(n, q) == (name == "lazy_top"), (logn, name)
        assert pow(oracle.NTT(n, q).psi, n, q) == q - 1, (logn, name)
    assert s["lazy_top"] <= bound < s["nonlazy_bottom"] < s["wrap"] < s["u32_top"] < 1 << 30
    assert 1 << 30 < s["u64_bottom"] < s["u64_top"] < T62
    assert (3 + logn) * s["wrap"] - 1 >= 1 << 32
    p27 = 132120577
    assert p27 % (2 * n) == 1 and p27 > bound and not P.is_lazy(n, p27) and P.word_bits(p27) == 32
    assert P.is_lazy(16384, p27)  # (it is lazy at the largest fused degree)


@pytest.mark.parametrize("logn", range(2, 15))
def test_limb_families(logn):
    """Three rings of three distinct NTT primes, every limb of a ring in the
    same kernel family (word and laziness), so that fhe_rns_ctx_create takes
    the one-launch path for each."""
    n = 1 << logn
    fam = P.limb_families(n)
    s = P.sweep_primes(n)
    assert tuple(fam) == P.LIMB_FAMILIES
    for name, ring in fam.items():
        assert len(ring) == 3 and len(set(ring)) == 3, (logn, name)
        for q in ring:
            assert P.is_prime(q) and q % (2 * n) == 1 and q < T62, (logn, name, q)
    assert all(P.is_lazy(n, q) and P.word_bits(q) == 32 for q in fam["lazy"])
    assert all(not P.is_lazy(n, q) and P.word_bits(q) == 32 for q in fam["nonlazy32"])
    assert all(not P.is_lazy(n, q) and P.word_bits(q) == 64 for q in fam["u64"])
    top, below, least = fam["lazy"]
    assert top == s["lazy_top"] and below < top and P.prime_above(below, n) == top
    assert not any(P.is_prime(c) for c in range(2 * n + 1, least, 2 * n)) and least < 1 << 20 < below
    assert fam["nonlazy32"] == [s["nonlazy_bottom"], s["wrap"], s["u32_top"]]
    lo, mid, hi = fam["u64"]
    assert (lo, hi) == (s["u64_bottom"], s["u64_top"]) and lo < 1 << 45 < mid < hi
    assert not any(P.is_prime(c) for c in range(mid - 2 * n, 1 << 45, -2 * n))


def test_pinned_limb_families():
    assert P.limb_families(16)["lazy"] == [357913921, 357913793, 97]
    f = P.limb_families(16384)
    assert f["lazy"] == [133857281, 132710401, 65537]
    assert f["nonlazy32"] == [134250497, 253001729, 1073643521]


@pytest.mark.parametrize("n,q", [(4, 536870849), (8, 17), (16, 97), (64, 268437889), (1024, 1073707009),
                                 (1024, T62 - 22527)])
@pytest.mark.parametrize("inverse", [False, True])
def test_base_rows(n, q, inverse):
    names, rows = P.base_rows(n, q, inverse)
    lim = (2 if inverse else 4) * q
    assert rows.dtype == np.uint64 and rows.shape == (len(names), n) and len(set(names)) == len(names)
    by = dict(zip(names, rows))
    for v, name in ((0, "0"), (q - 1, "q-1"), (q, "q"), (lim - 1, "lim-1"), (lim, "lim"), (lim + 1, "lim+1"),
                    (P.M64, "2^64-1")):
        assert (by["const " + name] == np.uint64(v)).all()
    assert (rows == np.uint64(2 * q)).all(axis=1).any()  # "2q" forward, "lim" inverse
    assert ("const 3q" in by) == ("const 2q" in by) == (not inverse)
    if not inverse:
        assert (by["const 3q"] == np.uint64(3 * q)).all()
    assert ("const 2^32-1" in by) == (q < 1 << 30)
    assert int(by["sparse first"][0]) == lim - 1 and not by["sparse first"][1:].any()
    assert int(by["sparse last"][-1]) == lim - 1 and not by["sparse last"][:-1].any()
    assert not by["sparse alternating"][0::2].any() and (by["sparse alternating"][1::2] == np.uint64(lim - 1)).all()
    mixed, slow = by["mixed in-window"], by["mixed one slow word per 16"]
    assert (mixed < np.uint64(lim)).all()
    g = min(n, 16)
    out = (slow >= np.uint64(lim)).reshape(-1, g)
    assert (out.sum(axis=1) == 1).all()
    assert ((slow == mixed) | (slow >= np.uint64(lim))).all() and (slow == np.uint64(lim)).any()
    assert (by["canonical"] < np.uint64(q)).all()
    # deterministic
    assert (P.base_rows(n, q, inverse)[1] == rows).all()
    assert "canonical" not in P.base_rows(n, q, inverse, reduced=True)[0]


def test_base_rows_wide_modulus():
    """q >= 2^62: no window (lim = q), no value past the word, no repeated row."""
    n, q = 64, P.QG
    names, rows = P.base_rows(n, q)
    consts = [int(r[0]) for nm, r in zip(names, rows) if nm.startswith("const")]
    assert consts == [0, q - 1, q, q + 1, P.M64]
    by = dict(zip(names, rows))
    assert (by["mixed in-window"] < np.uint64(q)).all()
    assert ((by["mixed one slow word per 16"] >= np.uint64(q)).reshape(-1, 16).sum(axis=1) == 1).all()
    assert int(by["sparse last"][-1]) == q - 1


@pytest.mark.parametrize("n,ppb", [(4, 256), (64, 16), (1024, 4), (16384, 1)])
@pytest.mark.parametrize("reduced", [False, True])
def test_multiply_partners_pairings(n, ppb, reduced):
    """The products the GPU sweeps check contain both operands at the top of
    the window, and every extreme row against a nonzero product."""
    q = P.boundary_primes(n)["nonlazy_bottom"]
    names, base = P.base_rows(n, q, reduced=reduced)
    for total in (max(ppb + 3, 4 * len(names)), ppb + 3):  # test_gpu_ranges / test_gpu_negacyclic tilings
        x = P.tile_rows(base, total, ppb)
        parts = P.multiply_partners(x, names, q)
        assert tuple(parts) == ("rolled", "squares", "canonical")
        row_of = {r.tobytes(): nm for nm, r in zip(names, base)}
        pairs = {(names[i % len(names)], row_of.get(y[i].tobytes(), "canonical nonzero"))
                 for y in parts.values() for i in range(x.shape[0])}
        for nm in ("const lim-1", "sparse first", "sparse last", "sparse alternating", "const 3q",
                   "mixed one slow word per 16"):
            assert (nm, nm) in pairs and (nm, "canonical nonzero") in pairs, (total, nm)
        canon = parts["canonical"]
        assert (canon == canon[0]).all() and (canon < np.uint64(q)).all() and canon[0].any()
        # the rolled operand pairs rows of different kinds
        assert any(a != b and not {a, b} & {"const 0", "const q", "const 2q", "const 3q", "const lim"}
                   for a, b in pairs if b != "canonical nonzero")


def test_tile_and_weight_rows():
    rows = np.arange(12, dtype=np.uint64).reshape(3, 4)
    t = P.tile_rows(rows, 8, ragged_for=4)
    assert t.shape == (9, 4) and (t[3:6] == rows).all() and (t[8] == rows[2]).all()
    assert P.tile_rows(rows, 2).shape == (3, 4)
    w = P.weight_rows(4, 17, 13, 3)
    assert (w[0:3] < 17).all() and (w[3:6] == 16).all() and (w[6:9] == 17).all() and (w[9:12] == P.M64).all()
    assert (w[12] < 17).all()


# ---------------------------------------------------------------- streaming helpers (the 2^63 edge)
T63, T64 = 1 << 63, 1 << 64


def test_pinned_stream_primes():
    s = P.stream_primes(16)
    assert (s["wide_bottom"], s["shoup_top"], s["wmont_bottom"], s["u64_max"]) == (
        4611686018427388097, 9223372036854775073, 9223372036854776257, 18446744073709551521)


@pytest.mark.parametrize("logn", range(2, 17))
def test_stream_primes_sides(logn):
    """Each prime is prime, 1 mod 2n, on the stated side of its threshold, and
    the nearest such prime to it."""
    n = 1 << logn
    s = P.stream_primes(n)
    b = P.boundary_primes(n)
    assert tuple(s) == P.STREAM_NAMES
    for name, q in s.items():
        assert P.is_prime(q) and q % (2 * n) == 1, (logn, name)
    assert all(s[x] == b[x] for x in ("u32_top", "u64_bottom", "u64_top"))
    assert s["u32_top"] < 1 << 30 < s["u64_bottom"] < s["u64_top"] < T62 < s["wide_bottom"]
    assert s["wide_bottom"] < s["shoup_top"] < T63 < s["wmont_bottom"] < s["u64_max"] < T64
    step = 2 * n

    def none_between(lo, hi):  # no prime of the progression strictly between lo and hi
        first = lo + (1 - lo) % step
        if first == lo:
            first += step
        return not any(P.is_prime(c) for c in range(first, hi, step))

    assert none_between(s["u32_top"], 1 << 30) and none_between(1 << 30, s["u64_bottom"])
    assert none_between(s["u64_top"], T62) and none_between(T62, s["wide_bottom"])
    assert none_between(s["shoup_top"], T63) and none_between(T63, s["wmont_bottom"])
    assert none_between(s["u64_max"], T64)


@pytest.mark.parametrize("q", [17, 97, 1073741689, T62 - 87, 4611686018427388097, 9223372036854775073,
                               9223372036854776257, 18446744073709551521, P.QG])
def test_stream_words_and_scalars(q):
    W, S = P.stream_words(q), P.stream_scalars(q)
    assert len(set(W)) == len(W) and len(set(S)) == len(S)
    assert all(0 <= v < T64 for v in W + S)
    want = [0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, q // 2, (1 << 32) - 1, 1 << 32, T63 - 1, T63, T64 - q,
            T64 - 2, T64 - 1]
    assert set(W) == {v for v in want if v < T64}
    assert set(S) >= {0, 1, 2, q - 1, q, q + 1, q // 2, T63, T64 - 1} and len(S) <= 11
    assert len(S) - len({0, 1, 2, q - 1, q, q + 1, q // 2, T63, T64 - 1}) == 2  # the two random words
    assert P.stream_scalars(q) == S  # deterministic
    # both kinds of word on either side of q, and residues 0 and q-1 among both lists
    for vals in (W, S):
        assert any(v < q for v in vals) and any(v >= q for v in vals)
        assert {0, q - 1} <= {v % q for v in vals}


@pytest.mark.parametrize("n,q,polys", [(4, 17, 1), (16, 97, 2), (16, 9223372036854775073, 3),
                                       (16, 18446744073709551521, 1), (4, 9223372036854775837, 2)])
def test_cross_ballots_hold_the_cross_product(n, q, polys):
    W, S = P.stream_words(q), P.stream_scalars(q)
    a, s = P.cross_ballots(q, n, polys)
    count = len(W) * len(S)
    assert a.dtype == s.dtype == np.uint64 and a.shape == (count, polys, n) and s.shape == (count,)
    flat = a.reshape(count, -1)
    full = {(w, c) for w in W for c in S}
    for j in range(polys * n):  # every column holds every pair
        assert {(int(flat[i, j]), int(s[i])) for i in range(count)} == full, j
    assert [int(v) for v in s[:len(S)]] == S and [int(v) for v in flat[0, :min(len(W), polys * n)]] == W[:polys * n]


def test_stream_counts_carry_into_the_high_word():
    """The sums of the streaming tests leave the 64-bit word: two or more
    terms of 2^64 - 1 have a non-zero high word, and at q = 97 the count of
    the all-ones case leaves a high word >= q (fold128 reduces hi too)."""
    assert P.STREAM_COUNTS == (1, 2, 7, 8, 9, 17, None)
    full = len(P.stream_words(97)) * len(P.stream_scalars(97))
    for count in P.STREAM_COUNTS:
        c = full if count is None else count
        total = sum(P.M64 for _ in range(c))
        assert (total >> 64 != 0) == (c > 1), c
    assert sum(P.M64 for _ in range(P.HIGH_WORD_COUNT)) >> 64 >= 97
    assert (sum(P.M64 for _ in range(P.HIGH_WORD_COUNT)) >> 64) % 97 != 0  # and its residue is not 0
    assert full >= P.HIGH_WORD_COUNT
