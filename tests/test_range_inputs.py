"""Conditions on the designed inputs of tests/range_inputs.py, checked on the
CPU with the references alone (bfv_ref.py, pack_ref.py, galois_ref.py): the GPU
sweeps that use them (test_gpu_scaled_bound.py, test_gpu_ranges_pack.py,
test_gpu_ranges_galois.py) cannot pass vacuously while these hold."""
import numpy as np
import pytest

import bfv_ref as R
import galois_ref
import ntt_primes as P
import pack_ref
import range_inputs as I

M64 = (1 << 64) - 1
BOUND_SHAPES = I.BOUND_SHAPES  # the shapes test_gpu_scaled_bound.py runs


# ---------------------------------------------------------------- scaled product
_PEAKS = {}


def peaks(n, q):
    """name -> (largest, smallest) coefficient of the tensor of each pair of
    bound_ciphertexts, computed once per shape."""
    if (n, q) not in _PEAKS:
        out = {}
        for name, (a, b) in I.bound_ciphertexts(n, q).items():
            X = R.tensor(a.tolist(), b.tolist(), q)
            flat = [x for row in X for x in row]
            out[name] = (max(flat), min(flat))
        _PEAKS[(n, q)] = out
    return _PEAKS[(n, q)]


def reach(n, q, t, count):
    """Largest |rnd(t count X / q)| over the pairs (rnd is monotonic: the
    extreme coefficients decide)."""
    return max(abs(R.rnd(t * count * x, q)) for pk in peaks(n, q).values() for x in pk)


@pytest.mark.parametrize("n,name", BOUND_SHAPES)
def test_bound_ciphertexts_reach_the_exactness_bound(n, name):
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    h = (q - 1) // 2
    pk = peaks(n, q)
    assert pk["all +h"] == (2 * n * h * h, -2 * (n - 2) * h * h)
    assert pk["sign-aligned"][0] == 2 * n * h * h
    assert pk["negated all +h"][1] == pk["negated sign-aligned"][1] == -2 * n * h * h
    if "all +h unreduced" in pk:
        assert pk["all +h unreduced"] == pk["all +h"]
    X1 = R.tensor(*(x.tolist() for x in I.bound_ciphertexts(n, q)["sign-aligned"]), q)[1]
    assert X1[0] == 2 * n * h * h  # the peak is at coefficient 0
    t1 = min(q - 1, (p1 - 1) // (n * q))
    mt = R.max_t(n, q, p1, p2)
    cases = I.scaled_bound_cases(n, q)
    assert cases
    for t, count, one in cases:
        bound = I.scaled_bound(n, q, t, count)
        got = reach(n, q, t, count)
        ratio = got / bound
        print(n, name, "t", t, "count", count, "one prime", one, "reach / bound %.10f" % ratio)
        # never past the bound -- and never AT it: rnd(t X) = +-bound needs |X| >= (bound - 1/2) q / t,
        # above the largest tensor coefficient whenever t count n q stays below the modulus of the channel
        assert got < bound, (t, count)
        binds = (t == t1 and count == 1) or (t == t1 // 7 and count == 7) or (mt < q - 1 and (t == mt or t == mt // 3))
        if binds:
            assert ratio >= 0.99, (t, count, ratio)
        if mt < q - 1 and t == mt:
            # 1.0 to every printed digit (stated for (1024, u64_max) and (16, u64_top)): the peak misses
            # the bound by about t n + (p1 p2 - 1) mod (n q), below 2^-40 of it
            assert (bound - got) * 10 ** 6 <= bound, (t, ratio)
    if (n, name) in ((1024, "u64_max"), (16, "u64_top")):
        assert mt < q - 1 and (mt, 1, False) in cases


def test_bound_reach_at_the_benchmark_modulus():
    """(1024, 132120577): t1 = 34087041 and the all +h pair reaches 0.99999996 of (p1 - 1) / 2."""
    n, q = 1024, 132120577
    p1, p2 = R.aux_for(q)
    t1 = min(q - 1, (p1 - 1) // (n * q))
    assert t1 == 34087041
    hi, lo = peaks(n, q)["all +h"]
    ratio = abs(R.rnd(t1 * hi, q)) / ((p1 - 1) // 2)
    assert abs(ratio - 0.99999996) < 1e-8 and ratio < 1


@pytest.mark.parametrize("n,name", BOUND_SHAPES)
def test_one_prime_expectation(n, name):
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    cases = I.scaled_bound_cases(n, q)
    for t, count, one in cases:
        assert 2 <= t < q and 1 <= count <= R.max_count(n, q, t, p1, p2)
        assert one == (t * count * n * q < p1) == I.one_prime(n, q, t, count)
    if q < 1 << 32 and n == 1024:
        assert {c[2] for c in cases if c[1] == 1} == {True, False}
        assert {c[1]: c[2] for c in cases if c[1] in (7, 8)} == {7: True, 8: False}
        t1 = min(q - 1, (p1 - 1) // (n * q))
        assert (t1, 1, True) in cases and (t1 + 1, 1, False) in cases
        # a wrongly taken one-prime channel cannot pass here: the peak is past p1 / 2
        over = I.over_one_prime(n, q)
        assert (over, 1, False) in cases and reach(n, q, over, 1) > (p1 - 1) // 2
        assert reach(n, q, t1 // 7, 8) > (p1 - 1) // 2
    assert (R.max_t(n, q, p1, p2), 1) in {c[:2] for c in cases}


@pytest.mark.parametrize("n,name", [(1024, "u64_top"), (1024, "u64_max"), (1024, "wide_bottom"), (16, "u64_top")])
def test_dot_count_at_a_third_of_max_t(n, name):
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    mt = R.max_t(n, q, p1, p2)
    assert mt < q - 1
    mc = R.max_count(n, q, mt // 3, p1, p2)
    assert 3 <= mc <= 6
    assert (mt // 3, mc, False) in I.scaled_bound_cases(n, q)
    assert reach(n, q, mt // 3, mc) / ((p1 * p2 - 1) // 2) >= 0.99


@pytest.mark.parametrize("n,name", BOUND_SHAPES)
def test_edge_values_hold_the_bound_itself_at_max_t(n, name):
    """What no tensor reaches, the stand-alone rounding step is given directly."""
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    t = R.max_t(n, q, p1, p2)
    bound = (p1 * p2 - 1) // 2
    xs = R.edge_values(q, t, p1, p2, count=24)
    assert len(xs) <= n * 64 and {bound, -bound} <= {R.rnd(t * v, q) for v in xs}


def test_auxiliary_primes():
    for i in (1, 2):
        p = R.AUX_PRIMES[i]
        assert P.is_prime(p) and p % 2048 == 1 and p < 1 << 62
        assert R.aux_for(p) == tuple(x for x in R.AUX_PRIMES if x != p)
        assert len(R.aux_for(p)) == 2 and p not in R.aux_for(p)
    assert R.aux_for(97) == R.AUX_PRIMES[:2]


def test_window_pairs_meet_the_rows_rolled_by_five():
    n, q = 16, P.stream_primes(16)["u64_top"]
    names, x, y = I.window_pairs(n, q)
    b = len(names)
    base = P.base_rows(n, q)[1]
    assert x.shape == y.shape == (b, 2, n)
    for i in range(b):
        for comp in range(2):
            assert (x[i, comp] == base[(2 * i + comp) % b]).all() and (y[i, comp] == base[(2 * i + comp + 5) % b]).all()
    assert {(2 * i) % b for i in range(b)} | {(2 * i + 1) % b for i in range(b)} == set(range(b))


# ---------------------------------------------------------------- packing
PACK_SLOTS = I.PACK_SLOTS
PACK_SHAPES = [I.PACK_STATES_DECOMP] + I.PACK_THRESHOLD_DECOMPS  # every (base_log, level) test_gpu_ranges_pack.py plants


@pytest.mark.parametrize("bl,lv", PACK_SHAPES)
def test_pack_planted_states(bl, lv):
    n, in_dim, slots = I.PACK_N, I.PACK_IN_DIM, PACK_SLOTS
    entries, S = in_dim * lv, len(PACK_SLOTS)
    planted = I.pack_planted(n, 7681, bl, lv, in_dim, slots)
    sums = {k: I.pack_sums(n, bl, lv, *v, slots) for k, v in planted.items()}
    two64 = 1 << 64

    # half: S = 0 mod 2^64, negative at n - 1 (j >= every h), positive at word 0
    for p in range(2):
        assert all(v % two64 == 0 for v in sums["half"][p])
        assert sums["half"][p][n - 1] == -S * entries * (1 << 63) < 0
        assert sums["half"][p][0] == (S - 2) * entries * (1 << 63) > 0
    # ones: -1 at j = 32 and +1 at j = 31 (slot 32 alone reaches them)
    terms = I.pack_sums(n, bl, lv, *planted["ones"], slots, bodies=False)
    assert terms[1][32] == -1 and terms[1][31] == 1 and terms[0][31] == 1
    # the body 2^64 - 1 of slot 32 -- in the last group of four slots, so every term of
    # the word is in the sum when it is added -- lands on the low word 2^64 - 1
    assert slots.index(32) >= S - 4 and int(planted["ones"][2][slots.index(32)]) == M64
    assert terms[0][32] % two64 == M64 and sums["ones"][0][32] == two64 - 2
    # minus: every term 2^64 - 1, all S * entries of them subtracted at n - 1
    for p in range(2):
        assert sums["minus"][p][n - 1] == -S * entries * M64
        assert sums["minus added"][p][0] == (S - 1) * entries * M64  # additions only
        assert sums["minus added"][p][n - 1] == -(S - 1) * entries * M64
    top = (1 << bl) - 1
    words = {int(w) for w in planted["minus added"][1].reshape(-1)}
    assert 0 in words and any(pack_ref.digits(w, bl, lv) == [top] * lv for w in words)
    # the sums are the reference's words
    for name, (key, lwe_a, lwe_b) in planted.items():
        for q in (7681, P.stream_primes(64)["u64_max"]):
            want = pack_ref.pack_formula(q, n, bl, lv, key, lwe_a[None], lwe_b[None], slots)[0]
            assert [[v % q for v in row] for row in sums[name]] == want.tolist(), (name, q)


@pytest.mark.parametrize("bl,lv", [(16, 4), (33, 1)])
def test_pack_references_agree_on_the_planted_inputs(bl, lv):
    n, in_dim, slots = 4, 8, [0, 3, 1, 1, 2, 3, 0, 2]
    for q in (7681, P.stream_primes(64)["shoup_top"], P.stream_primes(64)["u64_max"]):
        for name, (key, lwe_a, lwe_b) in I.pack_planted(n, q, bl, lv, in_dim, slots).items():
            prev = np.array(P.stream_words(q)[:2 * n], dtype=np.uint64).reshape(2, n)
            for pv in (None, prev):
                want = pack_ref.pack_formula_int(q, n, bl, lv, key, lwe_a, lwe_b, slots, pv)
                got = pack_ref.pack_formula(q, n, bl, lv, key, lwe_a[None], lwe_b[None], slots,
                                            None if pv is None else pv[None])
                assert got[0].tolist() == want, (q, name, pv is None)


@pytest.mark.parametrize("n,name", [(64, name) for name in P.STREAM_NAMES] + [(16, "97")])
def test_pack_window_meets_every_pair_of_words(n, name):
    """The arrays test_pack_window_words runs: every edge word is a mask, a
    body, a key word and a word of prev, and every (mask word, key word) pair
    meets in a term -- at the moduli below 2^63 (16 words, the fast
    accumulator) as well as above."""
    in_dim, lv, bl, batch = I.PACK_WINDOW
    S = len(I.pack_window_slots(n))
    q = 97 if name == "97" else P.stream_primes(n)[name]
    W = P.stream_words(q)
    assert len(W) == 16 or q >> 63
    key, lwe_a, lwe_b, prev = I.pack_window(n, q, in_dim, lv, batch, S)
    assert key.shape == (in_dim * lv, 2, n) and lwe_a.shape == (batch, S, in_dim)
    assert lwe_b.shape == (batch, S) and prev.shape == (batch, 2, n)
    for arr in (key, lwe_a, lwe_b, prev):
        assert set(arr.reshape(-1).tolist()) == set(W)
    for c in range(batch):  # in every ciphertext
        assert set(lwe_a[c].reshape(-1).tolist()) == set(W)
    pairs = set()
    for i in range(in_dim):  # entry e = i level + l multiplies a digit of mask word i with key[e]
        masks = set(lwe_a[:, :, i].reshape(-1).tolist())
        keys = set(key[i * lv:(i + 1) * lv].reshape(-1).tolist())
        pairs |= {(a, k) for a in masks for k in keys}
    assert len(pairs) == len(W) ** 2
    top = (1 << bl) - 1
    digs = {d for w in W for d in pack_ref.digits(w, bl, lv)}
    assert {0, top} <= digs


# ---------------------------------------------------------------- Galois
@pytest.mark.parametrize("n,name", [(16, "lazy_top"), (16, "u64_top"), (1024, "wrap")])
def test_galois_operands_cover_the_rows(n, name):
    q = P.sweep_primes(n)[name]
    rows = I.Rows(n, q)
    lv = 3 if q < 1 << 30 else 4
    bl = -(-q.bit_length() // lv)
    seen = [set(), set()]
    digit_values = set()
    for shift in (0, 1):
        ct = I.galois_operands(rows, shift)
        assert ct.shape == (len(rows.names), 2, n)
        for i, pair in enumerate(I.operand_rows(rows, shift)):
            for comp in range(2):
                assert (ct[i, comp] == rows.base[rows.names.index(pair[comp])]).all()
                seen[comp].add(pair[comp])
        ct = np.concatenate([ct, I.galois_digit_edges(n, q, bl)])  # as the GPU sweeps append them
        for g in (3, 2 * n - 1):
            s1 = galois_ref.sigma(ct[:, 1], g, q)
            for l in range(lv):
                digit_values |= set(((s1 >> np.uint64(l * bl)) & np.uint64((1 << bl) - 1)).reshape(-1).tolist())
    assert seen[0] == seen[1] == set(rows.names)
    assert 0 in digit_values and (1 << bl) - 1 in digit_values


def test_plant_words_puts_every_word_at_both_parities():
    q = P.stream_primes(256)["u64_max"]
    rows = I.Rows(256, q)
    ct = I.plant_words(I.galois_operands(rows, 0), P.stream_words(q))
    for comp in range(2):
        for w in P.stream_words(q):
            at = np.nonzero(ct[-1, comp] == np.uint64(w))[0]
            assert (at % 2 == 0).any() and (at % 2 == 1).any(), (comp, w)
