"""GPU parity of the streaming kernels at the edges of their word arithmetic
(csrc/tally.hip k_ct_sum / k_ct_sum_scaled / k_scalar_prep, threshold.hip
k_combine_partials / k_shamir_shares, elementwise.hip add / subtract / negate
/ multiply_scalar, and the host's scalar_entry).  They take any degree and any
odd modulus, and switch arithmetic at q = 2^63: the Shoup product
x s - hi(x s') q (up to 2q ~ 2^64 just below) and a Barrett reduction below,
the Montgomery product and one conditional subtraction, with carries out of
the word, above.  So: n = 16 (and 4, one 16-byte column per polynomial pair),
the primes on either side of 2^30, 2^62, 2^63 and at the top of the word
(ntt_primes.stream_primes), 97 and 2^64 - 2^32 + 1, and the full cross
product of the words and scalars at the edges of those ranges
(ntt_primes.stream_words / stream_scalars / cross_ballots).

Expected values are Python integers, sum((x % q) (s % q) % q) % q; the
decoded values and the noise of the combination come from the CPU oracle's
decrypt (the reference's int64 noise distance, which wraps at q >= 2^63).
Every check runs on host arrays and on device tensors: device scalars are
prepared by k_scalar_prep, host arrays and pointer tables by scalar_entry, two
implementations of one table.  Bit-exact.

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import ntt_primes as P
from test_gpu_threshold import oracle_decode

pytestmark = pytest.mark.gpu

N = 16
MODULI = list(P.STREAM_NAMES) + [97, P.QG]
moduli = pytest.mark.parametrize("name", MODULI)
splits = pytest.mark.parametrize("split", [None, "2"])


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def modulus(n, name):
    return name if isinstance(name, int) else P.stream_primes(n)[name]


def D(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def H(t):
    import torch

    if isinstance(t, np.ndarray):
        return t
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def off_by_8(a):
    """The words of `a` in a device view that starts 8 bytes past a 16-byte
    boundary: a flat tensor sliced [1:] and reshaped."""
    import torch

    a = np.ascontiguousarray(a)
    flat = torch.zeros(a.size + 1, dtype=torch.int64, device="cuda:0")
    flat[1:] = torch.from_numpy(a.reshape(-1).view(np.int64))
    view = flat[1:].reshape(a.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view


def set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_TALLY_SPLIT", split)


def u64(ints, shape=None):
    a = np.array([int(v) for v in ints], dtype=np.uint64)
    return a if shape is None else a.reshape(shape)


def word_rows(q, rows, n, roll=0):
    """[rows, n] of stream_words(q): row r is the list rolled by r + roll."""
    W = P.stream_words(q)
    return u64([W[(j + r + roll) % len(W)] for r in range(rows) for j in range(n)], (rows, n))


def scaled_sum(q, a, s=None, prior=None):
    """sum_i (a[i] % q) (s[i] % q) % q (+ prior % q), mod q, per column, in
    Python integers; s = None: every scalar 1."""
    count = a.shape[0]
    flat = a.reshape(count, -1)
    sc = [1] * count if s is None else [int(v) % q for v in s]
    pr = [0] * flat.shape[1] if prior is None else [int(v) % q for v in prior.reshape(-1)]
    out = [(sum((int(flat[i, j]) % q) * sc[i] % q for i in range(count)) + pr[j]) % q for j in range(flat.shape[1])]
    return u64(out, a.shape[1:])


# ---------------------------------------------------------------- elementwise
@moduli
def test_elementwise_cross_product(fg, name):
    """add, subtract, negate over stream_words x stream_words and
    multiply_scalar over stream_words x stream_scalars."""
    q = modulus(N, name)
    ring = fg.PolynomialRing(N, q)
    W, S = P.stream_words(q), P.stream_scalars(q)
    pairs = [(a, b) for a in W for b in W]
    pairs += pairs[:-len(pairs) % N]  # whole rows
    a = u64([p[0] for p in pairs], (-1, N))
    b = u64([p[1] for p in pairs], (-1, N))
    add = u64([(x % q + y % q) % q for x, y in pairs], a.shape)
    sub = u64([(x % q - y % q) % q for x, y in pairs], a.shape)
    # negate does not reduce: the reference's rule is x == 0 ? 0 : q - x on the raw word, in
    # u64 arithmetic (PolynomialRing::negate; tests/test_gpu_parity.py holds the library to it)
    neg = u64([0 if x == 0 else (q - x) % (1 << 64) for x, _ in pairs], a.shape)
    assert all(int(v) == -x % q for v, (x, _) in zip(neg.reshape(-1), pairs) if x < q)
    assert add.any() and sub.any() and neg.any()
    for put in (D, np.ascontiguousarray):
        x, y = put(a), put(b)
        assert (H(ring.add(x, y)) == add).all(), put.__name__
        assert (H(ring.subtract(x, y)) == sub).all(), put.__name__
        assert (H(ring.negate(x)) == neg).all(), put.__name__
    w = word_rows(q, 1, N)
    assert set(int(v) for v in w[0]) == set(W)
    for s in S:
        exp = u64([(int(v) % q) * (s % q) % q for v in w[0]], w.shape)
        assert exp.any() == (s % q != 0)
        for put in (D, np.ascontiguousarray):
            assert (H(ring.multiply_scalar(put(w), s)) == exp).all(), (s, put.__name__)


# ---------------------------------------------------------------- sums
def pick(full, count, seed):
    """`count` of the `full` ballots of cross_ballots, seeded (all of them for None)."""
    if count is None:
        return np.arange(full)
    return np.sort(np.random.default_rng([full, count, seed]).permutation(full)[:count])


def check_sums(fg, monkeypatch, n, q, split, scaled):
    ring = fg.PolynomialRing(n, q)
    set_split(monkeypatch, split)
    for polys in (1, 2, 3):
        a, s = P.cross_ballots(q, n, polys)
        full = a.shape[0]
        prior = word_rows(q, polys, n, roll=3)
        for count in P.STREAM_COUNTS:
            sel = pick(full, count, polys)
            sub, sc = np.ascontiguousarray(a[sel]), (np.ascontiguousarray(s[sel]) if scaled else None)
            exp, exp_acc = scaled_sum(q, sub, sc), scaled_sum(q, sub, sc, prior)
            if sel.size > 2:
                assert exp.any()
            assert exp_acc.any()  # one or two ballots may sum to zero (a scalar 0): the prior row does not
            where = (polys, count)
            dsub = D(sub)
            bufs = [dsub[i] for i in range(sel.size)]
            dout, hout, pout = D(prior.copy()), prior.copy(), D(prior.copy())
            if scaled:
                ints = [int(v) for v in sc]
                assert (H(ring.sum_scaled(dsub, D(sc))) == exp).all(), where          # k_scalar_prep
                assert (ring.sum_scaled(sub, sc) == exp).all(), where                 # host scalar_entry
                assert (H(ring.sum_scaled_buffers(bufs, ints)) == exp).all(), where   # host scalar_entry
                ring.sum_scaled(dsub, D(sc), out=dout, accumulate=True)
                ring.sum_scaled(sub, sc, out=hout, accumulate=True)
                ring.sum_scaled_buffers(bufs, ints, out=pout, accumulate=True)
            else:
                assert (H(ring.sum_batch(dsub)) == exp).all(), where
                assert (ring.sum_batch(sub) == exp).all(), where
                assert (H(ring.sum_buffers(bufs)) == exp).all(), where
                ring.sum_batch(dsub, out=dout, accumulate=True)
                ring.sum_batch(sub, out=hout, accumulate=True)
                ring.sum_buffers(bufs, out=pout, accumulate=True)
            assert (H(dout) == exp_acc).all(), where
            assert (hout == exp_acc).all(), where
            assert (H(pout) == exp_acc).all(), where


def check_all_ones(fg, monkeypatch, n, q, split):
    """HIGH_WORD_COUNT terms of 2^64 - 1: the 128-bit accumulator's high word
    is 98 (>= q at q = 97, so fold128 reduces it as well)."""
    ring = fg.PolynomialRing(n, q)
    set_split(monkeypatch, split)
    count = P.HIGH_WORD_COUNT
    a = np.full((count, 2, n), P.M64, dtype=np.uint64)
    exp = np.full((2, n), count * (P.M64 % q) % q, dtype=np.uint64)
    assert (count * P.M64) >> 64 == 98 and exp.any()
    da = D(a)
    assert (H(ring.sum_batch(da)) == exp).all()
    assert (ring.sum_batch(a) == exp).all()
    assert (H(ring.sum_buffers([da[i] for i in range(count)])) == exp).all()
    ones = np.ones(count, dtype=np.uint64)
    assert (H(ring.sum_scaled(da, D(ones))) == exp).all()
    assert (ring.sum_scaled(a, ones) == exp).all()


@moduli
@splits
def test_sum_cross_ballots(fg, monkeypatch, name, split):
    q = modulus(N, name)
    check_sums(fg, monkeypatch, N, q, split, scaled=False)
    check_all_ones(fg, monkeypatch, N, q, split)


@moduli
@splits
def test_sum_scaled_cross_ballots(fg, monkeypatch, name, split):
    check_sums(fg, monkeypatch, N, modulus(N, name), split, scaled=True)


@pytest.mark.parametrize("name", ["shoup_top", "wmont_bottom"])
@pytest.mark.parametrize("scaled", [False, True])
def test_sums_at_the_smallest_degree(fg, monkeypatch, name, scaled):
    """n = 4, one polynomial: a ballot is two 16-byte columns."""
    check_sums(fg, monkeypatch, 4, modulus(4, name), None, scaled)


# ---------------------------------------------------------------- Shamir shares
@moduli
def test_shamir_shares_of_edge_words(fg, name):
    """(2, 8), (5, 9), (3, 17): one full tile of kShTile = 8 points, one past
    it, and two tiles and one."""
    q = modulus(N, name)
    ring = fg.PolynomialRing(N, q)
    for threshold, total in ((1, 1), (2, 8), (5, 9), (3, 17)):
        coeffs = word_rows(q, threshold, N, roll=threshold)
        exp = u64([sum((int(coeffs[k, j]) % q) * pow(i, k, q) % q for k in range(threshold)) % q
                   for i in range(1, total + 1) for j in range(N)], (total, N))
        assert exp.any(axis=1).all()
        assert (H(fg.shamir_shares(ring, D(coeffs), total)) == exp).all(), (threshold, total)
        assert (fg.shamir_shares(ring, coeffs, total) == exp).all(), (threshold, total)


# ---------------------------------------------------------------- combination
@moduli
def test_combine_partials_cross_product(fg, name):
    """Partials x lambdas as the cross product (every partial block holds all
    of stream_words, the lambdas walk through stream_scalars), c0 from
    stream_words; count 4 and 5 around the unroll, 16 and 17 around the inline
    table.  The same call on views 8 bytes off 16-byte alignment takes the
    one-word-per-lane kernels."""
    q = modulus(N, name)
    ring = fg.PolynomialRing(N, q)
    W, S = P.stream_words(q), P.stream_scalars(q)
    b, seen, k = 3, set(), 0
    ct = np.stack([word_rows(q, b, N, roll=5), np.full((b, N), P.M64, dtype=np.uint64)], axis=1)  # c1 is never read
    for count in (1, 4, 5, 16, 17):
        par = np.stack([word_rows(q, b, N, roll=i) for i in range(count)])
        for t in (0, 16, 1 << 40):
            lams = [S[(k + i) % len(S)] for i in range(count)]
            k += count
            seen |= {(int(w), lam) for i, lam in enumerate(lams) for w in par[i, 0]}
            acc = scaled_sum(q, par.reshape(count, -1), lams).reshape(b, N)
            phase = u64([(int(c) % q - int(v)) % q for c, v in zip(ct[:, 0].reshape(-1), acc.reshape(-1))], (b, N))
            assert phase.any(axis=1).all()
            vals, mx = oracle_decode(N, q, t, phase)
            eng = fg.EncryptionEngine(ring, t)
            for kind, put in (("device", D), ("host", np.ascontiguousarray), ("off by 8", off_by_8)):
                res = eng.combine_partials(put(ct), put(par), lams, with_phase=True)
                where = (count, t, kind)
                assert (H(res.phase) == phase).all(), where
                assert (H(res.values) == vals).all(), where
                assert (res.max_noise == mx).all(), (where, res.max_noise, mx)
    assert seen == {(w, lam) for w in W for lam in S}
