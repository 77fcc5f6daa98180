"""The scale-invariant BFV product at its exactness bounds and at the modulus
edges (bfv_scale.hip, the host orchestration of fhe_ct_multiply_scaled_batch /
fhe_ct_dot_scaled_batch / fhe_ct_square_scaled_batch), word for word against
the exact-integer model tests/bfv_ref.py.

test_gpu_scaled.py runs random ciphertexts, whose |t X / q| stays orders of
magnitude below the bounds.  Here the operands are the designed pairs of
tests/range_inputs.py, whose tensor reaches 2 n ((q-1)/2)^2, at the plaintext
moduli on either side of the per-call one-prime decision (t count n q < p1)
and at the largest exact t and count (t count n q < p1 p2); the moduli are the
primes at the lazy, word-size, 2^62 and 2^63 thresholds; the operands of the
main channel fill the unreduced input window; and q equal to the second and
third auxiliary prime changes which two serve as (p1, p2).
tests/test_range_inputs.py asserts on the CPU that the bounds are reached.

Run on an MI355X with ``pytest -m gpu``."""
import numpy as np
import pytest

import bfv_ref as R
import range_inputs as I
from test_gpu_scaled import raw_words

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def D(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def H(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def U(rows):
    return np.array(rows, dtype=np.uint64)


def bad(got, want, names):
    rows = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
    return [names[i % len(names)] for i in rows]


def ring_of(fg, n, q):
    return fg.PolynomialRing(n, q, mode="negacyclic")


def multiplier(fg, r, t):
    sm = fg.ScaledMultiplier(r, t)
    assert sm.aux == R.aux_for(r.get_modulus()) and sm.t == t
    return sm


BOUND_SHAPES = I.BOUND_SHAPES


# ---- multiply and square of the pairs that reach the bound ----------------------
@pytest.mark.parametrize("n,name", BOUND_SHAPES)
def test_multiply_at_the_bound(fg, n, name):
    q = I.scaled_prime(n, name)
    r = ring_of(fg, n, q)
    pairs = I.bound_ciphertexts(n, q)
    names = list(pairs)
    x = np.stack([pairs[k][0] for k in names])
    y = np.stack([pairs[k][1] for k in names])
    X = [R.tensor(a.tolist(), b.tolist(), q) for a, b in zip(x, y)]      # t-independent: once per shape
    Xsq = [R.tensor(a.tolist(), a.tolist(), q) for a in x]
    h = (q - 1) // 2
    assert max(X[0][1]) == max(Xsq[0][1]) == 2 * n * h * h
    # d = ct - ref is all -h both ways: (q+1)/2 - 0 and 0 - (q-1)/2
    sd_ct = np.stack([np.full((2, n), (q + 1) // 2, dtype=np.uint64), np.zeros((2, n), dtype=np.uint64)])
    sd_ref = np.stack([np.zeros((2, n), dtype=np.uint64), np.full((2, n), h, dtype=np.uint64)])
    dx, dy = D(x), D(y)
    cases = [c for c in I.scaled_bound_cases(n, q) if c[1] == 1]
    assert cases
    for i, (t, _, one) in enumerate(cases):
        assert one == I.one_prime(n, q, t, 1)
        sm = multiplier(fg, r, t)
        want = U([R.scale_rows(Xi, q, t) for Xi in X])
        assert want.tolist() == [R.multiply_scaled(x[0].tolist(), y[0].tolist(), q, t)] + want[1:].tolist()
        got = H(sm.multiply(dx, dy))
        assert (got == want).all(), ("multiply", n, name, t, one, bad(got, want, names))
        want_sq = U([R.scale_rows(Xi, q, t) for Xi in Xsq])
        got = H(sm.square(dx))
        assert (got == want_sq).all(), ("square", n, name, t, one, bad(got, want_sq, names))
        want_sd = np.stack([want_sq[names.index("all +h")]] * 2)
        got = H(sm.squared_difference(D(sd_ct), D(sd_ref)))
        assert (got == want_sd).all(), ("squared_difference", n, name, t, one, bad(got, want_sd, ["ct -h", "ref +h"]))
        if i == 0:  # host residence, once per shape
            assert (sm.multiply(x, y) == want).all(), ("multiply on the host", n, name, t)
            assert (sm.squared_difference(sd_ct, sd_ref) == want_sd).all(), ("squared_difference on the host", n, name, t)
        sm.close()
    assert (H(dx) == x).all() and (H(dy) == y).all()


@pytest.mark.parametrize("n,name", BOUND_SHAPES)
def test_scale_round_at_the_bound(fg, n, name):
    """The stand-alone rounding step at the largest exact t of every modulus of
    the sweep: rnd(t X) = +-(p1 p2 - 1) / 2 exactly, which no tensor reaches
    (test_range_inputs.py), and the values on either side."""
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    t = R.max_t(n, q, p1, p2)
    sm = multiplier(fg, ring_of(fg, n, q), t)
    xs = R.edge_values(q, t, p1, p2, count=24)
    bound = (p1 * p2 - 1) // 2
    assert {bound, -bound} <= {R.rnd(t * v, q) for v in xs}
    rows = -(-len(xs) // n)
    xs = (xs * (rows * n // len(xs) + 1))[:rows * n]
    xq, x1, x2 = (U([v % m for v in xs]).reshape(rows, n) for m in (q, p1, p2))
    want = U([R.rnd(t * v, q) % q for v in xs]).reshape(rows, n)
    got = H(sm.scale_round(D(xq), D(x1), D(x2)))
    assert (got == want).all(), (n, name, np.argwhere(got != want)[:4].tolist())
    sm.close()


# ---- the dot product on either side of the one-prime decision -------------------
@pytest.mark.parametrize("name", ["lazy_top", "u64_bottom"])
def test_dot_across_the_one_prime_threshold(fg, monkeypatch, name):
    n = 1024
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    t7 = min(q - 1, (p1 - 1) // (n * q)) // 7
    cases = {c[1]: c[2] for c in I.scaled_bound_cases(n, q) if c[0] == t7}
    assert cases == {7: True, 8: False}
    plus, _ = I.bound_ciphertexts(n, q)["all +h"]
    minus, _ = I.bound_ciphertexts(n, q)["negated all +h"]
    sm = multiplier(fg, ring_of(fg, n, q), t7)
    for count in (7, 8):
        a = np.broadcast_to(plus, (2, count, 2, n)).copy()
        b = a.copy()
        a[1, count // 2] = minus  # the second group: one pair negated, the sum below the peak
        want = U([R.dot_scaled(g.tolist(), k.tolist(), q, t7) for g, k in zip(a, b)])
        assert (want[0] != want[1]).any()
        for chunk in (None, "3"):  # 3: a group goes through several steps that accumulate at the bound
            if chunk is None:
                monkeypatch.delenv("FHE_SCALE_CHUNK", raising=False)
            else:
                monkeypatch.setenv("FHE_SCALE_CHUNK", chunk)
            got = H(sm.dot(D(a), D(b)))
            assert (got == want).all(), (name, count, chunk, bad(got, want, ["all +h", "one pair negated"]))
            got = sm.dot(a, b)
            assert (got == want).all(), (name, count, chunk, "host", bad(got, want, ["all +h", "one pair negated"]))
    sm.close()


@pytest.mark.parametrize("name", ["u64_top", "u64_max"])
def test_dot_at_max_count(fg, name):
    n = 1024
    q = I.scaled_prime(n, name)
    p1, p2 = R.aux_for(q)
    t = R.max_t(n, q, p1, p2) // 3
    count = R.max_count(n, q, t, p1, p2)
    assert 3 <= count <= 6 and (t, count, False) in I.scaled_bound_cases(n, q)
    sm = multiplier(fg, ring_of(fg, n, q), t)
    assert sm.max_count == count
    plus, _ = I.bound_ciphertexts(n, q)["all +h"]
    a = np.broadcast_to(plus, (count, 2, n)).copy()
    want = U(R.dot_scaled(a.tolist(), a.tolist(), q, t))
    got = H(sm.dot(D(a), D(a)))
    assert (got == want).all(), (name, t, count, "all +h")
    over = np.broadcast_to(plus, (count + 1, 2, n)).copy()
    out = D(np.full((3, n), 7, dtype=np.uint64))
    with pytest.raises(fg.FHEError) as e:
        sm.dot(D(over), D(over), out=out)
    assert e.value.code == -10 and "largest exact count %d" % count in str(e.value)
    assert (H(out) == 7).all()  # nothing ran
    sm.close()


# ---- the main channel at the modulus edges, operands at the top of the window ---
@pytest.mark.parametrize("name", I.SCALED_NAMES)
@pytest.mark.parametrize("n", [16, 1024])
def test_multiply_window_rows(fg, n, name):
    q = I.scaled_prime(n, name)
    r = ring_of(fg, n, q)
    names, x, y = I.window_pairs(n, q)
    X = [R.tensor(a.tolist(), b.tolist(), q) for a, b in zip(x, y)]
    dx, dy = D(x), D(y)
    sm = None
    for t in [t for t in (2, 65537) if t < q]:
        sm = multiplier(fg, r, t)
        want = U([R.scale_rows(Xi, q, t) for Xi in X])
        if n == 16:
            assert want.tolist() == [R.multiply_scaled(a.tolist(), b.tolist(), q, t) for a, b in zip(x, y)]
        got = H(sm.multiply(dx, dy))
        assert (got == want).all(), ("multiply", n, name, t, bad(got, want, [names[2 * i % len(names)] for i in range(len(names))]))
    # the centred lift of the same rows
    p1, p2 = sm.aux
    rows = x.reshape(-1, n)
    lifted = [R.lift(v, q) for v in rows.reshape(-1).tolist()]
    want1, want2 = (U([v % p for v in lifted]).reshape(rows.shape) for p in (p1, p2))
    o1, o2 = sm.center_lift(D(rows))
    assert (H(o1) == want1).all(), ("lift mod p1", n, name, bad(H(o1), want1, names))
    assert (H(o2) == want2).all(), ("lift mod p2", n, name, bad(H(o2), want2, names))
    sm.close()


# ---- q equal to an auxiliary prime ---------------------------------------------
@pytest.mark.parametrize("which", [1, 2])
def test_modulus_equal_to_an_auxiliary_prime(fg, which):
    n, t = 256, 65537
    q = R.AUX_PRIMES[which]
    sm = multiplier(fg, ring_of(fg, n, q), t)
    assert sm.aux == R.aux_for(q) == tuple(p for p in R.AUX_PRIMES if p != q) and q not in sm.aux
    plus, _ = I.bound_ciphertexts(n, q)["all +h"]
    x = np.concatenate([raw_words([n, 21], q, (2, 2, n)), plus[None]])
    y = np.concatenate([raw_words([n, 22], q, (2, 2, n)), plus[None]])
    want = U([R.multiply_scaled(a.tolist(), b.tolist(), q, t) for a, b in zip(x, y)])
    got = H(sm.multiply(D(x), D(y)))
    assert (got == want).all(), (q, bad(got, want, ["raw words", "raw words", "all +h"]))
    assert (sm.multiply(x, y) == want).all(), (q, "host")
    sm.close()
