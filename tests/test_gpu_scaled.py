"""The scale-invariant BFV product on the GPU (fhe_scale_ctx, the two kernels
of bfv_scale.hip and fhe_ct_multiply_scaled_batch / fhe_ct_dot_scaled_batch /
fhe_ct_square_scaled_batch) against the exact-integer model tests/bfv_ref.py:

- the centred lift and the scale-and-round step, word for word, at the
  modulus edges and with the reference subtracted while loading;
- the whole multiply against schoolbook and Kronecker products;
- the identities between the three entry points, chunking and residence;
- the errors that need a context;
- the meaning with the library's own keys: multiply_scaled -> relinearize ->
  decrypt gives the product of the plaintexts, a weighted tally under encrypted
  weights gives sum w_i b_i, each with its noise below q / (2 t) / 4;
- the JS engine (tests/js/scaled_test.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bfv_ref as R
from ntt_primes import stream_words

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
QG = 18446744069414584321     # 2^64 - 2^32 + 1
M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD_SHAPES = [(4, 97), (1024, P27), (1024, P62), (256, QG), (32768, P27)]


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


_RINGS = {}


def scaled(fg, n, q, t):
    """One ring per (n, q) and one scale context per (n, q, t) for the module."""
    if (n, q) not in _RINGS:
        _RINGS[(n, q)] = (fg.PolynomialRing(n, q, mode="negacyclic"), {})
    r, by_t = _RINGS[(n, q)]
    if t not in by_t:
        by_t[t] = fg.ScaledMultiplier(r, t)
    return r, by_t[t]


def raw_words(seed, q, shape):
    """Full-range u64 words with the residues at both ends of the centred
    range planted."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = U([0, q - 1, q, M64, (q - 1) // 2, (q + 1) // 2])
    k = min(len(edge), shape[-1])
    a[..., :k] = edge[:k]
    return a


def lift_inputs(n, q, rows):
    """stream_words(q), (q -+ 1) / 2 and their unreduced copies, then random raw words: [rows, n]."""
    words = stream_words(q) + [(q - 1) // 2, (q + 1) // 2]
    words += [w + q for w in ((q - 1) // 2, (q + 1) // 2) if w + q <= M64]
    a = np.random.default_rng([n, q % (1 << 32), 11]).integers(0, 1 << 64, size=rows * n, dtype=np.uint64)
    assert rows * n >= len(words), "every edge word is in the input"
    a[:len(words)] = U(words)
    return a.reshape(rows, n)


# ---- 1. lift -------------------------------------------------------------------
@pytest.mark.parametrize("n,q", WORD_SHAPES)
def test_lift_words(fg, n, q):
    rows = 8 if n == 4 else 1 if n == 32768 else 4
    r, sm = scaled(fg, n, q, 2)
    p1, p2 = sm.aux
    assert (p1, p2) == R.aux_for(q)
    x = lift_inputs(n, q, rows)
    lifted = [R.lift(v, q) for v in x.reshape(-1).tolist()]
    want1, want2 = U([v % p1 for v in lifted]).reshape(x.shape), U([v % p2 for v in lifted]).reshape(x.shape)
    o1, o2 = sm.center_lift(D(x))
    assert (H(o1) == want1).all() and (H(o2) == want2).all()
    h1, h2 = sm.center_lift(x)
    assert (h1 == want1).all() and (h2 == want2).all()
    if rows == 1:
        return
    # the reference subtracted while loading: one ciphertext for all, and one per ciphertext
    ct = x.reshape(rows // 2, 2, n)
    for ref in (ct[-1][::-1].copy(), np.ascontiguousarray(np.roll(ct, 1, axis=0)[:, ::-1])):
        full = np.broadcast_to(ref, ct.shape)
        d = [R.lift(a % q - b % q, q) for a, b in zip(ct.reshape(-1).tolist(), full.reshape(-1).tolist())]
        o1, o2 = sm.center_lift(D(ct), D(ref))
        assert (H(o1).reshape(-1) == U([v % p1 for v in d])).all(), ref.shape
        assert (H(o2).reshape(-1) == U([v % p2 for v in d])).all(), ref.shape


# ---- 2. scale and round --------------------------------------------------------
def t_values(n, q):
    p1, p2 = R.aux_for(q)
    ts = [t for t in (2, 4, 65537) if t < q]
    return ts + [R.max_t(n, q, p1, p2)]


@pytest.mark.parametrize("n,q,t", [(n, q, t) for n, q in WORD_SHAPES for t in t_values(n, q)])
def test_scale_round_words(fg, n, q, t):
    r, sm = scaled(fg, n, q, t)
    p1, p2 = sm.aux
    assert sm.max_count == min(R.max_count(n, q, t, p1, p2), M64) >= 1  # the field is a u64
    rows = 16 if n == 4 else 1
    xs = R.edge_values(q, t, p1, p2, count=max(24, rows * n - 24))
    xs = (xs * (rows * n // len(xs) + 1))[:rows * n]
    shape = (rows, n)
    xq, x1, x2 = (U([x % m for x in xs]).reshape(shape) for m in (q, p1, p2))
    want = U([R.rnd(t * x, q) % q for x in xs]).reshape(shape)
    got = H(sm.scale_round(D(xq), D(x1), D(x2)))
    assert (got == want).all(), np.argwhere(got != want)[:4]
    if n <= 1024:
        assert (sm.scale_round(xq, x1, x2) == want).all()


# ---- 3. the whole multiply -----------------------------------------------------
def model_multiply(x, y, q, t):
    return U([R.multiply_scaled(a.tolist(), b.tolist(), q, t) for a, b in zip(x, y)])


@pytest.mark.parametrize("q,t", [(P27, 4), (P62, 65537), (QG, 257)])
@pytest.mark.parametrize("n", [4, 16, 64])
def test_multiply_against_schoolbook(fg, n, q, t):
    r, sm = scaled(fg, n, q, t)
    x, y = raw_words([n, 1], q, (3, 2, n)), raw_words([n, 2], q, (3, 2, n))
    want = model_multiply(x, y, q, t)
    assert (H(sm.multiply(D(x), D(y))) == want).all()
    assert (sm.multiply(x, y) == want).all()


@pytest.mark.parametrize("n,q,t,batch", [(1024, P27, 4, 2), (1024, P27, P27 - 1, 2), (4096, P62, 65537, 1),
                                         (16384, P27, 4, 3), (32768, P27, 2, 1)])
def test_multiply_against_kronecker(fg, n, q, t, batch):
    """(1024, 27-bit) runs both forms: t = 4 leaves t n q below the first
    auxiliary prime (its channel alone runs), t = q - 1 does not."""
    r, sm = scaled(fg, n, q, t)
    assert (t * n * q < sm.aux[0]) == (q == P27 and t <= 4)
    x, y = raw_words([n, 3], q, (batch, 2, n)), raw_words([n, 4], q, (batch, 2, n))
    assert (H(sm.multiply(D(x), D(y))) == model_multiply(x, y, q, t)).all()


# ---- 4. identities -------------------------------------------------------------
IDENT = [(64, P27, 4), (256, P62, 65537), (64, QG, 257)]


@pytest.mark.parametrize("n,q,t", IDENT)
def test_dot_and_square_identities(fg, n, q, t):
    r, sm = scaled(fg, n, q, t)
    b = 3
    x, y = raw_words([n, 5], q, (b, 2, n)), raw_words([n, 6], q, (b, 2, n))
    mul = H(sm.multiply(D(x), D(y)))
    # count 1 in b groups is the multiply
    assert (H(sm.dot(D(x.reshape(b, 1, 2, n)), D(y.reshape(b, 1, 2, n)))) == mul).all()
    # square(ct - ref) is multiply(d, d)
    for ref in (y[0], y):
        d = r.subtract(x, np.ascontiguousarray(np.broadcast_to(ref, x.shape)))
        want = H(sm.multiply(D(d), D(d)))
        assert (H(sm.squared_difference(D(x), D(ref))) == want).all(), ref.shape
        assert (sm.squared_difference(x, ref) == want).all(), ref.shape
    assert (H(sm.square(D(x))) == H(sm.multiply(D(x), D(x)))).all()
    # count 7 against the model, in two groups
    a7, b7 = raw_words([n, 7], q, (2, 7, 2, n)), raw_words([n, 8], q, (2, 7, 2, n))
    want = U([R.dot_scaled(g.tolist(), h.tolist(), q, t) for g, h in zip(a7, b7)])
    assert (H(sm.dot(D(a7), D(b7))) == want).all()
    assert (sm.dot(a7, b7) == want).all()  # host residence


def test_dot_rescales_once_and_differs_from_a_sum_of_multiplies(fg):
    """Rounding is not linear: the dot product carries one rounding error, a
    sum of seven scaled multiplies seven.  The words differ; do not 'fix' it."""
    n, q, t = 64, P27, 4
    r, sm = scaled(fg, n, q, t)
    a, b = raw_words([n, 9], q, (7, 2, n)), raw_words([n, 10], q, (7, 2, n))
    dot = H(sm.dot(D(a), D(b)))
    summed = sm.multiply(a, b).astype(object).sum(axis=0) % q
    assert summed.shape == dot.shape
    diff = (summed - dot.astype(object)) % q
    diff = np.minimum(diff, q - diff)
    assert (summed != dot).any()
    assert diff.max() <= 4  # seven roundings of at most 1/2 each against one


@pytest.mark.parametrize("n,q,t", IDENT)
def test_chunks_and_residence_give_the_same_words(fg, n, q, t, monkeypatch):
    r, sm = scaled(fg, n, q, t)
    x, y = raw_words([n, 11], q, (5, 2, n)), raw_words([n, 12], q, (5, 2, n))
    whole = {"mul": H(sm.multiply(D(x), D(y))), "dot": H(sm.dot(D(x), D(y))),
             "dot2": H(sm.dot(D(x[:4].reshape(2, 2, 2, n)), D(y[:4].reshape(2, 2, 2, n)))),
             "sq": H(sm.squared_difference(D(x), D(y)))}
    monkeypatch.setenv("FHE_SCALE_CHUNK", "2")
    for device in (True, False):
        w = D if device else (lambda a: a)
        back = H if device else (lambda a: a)
        got = {"mul": back(sm.multiply(w(x), w(y))), "dot": back(sm.dot(w(x), w(y))),
               "dot2": back(sm.dot(w(x[:4].reshape(2, 2, 2, n)), w(y[:4].reshape(2, 2, 2, n)))),
               "sq": back(sm.squared_difference(w(x), w(y)))}
        for k, v in got.items():
            assert (v == whole[k]).all(), (k, device)
    monkeypatch.setenv("FHE_SCALE_CHUNK", "1")
    assert (H(sm.dot(D(x[:4].reshape(2, 2, 2, n)), D(y[:4].reshape(2, 2, 2, n)))) == whole["dot2"]).all()


# ---- 5. errors -----------------------------------------------------------------
def test_errors_that_need_a_context(fg):
    import torch

    n, q = 64, P27
    with pytest.raises(fg.FHEError) as e:
        fg.ScaledMultiplier(fg.PolynomialRing(n, q, mode="compat"), 4)
    assert e.value.code == -10 and "FHE_MODE_NEGACYCLIC" in str(e.value)
    if torch.cuda.device_count() >= 1:
        with pytest.raises(fg.FHEError) as e:
            fg.ScaledMultiplier(fg.PolynomialRing(n, q, mode="negacyclic", devices=[0, 0]), 4)
        assert e.value.code == -10 and "single-device" in str(e.value)
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    for t in (1, q, q + 1, M64):
        with pytest.raises(fg.FHEError) as e:
            fg.ScaledMultiplier(r, t)
        assert e.value.code == -9 and "2 <= t < q" in str(e.value), t
    assert fg.ScaledMultiplier(r, 0).t == 4
    # a count above max_count: the largest t leaves room for one pair only
    rg = fg.PolynomialRing(256, QG, mode="negacyclic")
    p1, p2 = R.aux_for(QG)
    sm = fg.ScaledMultiplier(rg, R.max_t(256, QG, p1, p2))
    assert sm.max_count == 1
    z = np.zeros((2, 2, 256), np.uint64)
    with pytest.raises(fg.FHEError) as e:
        sm.dot(z, z)
    assert e.value.code == -10 and "largest exact count 1" in str(e.value)
    with pytest.raises(fg.FHEError) as e:
        fg.ScaledMultiplier(rg, R.max_t(256, QG, p1, p2) + 1)
    assert e.value.code == -10 and "largest count is 0" in str(e.value)
    # an output that overlaps an input
    sm = fg.ScaledMultiplier(r, 4)
    buf = torch.zeros(5 * n, dtype=torch.int64, device="cuda:0")
    with pytest.raises(fg.FHEError) as e:
        sm.multiply(buf[:2 * n].reshape(1, 2, n), buf[2 * n:4 * n].reshape(1, 2, n), out=buf[2 * n:].reshape(1, 3, n))
    assert e.value.code == -9 and "overlap" in str(e.value)


# ---- 6. meaning ----------------------------------------------------------------
def keys(fg, r, bl, lv, seed):
    kg = fg.KeyGenerator(r, seed=seed)
    s = kg.secret_key(1)
    pk = fg.PublicKey(r, kg.public_key(s, 2))
    ek = fg.EvaluationKey(r, kg.eval_key(s, bl, lv, 10), bl)
    return s, fg.SecretKey(r, s), pk, ek


def dev_key(fg, r, s, bl, lv, seed):
    """The evaluation key of keys() on the device."""
    return fg.EvaluationKey(r, D(fg.KeyGenerator(r, seed=seed).eval_key(s, bl, lv, 10)), bl)


def check_noise(res, q, t, what):
    bound = q // (2 * t) // 4
    print(what, "max_noise", res.max_noise.tolist(), "q / (2 t) / 4 =", bound)
    assert (res.max_noise.astype(object) < bound).all()


@pytest.mark.parametrize("n,q,t,bl,lv", [(1024, P62, 65537, 16, 4), (256, P27, 4, 7, 4)])
def test_multiply_scaled_decrypts_to_the_product(fg, n, q, t, bl, lv):
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    s, sk, pk, ek = keys(fg, r, bl, lv, 20261021)
    rng = np.random.default_rng([n, t])
    m1, m2 = (rng.integers(0, t, size=(2, n), dtype=np.uint64) for _ in range(2))
    c1, c2 = eng.encrypt_sampled(m1, pk, 20261021, 100), eng.encrypt_sampled(m2, pk, 20261021, 200)
    assert (eng.decrypt(c1, sk).values == m1).all()
    want = U([R.plain_product(a.tolist(), b.tolist(), t) for a, b in zip(m1, m2)])
    res = eng.decrypt(eng.multiply_relin_scaled(c1, c2, ek), sk)
    assert (res.values == want).all()
    check_noise(res, q, t, "multiply n=%d" % n)
    res = eng.decrypt(H(eng.relinearize(eng.multiply_scaled(D(c1), D(c2)), dev_key(fg, r, s, bl, lv, 20261021))), sk)
    assert (res.values == want).all()
    # the unscaled tensor at the same parameters does not decrypt to it
    plain = eng.decrypt(eng.relinearize(eng.multiply(c1, c2), ek), sk)
    assert (plain.values != want).any()
    # squares: (m1 - m2)^2
    d = [[(int(a) - int(b)) % t for a, b in zip(x, y)] for x, y in zip(m1, m2)]
    res = eng.decrypt(eng.relinearize(eng.squared_difference_scaled(c1, c2), ek), sk)
    assert (res.values == U([R.plain_product(x, x, t) for x in d])).all()
    check_noise(res, q, t, "square n=%d" % n)


def test_weighted_tally_under_encrypted_weights(fg):
    """Seven ballots, weights encrypted as constants: sum_i w_i b_i mod t."""
    n, q, t, bl, lv = 256, P27, 4, 7, 4
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    s, sk, pk, ek = keys(fg, r, bl, lv, 7)
    rng = np.random.default_rng(7)
    ballots = rng.integers(0, 2, size=(7, n), dtype=np.uint64)
    weights = np.zeros((7, n), dtype=np.uint64)
    weights[:, 0] = rng.integers(1, t, size=7)
    cb, cw = eng.encrypt_sampled(ballots, pk, 7, 100), eng.encrypt_sampled(weights, pk, 7, 200)
    want = (ballots * weights[:, :1]).sum(axis=0) % t
    res = eng.decrypt(eng.tally_weighted_votes_scaled(cb, cw, ek), sk)
    assert (res.values == want).all()
    check_noise(res, q, t, "tally of 7")
    res = eng.decrypt(H(eng.tally_weighted_votes_scaled(list(D(cb)), list(D(cw)), dev_key(fg, r, s, bl, lv, 7))), sk)
    assert (res.values == want).all()
    # the reference's tally under the same keys does not open to it
    plain = eng.decrypt(eng.tally_weighted_votes(cb, cw, ek, relinearize="once"), sk)
    assert (plain.values != want).any()


# ---- 7. the JS engine ----------------------------------------------------------
def test_js_engine():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "scaled_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
