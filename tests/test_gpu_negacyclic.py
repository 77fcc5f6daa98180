"""GPU parity of negacyclic mode against references that share nothing with
the library: oracle/pyref.py's big-integer transforms (negacyclic_forward /
negacyclic_inverse) and its exact ring product by Kronecker substitution
(negacyclic_multiply).  The C oracle is compat-only, so above the golden
vectors (N <= 256) negacyclic results were so far compared with the
library's own kernels; a wrong but self-consistent stage table would pass
that.  Here every degree 4..16384 runs with the primes on either side of the
lazy threshold and at the top of the 64-bit lanes (tests/ntt_primes.py), fed
with the rows that fill the unreduced input windows, and the ciphertext
operations are checked against ring formulas written out in Python integers.

Bit-exact throughout.  Run on an MI355X with ``pytest -m gpu``.
"""
import hashlib

import numpy as np
import pytest

import ntt_primes as P
import oracle
from oracle import pyref

pytestmark = pytest.mark.gpu

P27 = 132120577
QG = P.QG
T = 16  # plaintext modulus of the engine tests


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def rnd(seed, q, *shape):
    return oracle.splitmix_fill(seed, q, int(np.prod(shape))).reshape(shape)


# ------------------------------------------------------------ references, computed once per distinct row
# pyref reads its inputs mod q, so rows with the same residues (0, q, 2q, ...)
# share one reference result.
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _CACHE.clear()


def _res(q, row):
    return np.ascontiguousarray(np.asarray(row, dtype=np.uint64) % np.uint64(q))


def _cached(kind, q, rows, fn):
    res = [_res(q, r) for r in rows]
    key = (kind, q) + tuple(hashlib.sha256(r.tobytes()).digest() for r in res)
    if key not in _CACHE:
        _CACHE[key] = np.array(fn(*[[int(v) for v in r] for r in res]), dtype=np.uint64)
    return _CACHE[key]


def ref_forward(q, row):
    return _cached("fwd", q, (row,), lambda a: pyref.negacyclic_forward(a, q))


def ref_inverse(q, row):
    return _cached("inv", q, (row,), lambda a: pyref.negacyclic_inverse(a, q))


def ref_mul(q, a, b):
    a, b = sorted((_res(q, a), _res(q, b)), key=lambda r: r.tobytes())  # the ring is commutative: one product per pair
    return _cached("mul", q, (a, b), lambda x, y: pyref.negacyclic_multiply(x, y, q))


def rows_of(fn, q, *operands):
    return np.stack([fn(q, *rows) for rows in zip(*operands)])


# ------------------------------------------------------------ transforms
SWEEP = [(1 << logn, name) for logn in range(2, 15) for name in ("lazy_top", "nonlazy_bottom", "wrap", "u64_top")]
# the wide family, and the two-pass degrees with two rows each
EXTRA = [(1024, QG), (16384, QG), (32768, P27), (65536, QG)]
# multiply once per kind of second operand (ntt_primes.multiply_partners)
OPS = ("forward", "inverse", "multiply rolled", "multiply squares", "multiply canonical", "forward_ntt_mul")


def modulus(n, name):
    if isinstance(name, int):
        return name
    return P.sweep_primes(n)[name] if name in P.SWEEP_NAMES else P.stream_primes(n)[name]


def operand_rows(n, q, inverse, ppb):
    """Full row set up to n = 1024; above, the constant and sparse extremes
    and the two mixed rows; two rows at the two-pass degrees.  Tiled to a
    ragged last workgroup."""
    names, base = P.base_rows(n, q, inverse=inverse, reduced=n > 1024)
    if n > 16384:
        top = "const lim-1" if "const lim-1" in names else "const q-1"  # q >= 2^62: lim = q
        keep = [names.index(top), names.index("mixed one slow word per 16")]
        names, base = [names[i] for i in keep], base[keep]
    return names, P.tile_rows(base, ppb + 3 if n <= 16384 else 2, ppb)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n,name", SWEEP + EXTRA)
def test_transforms_vs_pyref(fg, n, name, op):
    q = modulus(n, name)
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    assert r.primitive_root == pyref.find_psi(n, q)
    ppb = max(1, r.info.polys_per_block)
    names, x = operand_rows(n, q, op == "inverse", ppb)
    b = x.shape[0]
    if op == "forward":
        got, exp = r.forward_ntt(x), rows_of(ref_forward, q, x)
    elif op == "inverse":
        got, exp = r.inverse_ntt(x), rows_of(ref_inverse, q, x)
    elif op.startswith("multiply"):
        kind = op.split()[1]
        y = P.multiply_partners(x, names, q)[kind]
        if n > 16384 and kind != "rolled":  # one big-integer product of 2^16 slots takes seconds: the top row only
            x, y = x[:1], y[:1]
        got, exp = r.multiply(x, y), rows_of(ref_mul, q, x, y)
    else:
        w = P.weight_rows(n, q, b, 1)  # the kind changes every row
        got = r.forward_ntt_mul(x, w)
        exp = np.stack([np.array([int(f) * (int(v) % q) % q for f, v in zip(ref_forward(q, x[i]), w[i])],
                                 dtype=np.uint64) for i in range(b)])
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (op, sorted({names[i % len(names)] for i in bad}))


# ------------------------------------------------------------ ciphertext operations vs ring formulas
CT_CASES = [(n, name) for n in (256, 4096, 16384) for name in ("lazy_top", "u64_top")]
ct_cases = pytest.mark.parametrize("n,name", CT_CASES)


class Ring:
    """Negacyclic context, engine and ciphertext operands cut from the
    adversarial rows; the ring arithmetic of the expected values is Python
    integers over pyref.negacyclic_multiply."""

    def __init__(self, fg, n, name):
        self.n, self.q = n, modulus(n, name)
        self.ring = fg.PolynomialRing(n, self.q, mode="negacyclic")
        self.eng = fg.EncryptionEngine(self.ring, T)
        names, base = P.base_rows(n, self.q, reduced=True)
        # the rows a product is most likely to break on first: every word at the
        # top of the window, one slow word among in-window ones, sparse, raw
        order = ["const lim-1", "mixed one slow word per 16", "sparse alternating", "const 2^64-1",
                 "mixed in-window", "const lim", "sparse last", "const q-1"]
        # (q >= 2^62: the window is [0, q), lim-1 and lim are the q-1 and q rows)
        self.base = base[[names.index(x) for x in order if x in names]]

    def cts(self, count, comps, shift=0):
        rows = P.tile_rows(self.base, count * comps + shift)[shift:shift + count * comps]
        return np.ascontiguousarray(rows.reshape(count, comps, self.n))

    def key(self, seed, *lead):
        return rnd(seed + self.n, self.q, *lead, self.n)

    def mul(self, a, b):
        return [int(v) for v in ref_mul(self.q, a, b)]

    def arr(self, ints):
        return np.array([v % self.q for v in ints], dtype=np.uint64)

    def add(self, *polys):
        return [sum(int(v) for v in vs) % self.q for vs in zip(*polys)]

    def tensor(self, x, y):
        """(a0 b0, a0 b1 + a1 b0, a1 b1)"""
        return [self.mul(x[0], y[0]), self.add(self.mul(x[0], y[1]), self.mul(x[1], y[0])), self.mul(x[1], y[1])]


@ct_cases
def test_ct_multiply_is_ring_tensor(fg, n, name):
    R = Ring(fg, n, name)
    b = 2
    x, y = R.cts(b, 2), R.cts(b, 2, shift=3)
    got = R.eng.multiply(x, y)
    for i in range(b):
        assert (got[i] == np.stack([R.arr(c) for c in R.tensor(x[i], y[i])])).all(), i


@ct_cases
def test_relinearize_is_key_switch_sum(fg, n, name):
    """(c0 + sum_l d_l b_l, c1 + sum_l d_l a_l), d_l = (c2 >> l B) & (2^B - 1)
    of the raw word (include/fhe_gpu.h, fhe_relinearize_batch)."""
    R = Ring(fg, n, name)
    q, lv = R.q, 2
    bl = -(-q.bit_length() // lv)
    b = 1 if n == 16384 else 2
    ct3 = R.cts(b, 3)
    rlk = R.key(31, lv, 2)
    got = R.eng.relinearize(ct3, fg.EvaluationKey(R.ring, rlk, bl))
    for i in range(b):
        c0, c1 = [int(v) for v in ct3[i, 0]], [int(v) for v in ct3[i, 1]]
        for l in range(lv):
            d = [(int(v) >> (l * bl)) & ((1 << bl) - 1) for v in ct3[i, 2]]
            c0 = R.add(c0, R.mul(d, rlk[l, 1]))
            c1 = R.add(c1, R.mul(d, rlk[l, 0]))
        assert (got[i, 0] == R.arr(c0)).all() and (got[i, 1] == R.arr(c1)).all(), i


@ct_cases
def test_external_product_is_digit_sum(fg, n, name):
    """out_j = sum over the rows (i, l) of digit_l(glwe_i) * ggsw[i L + l][j],
    digits by the reference's decomposition (oracle.decompose)."""
    R = Ring(fg, n, name)
    q, lv, k = R.q, 2, 1
    bl = -(-q.bit_length() // lv)
    b = 1 if n == 16384 else 2
    glwe = R.cts(b, 2)
    ggsw = R.key(37, 2 * lv, 2)
    got = fg.ExternalProduct(R.ring, ggsw, bl, lv, k)(glwe)
    for i in range(b):
        out = [[0] * n, [0] * n]
        for c in range(2):
            dec = oracle.decompose(q, glwe[i, c], bl, lv)
            for l in range(lv):
                for j in range(2):
                    out[j] = R.add(out[j], R.mul(dec[l], ggsw[c * lv + l, j]))
        assert (got[i, 0] == R.arr(out[0])).all() and (got[i, 1] == R.arr(out[1])).all(), i


@ct_cases
def test_encrypt_is_rlwe_formula(fg, n, name):
    """(pk.b u + e1 + m, pk.a u + e2), m = oracle.encode(values)."""
    R = Ring(fg, n, name)
    b = 2
    pk = R.key(41, 2)
    ops = R.cts(b, 4)
    vals, u, e1, e2 = (np.ascontiguousarray(ops[:, j]) for j in range(4))
    ct = R.eng.encrypt(vals, fg.PublicKey(R.ring, pk), u, e1, e2)
    for i in range(b):
        m = oracle.encode(R.q, T, vals[i])
        assert (ct[i, 0] == R.arr(R.add(R.mul(pk[1], u[i]), e1[i], m))).all(), i
        assert (ct[i, 1] == R.arr(R.add(R.mul(pk[0], u[i]), e2[i]))).all(), i


@ct_cases
@pytest.mark.parametrize("comps", [2, 3])
def test_decrypt_phase_is_ring_formula(fg, n, name, comps):
    """phase = c0 - c1 s (- c2 s^2); values and max_noise from the phase by
    the rule of include/fhe_gpu.h (fhe_decrypt_batch)."""
    R = Ring(fg, n, name)
    q, b = R.q, 2
    s = rnd(43 + n, 3, n)
    s = np.where(s == 2, np.uint64(q - 1), s).astype(np.uint64)
    ct = R.cts(b, comps)
    res = R.eng.decrypt(ct, fg.SecretKey(R.ring, s), with_phase=True)
    s2 = R.mul(s, s)
    delta = q // T
    for i in range(b):
        ph = [int(v) for v in ct[i, 0]]
        ph = R.add(ph, [-v for v in R.mul(ct[i, 1], s)])
        if comps == 3:
            ph = R.add(ph, [-v for v in R.mul(ct[i, 2], s2)])
        assert (res.phase[i] == R.arr(ph)).all(), i
        rounded = [(c * T + q // 2) // q for c in ph]
        assert (res.values[i] == np.array([v % T for v in rounded], dtype=np.uint64)).all(), i
        noise = [abs(c - v * delta % q) for c, v in zip(ph, rounded)]
        assert int(res.max_noise[i]) == max(q - v if v > q // 2 else v for v in noise), i


@ct_cases
def test_dot_is_sum_of_tensors(fg, n, name):
    R = Ring(fg, n, name)
    count = 3
    a, bb = R.cts(count, 2), R.cts(count, 2, shift=3)
    got = R.eng.dot(a, bb)
    terms = [R.tensor(a[i], bb[i]) for i in range(count)]
    for j in range(3):
        assert (got[j] == R.arr(R.add(*[t[j] for t in terms]))).all(), j


# ------------------------------------------------------------ squaring, threshold decryption, plaintext dot
# ct_cases, and the composed paths of the wide family, whose true inverses
# only negacyclic mode uses: 2^64 - 2^32 + 1 and the first prime above 2^63.
# The tests cut the same operands, so the tensor of one is the cached
# reference of the next.
NEW_CASES = CT_CASES + [(1024, QG), (1024, "wmont_bottom")]
new_cases = pytest.mark.parametrize("n,name", NEW_CASES)


def square_operands(R):
    b = 1 if R.n == 16384 else 2
    return b, R.cts(b, 2), R.cts(b, 2, shift=3)


def difference(R, ct, ref):
    """ct - ref per component, canonical Python integers."""
    return [[(int(x) % R.q - int(y) % R.q) % R.q for x, y in zip(ct[j], ref[j])] for j in range(2)]


def live(polys):
    """Every polynomial of the expected value has a nonzero coefficient."""
    return all(any(p) for p in polys)


@new_cases
def test_square_is_ring_tensor(fg, n, name):
    """square(ct) = ct (x) ct and squared_difference(ct, ref) = d (x) d,
    d = ct - ref, with one ref per ciphertext and one shared by all."""
    R = Ring(fg, n, name)
    b, x, ref = square_operands(R)
    got = R.eng.square(x)
    for i in range(b):
        exp = R.tensor(x[i], x[i])
        assert live(exp), i
        assert (got[i] == np.stack([R.arr(c) for c in exp])).all(), i
    for rf in (ref, ref[0]) if b > 1 else (ref,):
        got = R.eng.squared_difference(x, rf)
        for i in range(b):
            d = difference(R, x[i], rf if rf.ndim == 2 else rf[i])
            exp = R.tensor(d, d)
            assert live(exp), (rf.ndim, i)
            assert (got[i] == np.stack([R.arr(c) for c in exp])).all(), (rf.ndim, i)


@new_cases
def test_square_relin_is_key_switch_sum(fg, n, name):
    """The key-switch sum of test_relinearize_is_key_switch_sum applied to the
    tensor of the difference (its c2 is a canonical word)."""
    R = Ring(fg, n, name)
    q, lv = R.q, 2
    bl = -(-q.bit_length() // lv)
    b, x, ref = square_operands(R)
    rlk = R.key(47, lv, 2)
    ek = fg.EvaluationKey(R.ring, rlk, bl)
    # square_relin is the same entry point without a ref; at n = 16384 one of the two
    for rf in (ref,) if n == 16384 else (None, ref):
        got = R.eng.square_relin(x, ek) if rf is None else R.eng.compute_anomaly_score(x, rf, ek)
        for i in range(b):
            d = [[int(v) % q for v in x[i, j]] for j in range(2)] if rf is None else difference(R, x[i], rf[i])
            c0, c1, c2 = R.tensor(d, d)
            assert any(c2)
            for l in range(lv):
                dg = [(v >> (l * bl)) & ((1 << bl) - 1) for v in c2]
                c0 = R.add(c0, R.mul(dg, rlk[l, 1]))
                c1 = R.add(c1, R.mul(dg, rlk[l, 0]))
            assert any(c0) and any(c1)
            assert (got[i, 0] == R.arr(c0)).all() and (got[i, 1] == R.arr(c1)).all(), (rf is None, i)


@new_cases
def test_partial_decrypt_and_combine_are_ring_formulas(fg, n, name):
    """partial_s = c1 share_s for one and for three shares; combining the
    three with the Lagrange coefficients of the ids (1, 3, 4) opens
    c0 - c1 (sum_s lambda_s share_s)."""
    R = Ring(fg, n, name)
    q, ids = R.q, (1, 3, 4)
    b, x, _ = square_operands(R)
    sh = R.cts(1, 3, shift=1)[0]  # raw words: one slow word per 16, sparse, 2^64 - 1
    shares = [fg.KeyShare(R.ring, i, sh[k]) for k, i in enumerate(ids)]
    got = R.eng.partial_decrypt(x, shares)
    assert got.shape == (3, b, n)
    for k in range(3):
        for i in range(b):
            exp = R.mul(x[i, 1], sh[k])
            assert any(exp)
            assert (got[k, i] == R.arr(exp)).all(), (k, i)
    one = R.eng.partial_decrypt(x, shares[:1])
    assert one.shape == (1, b, n) and (one == got[:1]).all()
    lam = [1] * 3
    for k, i in enumerate(ids):
        for j in ids:
            if j != i:
                lam[k] = lam[k] * j * pow(j - i, -1, q) % q
    assert sum(lam) % q == 1 and all(lam)
    key = [sum(l * (int(v) % q) for l, v in zip(lam, col)) % q for col in zip(*sh)]
    if q < 1 << 63:
        assert fg.lagrange_coefficients(q, ids) == lam
        res = R.eng.combine_partial_decryptions(x, got, ids, with_phase=True)
    else:
        # lagrange_coefficients is the reference's lagrange_coefficient, whose signed Euclid
        # returns no inverse at q >= 2^63 (fhe_gpu.cpp ref_mod_inverse): (0, 4, 0) for these
        # ids, pinned here.  The interpolating coefficients go to the kernel directly.
        assert fg.lagrange_coefficients(q, ids) == [0, 4, 0]
        res = R.eng.combine_partials(x, got, lam, with_phase=True)
    delta = q // T
    for i in range(b):
        ph = R.add([int(v) for v in x[i, 0]], [-v for v in R.mul(x[i, 1], key)])
        assert any(ph)
        assert (res.phase[i] == R.arr(ph)).all(), i
        if q < 1 << 63:  # above, the noise distance is the reference's wrapping int64 one (test_gpu_ranges_stream.py)
            rounded = [(c * T + q // 2) // q for c in ph]
            assert (res.values[i] == np.array([v % T for v in rounded], dtype=np.uint64)).all(), i
            noise = [abs(c - v * delta % q) for c, v in zip(ph, rounded)]
            assert int(res.max_noise[i]) == max(q - v if v > q // 2 else v for v in noise), i


@new_cases
def test_dot_plain_is_sum_of_products(fg, n, name):
    """(sum_i c0_i p_i, sum_i c1_i p_i), count 3."""
    R = Ring(fg, n, name)
    count = 3
    cts = R.cts(count, 2)
    pts = np.ascontiguousarray(R.cts(count, 1, shift=5)[:, 0])
    got = R.eng.dot_plain(cts, pts)
    assert got.shape == (2, n)
    for j in range(2):
        exp = R.add(*[R.mul(cts[i, j], pts[i]) for i in range(count)])
        assert any(exp)
        assert (got[j] == R.arr(exp)).all(), j
