"""GPU parity at the edges of the range analysis: every degree 4..16384 with
the NTT-friendly primes on either side of each kernel-family threshold
(tests/ntt_primes.py: the lazy bound (4 + 2 log2 N) q <= 2^32 of
fhe_ctx_create, q = 2^30 between 32- and 64-bit lanes, q = 2^62 at the top
of the 64-bit lanes; and the first prime at which the lazy butterflies would
wrap on a known row, ntt_primes.wrap_prime), fed with rows that fill the
unreduced input windows instead of random ones: every word at the top of
[0, 4q) (forward-type loads) or [0, 2q) (inverse loads), rows congruent to 0
that are not 0, sparse rows, and rows where one word of a thread leaves the
window.

Compat mode, bit-exact against the CPU oracle (oracle/ref_cpu.c).

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import ntt_primes as P
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def rnd(seed, q, *shape):
    return oracle.splitmix_fill(seed, q, int(np.prod(shape))).reshape(shape)


def bad_rows(got, exp, names):
    """Names of the (tiled) base rows whose words differ, for the message."""
    rows = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0]
    return sorted({names[i % len(names)] for i in rows})


# ------------------------------------------------------------ transforms
@pytest.mark.parametrize("name", P.SWEEP_NAMES)
@pytest.mark.parametrize("logn", range(2, 15))
def test_window_rows_vs_oracle(fg, logn, name):
    n = 1 << logn
    q = P.sweep_primes(n)[name]
    assert P.word_bits(q) == (64 if name in ("u64_bottom", "u64_top") else 32)
    check_window_rows(fg, n, q)


def test_window_rows_benchmark_shape(fg):
    """bench.py's own context (N = 16384, q = 132120577: lazy, at 98.4 % of
    the bound) with the same rows, the all-zero and all-(q-1) ones included."""
    assert P.is_lazy(16384, 132120577)
    check_window_rows(fg, 16384, 132120577)


def check_window_rows(fg, n, q):
    import torch

    r = fg.PolynomialRing(n, q)
    t = oracle.NTT(n, q)
    assert r.info.word_bits == P.word_bits(q)
    assert r.primitive_root == t.psi
    ppb = r.info.polys_per_block
    assert 1 <= ppb <= 256

    names, base = P.base_rows(n, q)
    inames, ibase = P.base_rows(n, q, inverse=True)
    # four tiles of the base rows (each meets every kind of second operand),
    # at least polys_per_block + 3 rows, never a whole number of workgroups
    x = P.tile_rows(base, max(ppb + 3, 4 * len(names)), ppb)
    xi = P.tile_rows(ibase, max(ppb + 3, len(inames)), ppb)
    b = x.shape[0]

    got = r.forward_ntt(x)
    exp_fwd = t.forward(x)
    assert (got == exp_fwd).all(), ("forward", bad_rows(got, exp_fwd, names))

    got = r.inverse_ntt(xi)
    exp = t.inverse(xi)
    assert (got == exp).all(), ("inverse", bad_rows(got, exp, inames))

    # extreme rows against each other, against themselves (lim-1 against
    # lim-1), and against a nonzero canonical row (ntt_primes.multiply_partners)
    for kind, y in P.multiply_partners(x, names, q).items():
        got = r.multiply(x, y)
        exp = t.polymul(x, y)
        assert (got == exp).all(), ("multiply", kind, bad_rows(got, exp, names))

    w = P.weight_rows(n, q, b, len(names))
    got = r.forward_ntt_mul(x, w)
    exp = t.fwd_mul(x, w)
    assert (got == exp).all(), ("forward_ntt_mul", bad_rows(got, exp, names))

    got = r.pointwise_multiply(x, w)
    exp = oracle.pointwise(q, x.ravel(), w.ravel()).reshape(b, n)
    assert (got == exp).all(), ("pointwise_multiply", bad_rows(got, exp, names))

    dx = torch.from_numpy(x.view(np.int64)).cuda()
    r.forward_ntt(dx, out=dx)  # in place on the device
    torch.cuda.synchronize()
    got = dx.cpu().numpy().view(np.uint64)
    assert (got == exp_fwd).all(), ("forward in place", bad_rows(got, exp_fwd, names))


# ------------------------------------------------------------ fused ciphertext kernels
FUSED_N = (16, 256, 1024, 4096, 16384)
FUSED_PRIMES = ("lazy_top", "nonlazy_bottom", "wrap", "u64_top")
fused = pytest.mark.parametrize("n,name", [(n, p) for n in FUSED_N for p in FUSED_PRIMES])


def digits(q, level):
    """base_log for `level` digits that together cover the bits of q."""
    return -(-q.bit_length() // level)


class Ctx:
    """One compat context, its oracle and ciphertext operands cut from the
    adversarial rows: cts(count, comps) -> [count, comps, n]."""

    def __init__(self, fg, n, name):
        self.n, self.q = n, P.sweep_primes(n)[name]
        self.ring = fg.PolynomialRing(n, self.q)
        self.ref = oracle.NTT(n, self.q)
        self.eng = fg.EncryptionEngine(self.ring, 16)
        self.names, self.base = P.base_rows(n, self.q)

    def cts(self, count, comps, shift=0):
        rows = P.tile_rows(self.base, count * comps + shift)[shift:shift + count * comps]
        return np.ascontiguousarray(rows.reshape(count, comps, self.n))

    def keys(self, seed, *lead):
        """Canonical random key rows; the first one all q-1 (the largest products)."""
        k = rnd(seed + self.n, self.q, *lead, self.n)
        k.reshape(-1, self.n)[0] = self.q - 1
        return k

    def ternary(self, seed):
        s = rnd(seed + self.n, 3, self.n)
        return np.where(s == 2, np.uint64(self.q - 1), s).astype(np.uint64)


@fused
def test_fused_ct_multiply(fg, n, name):
    c = Ctx(fg, n, name)
    b = len(c.names)
    x = c.cts(b, 2)
    for y in (c.cts(b, 2, shift=5), x):  # other rows, and the squares (lim-1 against lim-1)
        for is_ntt in (False, True):
            got = c.eng.multiply(x, y, is_ntt=is_ntt)
            for i in range(b):
                assert (got[i] == c.ref.ct_multiply(x[i], y[i], is_ntt=is_ntt)).all(), (y is x, is_ntt, i)


@fused
def test_fused_relinearize(fg, n, name):
    c = Ctx(fg, n, name)
    b = len(c.names)
    lv = 3 if c.q < 1 << 30 else 4
    bl = digits(c.q, lv)
    ct3 = c.cts(b, 3)
    rlk = c.keys(11, lv, 2)
    got = c.eng.relinearize(ct3, fg.EvaluationKey(c.ring, rlk, bl))
    for i in range(b):
        assert (got[i] == c.ref.relinearize(bl, lv, ct3[i], rlk)).all(), i


@fused
@pytest.mark.parametrize("lv", [1, 2])
def test_fused_external_product(fg, n, name, lv):
    c = Ctx(fg, n, name)
    b, k = len(c.names), 1
    bl = digits(c.q, lv)
    glwe = c.cts(b, 2)
    ggsw = c.keys(13 + lv, 2 * lv, 2)
    got = fg.ExternalProduct(c.ring, ggsw, bl, lv, k)(glwe)
    for i in range(b):
        assert (got[i] == c.ref.external_product(k, bl, lv, glwe[i], ggsw)).all(), i


@fused
def test_fused_encrypt(fg, n, name):
    c = Ctx(fg, n, name)
    b = len(c.names)
    pk = c.keys(17, 2)
    ops = c.cts(b, 4)  # values, u, e1, e2: any u64, read mod q (values: times delta, wrapping)
    vals, u, e1, e2 = (np.ascontiguousarray(ops[:, j]) for j in range(4))
    ct = c.eng.encrypt(vals, fg.PublicKey(c.ring, pk), u, e1, e2)
    for i in range(b):
        assert (ct[i] == c.ref.encrypt(16, pk, vals[i], u[i], e1[i], e2[i])).all(), i


@fused
@pytest.mark.parametrize("comps", [2, 3])
def test_fused_decrypt(fg, n, name, comps):
    c = Ctx(fg, n, name)
    b = len(c.names)
    sk = c.ternary(19)
    key = fg.SecretKey(c.ring, sk)
    ct = c.cts(b, comps)
    for is_ntt in (False, True):
        res = c.eng.decrypt(ct, key, is_ntt=is_ntt, with_phase=True)
        for i in range(b):
            ev, eph, emx = c.ref.decrypt(16, sk, ct[i], is_ntt)
            assert (res.phase[i] == eph).all(), (is_ntt, i)
            assert (res.values[i] == ev).all(), (is_ntt, i)
            assert int(res.max_noise[i]) == emx, (is_ntt, i)


@fused
def test_fused_add_plain(fg, n, name):
    c = Ctx(fg, n, name)
    b = len(c.names)
    ct = c.cts(b, 2)
    vals = np.ascontiguousarray(c.cts(b, 1, shift=7)[:, 0])
    for is_ntt in (False, True):
        got = c.eng.add_plain(ct, vals, is_ntt=is_ntt)
        for i in range(b):
            assert (got[i] == c.ref.add_plain(16, ct[i], vals[i], is_ntt)).all(), (is_ntt, i)


@fused
@pytest.mark.parametrize("split", [None, "2"])
def test_fused_dot(fg, monkeypatch, n, name, split):
    """fhe_ct_dot_batch, count 3: the sequential poly_add fold of the oracle's
    ct_multiply over the pairs (inputs read as x mod q)."""
    c = Ctx(fg, n, name)
    groups, count = 3, 3
    a = c.cts(groups * count, 2).reshape(groups, count, 2, n)
    bb = c.cts(groups * count, 2, shift=5).reshape(groups, count, 2, n)
    qq = np.uint64(c.q)
    exp = np.empty((groups, 3, n), dtype=np.uint64)
    for g in range(groups):
        acc = np.zeros(3 * n, dtype=np.uint64)
        for i in range(count):
            acc = oracle.poly_add(c.q, acc, c.ref.ct_multiply(a[g, i] % qq, bb[g, i] % qq).ravel())
        exp[g] = acc.reshape(3, n)
    if split is None:
        monkeypatch.delenv("FHE_DOT_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_DOT_SPLIT", split)
    got = c.eng.dot(a, bb)
    assert (got == exp).all()


@pytest.mark.parametrize("name", ["lazy_top", "u64_top"])
def test_fused_blind_rotate(fg, name):
    n, k, dim, lv = 1024, 1, 4, 3
    c = Ctx(fg, n, name)
    q = c.q
    bl = digits(q, lv)
    b = len(c.names)
    be = fg.BootstrapEngine(c.ring, bl, lv, k)
    bsk = c.keys(23, dim, (k + 1) * lv, k + 1)
    lwe_a = rnd(24, q, b, dim)
    lwe_a[0, :2] = [0, q - 1]  # a skipped step, a rotation of 2N
    lwe_b = rnd(25, q, b)
    acc0 = c.cts(b, k + 1)
    acc = acc0.copy()
    be.blind_rotate(acc, lwe_a, lwe_b, be.prepare_ggsw(bsk))
    for i in range(b):
        exp = c.ref.blind_rotate(k, bl, lv, lwe_a[i], int(lwe_b[i]), q, bsk, acc0[i])
        assert (acc[i] == exp).all(), i
