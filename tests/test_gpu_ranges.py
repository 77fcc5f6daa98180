"""GPU parity at the edges of the range analysis: every degree 4..16384 with
the NTT-friendly primes on either side of each kernel-family threshold
(tests/ntt_primes.py: the lazy bound (4 + 2 log2 N) q <= 2^32 of
fhe_ctx_create, q = 2^30 between 32- and 64-bit lanes, q = 2^62 at the top
of the 64-bit lanes; and the first prime at which the lazy butterflies would
wrap on a known row, ntt_primes.wrap_prime), fed with rows that fill the
unreduced input windows instead of random ones: every word at the top of
[0, 4q) (forward-type loads) or [0, 2q) (inverse loads), rows congruent to 0
that are not 0, sparse rows, and rows where one word of a thread leaves the
window.  The fused ciphertext kernels run on operands cut from those rows;
squaring, the squared difference, partial decryption and the plaintext dot
product at every degree, since their instantiations differ from one log2 N to
the next.  (The streaming kernels' edges, around q = 2^63, are in
test_gpu_ranges_stream.py; the two-pass degrees 32768 and 65536 in
test_gpu_ranges_big.py, which runs check_window_rows and the fused bodies
below.)

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


def check_window_rows(fg, n, q, tiles=4, ragged_for=None):
    """tiles: how often the base rows repeat (and one row more below four);
    ragged_for: the row count is no multiple of it (default: the polynomials
    per workgroup)."""
    import torch

    r = fg.PolynomialRing(n, q)
    t = oracle.NTT(n, q)
    assert r.info.word_bits == P.word_bits(q)
    assert r.primitive_root == t.psi
    ppb = r.info.polys_per_block
    assert 1 <= ppb <= 256
    ragged_for = ppb if ragged_for is None else ragged_for

    names, base = P.base_rows(n, q)
    inames, ibase = P.base_rows(n, q, inverse=True)
    # four tiles of the base rows (each meets every kind of second operand),
    # at least polys_per_block + 3 rows, never a whole number of workgroups
    x = P.tile_rows(base, max(ppb + 3, tiles * len(names) + (tiles < 4)), ragged_for)
    xi = P.tile_rows(ibase, max(ppb + 3, len(inames)), ragged_for)
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
        self.n, self.q = n, name if isinstance(name, int) else P.sweep_primes(n)[name]
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


def check_ct_multiply(c, x, others):
    """x [b, 2, n] against each second operand of `others`, both domains."""
    for y in others:
        for is_ntt in (False, True):
            got = c.eng.multiply(x, y, is_ntt=is_ntt)
            for i in range(x.shape[0]):
                assert (got[i] == c.ref.ct_multiply(x[i], y[i], is_ntt=is_ntt)).all(), (y is x, is_ntt, i)


def check_relinearize(fg, c, ct3):
    lv = 3 if c.q < 1 << 30 else 4
    bl = digits(c.q, lv)
    rlk = c.keys(11, lv, 2)
    got = c.eng.relinearize(ct3, fg.EvaluationKey(c.ring, rlk, bl))
    for i in range(ct3.shape[0]):
        assert (got[i] == c.ref.relinearize(bl, lv, ct3[i], rlk)).all(), i


def check_decrypt(fg, c, ct):
    sk = c.ternary(19)
    key = fg.SecretKey(c.ring, sk)
    for is_ntt in (False, True):
        res = c.eng.decrypt(ct, key, is_ntt=is_ntt, with_phase=True)
        for i in range(ct.shape[0]):
            ev, eph, emx = c.ref.decrypt(16, sk, ct[i], is_ntt)
            assert (res.phase[i] == eph).all(), (is_ntt, i)
            assert (res.values[i] == ev).all(), (is_ntt, i)
            assert int(res.max_noise[i]) == emx, (is_ntt, i)


@fused
def test_fused_ct_multiply(fg, n, name):
    c = Ctx(fg, n, name)
    b = len(c.names)
    x = c.cts(b, 2)
    check_ct_multiply(c, x, (c.cts(b, 2, shift=5), x))  # other rows, and the squares (lim-1 against lim-1)


@fused
def test_fused_relinearize(fg, n, name):
    c = Ctx(fg, n, name)
    check_relinearize(fg, c, c.cts(len(c.names), 3))


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
    check_decrypt(fg, c, c.cts(len(c.names), comps))


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


# ------------------------------------------------------------ squaring, partial decryption, plaintext dot
# ct_square.hip, threshold.hip k_partial_dec and dot_plain.hip are instantiated
# for every log2 n from 2 to 14 (polynomials per workgroup and the stash of
# the spectrum -- registers, LDS, the output row -- change in between), so
# these run at every degree.  The oracle sees every raw input mod q.
every_degree = pytest.mark.parametrize("n,name", [(1 << logn, p) for logn in range(2, 15) for p in FUSED_PRIMES])
P27 = 132120577
Q62 = 4611686018429485057     # 2^62 + 2^21 + 1 and
Q63 = 9223370937344327681     # just below 2^63: wide transforms with a true N^-1 (test_gpu_wide.py)
# outside the fused family (two-pass degree, wide moduli): the composed paths,
# two ciphertexts.  At QG the compat N^-1 is the reference's 0 and every
# coefficient-form result is all zeros (test_gpu_wide.py), so only the
# NTT-domain results say anything there.
# P27 is past the lazy bound at 32768, so the lazy row kernel of ntt_big.hip
# and the first 64-bit modulus at 65536 come in through BIG_COMPOSED.
BIG_COMPOSED = [(32768, P.sweep_primes(32768)["lazy_top"]), (65536, P.sweep_primes(65536)["u64_bottom"])]
COMPOSED = [(32768, P27), (1024, Q62), (1024, Q63), (1024, P.QG)] + BIG_COMPOSED
composed = pytest.mark.parametrize("n,q", COMPOSED)
COEFF_COMPOSED = [nq for nq in COMPOSED if nq[1] != P.QG]  # coefficient-form results: not at QG


def domains(q):
    return (True,) if q == P.QG else (False, True)


def ragged(c, b):
    """A batch of b ciphertexts leaves a workgroup partly filled (or every
    ciphertext has a workgroup of its own)."""
    ppb = c.ring.info.polys_per_block
    return ppb <= 1 or b % ppb != 0


def cut(c, few=False, extra=0):
    """Ciphertexts [b, 2, n] cut from the adversarial rows at shifts 0 and 1,
    so that every row is a c0 and a c1; with the `extra` ciphertexts the
    caller appends, b + extra is no multiple of the polynomials per workgroup
    (a tail ciphertext exists).  few: two ciphertexts, the top-of-window and
    the one-slow-word rows as c0 and as c1."""
    if few:
        top = "const lim-1" if "const lim-1" in c.names else "const q-1"
        rows = c.base[[c.names.index(top), c.names.index("mixed one slow word per 16")]]
        return np.ascontiguousarray(np.stack([rows, rows[::-1]]))
    half = -(-len(c.names) // 2)
    x = np.concatenate([c.cts(half, 2), c.cts(half, 2, shift=1)])
    if not ragged(c, x.shape[0] + extra):
        x = np.concatenate([x, c.cts(1, 2, shift=2)])
    assert ragged(c, x.shape[0] + extra)
    return np.ascontiguousarray(x)


def lift(v, k, q):
    """v + k q (fewer multiples where that leaves the word: q >= 2^62)."""
    v = np.asarray(v, dtype=np.uint64)
    room = (np.uint64(P.M64) - v) // np.uint64(q)
    return v + np.minimum(room, np.uint64(k)) * np.uint64(q)


def mixed_pair(n, q, seed):
    """A ciphertext and its ref [2, n] whose word pairs change kind from word
    to word.  The difference loader (ntt_core.hpp load_diff_chunked) takes a
    thread's pairs CH = min(E, 8) at a time (E coefficients per thread) and
    sends only the pairs with a word >= q to its slow path.  With one
    polynomial per workgroup and E >= 8 a chunk is the words p, p + n/8, ..,
    p + 7n/8: kind = (8 pos // n + pos mod (n / 8) + 4 comp) mod 8 puts all
    eight kinds into every such set of positions, whichever E the kernel has
    (asserted below); a chunk of fewer words is a subset of one of these sets
    and holds as many different kinds as it has words.  Below n = 8,
    kind = pos + 4 comp: all eight over the two components together.
      0 only the ct word >= q      4 ct = ref + q  (congruent, not equal)
      1 only the ref word >= q     5 ref = ct + 3q (the same, the other way)
      2 both >= q                  6 ct = 2^64 - 1
      3 neither                    7 ref = 4q + 1
    Every ref residue is nonzero (below_of needs that)."""
    rng = np.random.default_rng([n, q % (1 << 32), q >> 32, seed])
    a = rng.integers(1, q, size=(2, n), dtype=np.uint64)
    b = rng.integers(1, q, size=(2, n), dtype=np.uint64)
    b = np.where(a == b, np.uint64(1) + (b % np.uint64(q - 1)), b)  # (a fresh residue where they met; q > 2)
    pos = np.arange(n)
    kind = np.stack([((8 * pos // n + pos % (n // 8) if n >= 8 else pos) + 4 * comp) % 8 for comp in range(2)])
    ct, ref = a.copy(), b.copy()
    for k, (cv, rv) in enumerate([(lift(a, 1, q), b), (a, lift(b, 1, q)), (lift(a, 2, q), lift(b, 3, q)), (a, b),
                                  (lift(a, 1, q), a), (a, lift(a, 3, q)), (np.full_like(a, P.M64), b),
                                  (a, lift(np.ones_like(a), 4, q))]):
        ct, ref = np.where(kind == k, cv, ct), np.where(kind == k, rv, ref)
    assert set(kind.reshape(-1).tolist()) == set(range(8))
    for comp in range(2):  # the chunk positions p + k n/8 (and p + k n/CH for a shorter chunk) differ in kind
        for p in range(n // 8):
            assert sorted(kind[comp, p::n // 8].tolist()) == list(range(8)), (n, comp, p)
    if 4 * q <= P.M64:  # each kind is what its name says (q >= 2^62: lift() has no room for every multiple)
        qq = np.uint64(q)
        assert ((ct >= qq) & (ref < qq))[kind == 0].all() and ((ct < qq) & (ref >= qq))[kind == 1].all()
        assert ((ct >= qq) & (ref >= qq))[kind == 2].all() and ((ct < qq) & (ref < qq))[kind == 3].all()
        assert ((ct % qq == ref % qq) & (ct != ref))[(kind == 4) | (kind == 5)].all()
        assert (ct[kind == 6] == np.uint64(P.M64)).all() and (ref[kind == 7] == np.uint64(4 * q + 1)).all()
    return np.ascontiguousarray(ct), np.ascontiguousarray(ref), kind


def below_of(ref, q, seed):
    """Canonical words below the residue of every word of ref (all nonzero):
    each difference wraps."""
    r = ref % np.uint64(q)
    assert r.all()
    return np.random.default_rng([seed, q % (1 << 32)]).integers(0, 1 << 62, size=ref.shape, dtype=np.uint64) % r


def difference_operands(c, shared, few=False):
    """(ct [b, 2, n], ref [2, n] or [b, 2, n], index of the ciphertext that
    equals its ref).  The last three ciphertexts are designed: mixed_pair,
    one equal to its ref word for word, one below its ref's residue in every
    word; before them the adversarial rows, the refs cut at another shift."""
    n, q = c.n, c.q
    x = cut(c, few, extra=3)
    mct, mref, _ = mixed_pair(n, q, 1)
    if shared:
        ct = np.concatenate([x, np.stack([mct, mref, below_of(mref, q, 2)])])
        return np.ascontiguousarray(ct), mref, ct.shape[0] - 2
    y = c.cts(x.shape[0], 2, shift=7)     # (a shift at which no ciphertext is congruent to its ref by accident)
    eq = c.cts(1, 2, shift=9)[0]          # raw words, equal ones on both sides
    lo_ref = lift(mixed_pair(n, q, 3)[1] % np.uint64(q), 2, q)
    ct = np.concatenate([x, np.stack([mct, eq, below_of(lo_ref, q, 4)])])
    ref = np.concatenate([y, np.stack([mref, eq, lo_ref])])
    return np.ascontiguousarray(ct), np.ascontiguousarray(ref), ct.shape[0] - 2


def square_expected(ref, q, ct, rf, is_ntt):
    """ct_multiply(d, d) per ciphertext, d = poly_sub(ct % q, rf % q)
    (test_gpu_square.py's expected())."""
    qq = np.uint64(q)
    out = np.empty((ct.shape[0], 3, ct.shape[-1]), dtype=np.uint64)
    for i in range(ct.shape[0]):
        d = np.ascontiguousarray(ct[i] % qq)
        if rf is not None:
            ri = rf if rf.ndim == 2 else rf[i]
            d = oracle.poly_sub(q, d.ravel(), np.ascontiguousarray(ri % qq).ravel()).reshape(d.shape)
        out[i] = ref.ct_multiply(d, d, is_ntt)
    return out


def check_square(c, few=False):
    x = cut(c, few)
    live = (x % np.uint64(c.q)).reshape(x.shape[0], -1).any(axis=1)   # rows 0, q, 2q, .. pair up to a zero ciphertext
    assert live.sum() > x.shape[0] // 2
    for is_ntt in domains(c.q):
        exp = square_expected(c.ref, c.q, x, None, is_ntt)
        assert (exp.reshape(x.shape[0], -1).any(axis=1) == live).all(), is_ntt
        got = c.eng.square(x, is_ntt=is_ntt)
        bad = np.nonzero((got != exp).reshape(x.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (is_ntt, bad.tolist())


def check_squared_difference(c, few=False):
    for shared in (True, False):
        ct, rf, zero = difference_operands(c, shared, few)
        b = ct.shape[0]
        assert few or ragged(c, b)
        for is_ntt in domains(c.q):
            exp = square_expected(c.ref, c.q, ct, rf, is_ntt)
            live = exp.reshape(b, -1).any(axis=1)
            assert not live[zero] and live[np.arange(b) != zero].all(), (shared, is_ntt, np.nonzero(~live)[0].tolist())
            got = c.eng.squared_difference(ct, rf, is_ntt=is_ntt)
            bad = np.nonzero((got != exp).reshape(b, -1).any(axis=1))[0]
            assert bad.size == 0, (shared, is_ntt, bad.tolist(), b)


def check_square_relin(fg, c, few=False):
    lv = 3 if c.q < 1 << 30 else 4
    bl = digits(c.q, lv)
    rlk = c.keys(29, lv, 2)
    ek = fg.EvaluationKey(c.ring, rlk, bl)
    for mode in ("none", "shared", "each"):
        if mode == "none":
            ct, rf, zero = cut(c, few), None, None
            got = c.eng.square_relin(ct, ek)
        else:
            ct, rf, zero = difference_operands(c, mode == "shared", few)
            got = c.eng.compute_anomaly_score(ct, rf, ek)
        ct3 = square_expected(c.ref, c.q, ct, rf, False)
        assert got.shape == ct.shape and (few or ragged(c, ct.shape[0]))
        for i in range(ct.shape[0]):
            exp = c.ref.relinearize(bl, lv, ct3[i], rlk)
            assert exp.any() == ct3[i].any() and (i == zero or mode == "none" or exp.any()), (mode, i)
            assert (got[i] == exp).all(), (mode, i)


def check_partial_decrypt(fg, c, few=False):
    """1 and 3 shares (k_partial_dec's MULTI variants): raw share rows from
    the adversarial rows, one of the three all q-1."""
    qq = np.uint64(c.q)
    ct = cut(c, few)
    b = ct.shape[0]
    c1 = np.ascontiguousarray(ct[:, 1])
    live = (c1 % qq).any(axis=1)
    assert live.sum() > b // 2  # the others: c1 is one of the rows 0, q, 2q, ..
    top = "const lim-1" if "const lim-1" in c.names else "const 2^64-1"
    row = {nm: c.base[c.names.index(nm)] for nm in (top, "mixed one slow word per 16", "const q-1", "sparse alternating")}
    for picked in ((top,), ("mixed one slow word per 16", "const q-1", "sparse alternating")):
        sh = np.stack([row[nm] for nm in picked])
        assert (sh % qq).any(axis=1).all()
        shares = [fg.KeyShare(c.ring, i + 1, sh[i]) for i in range(len(picked))]
        got = c.eng.partial_decrypt(ct, shares)
        assert got.shape == (len(picked), b, c.n)
        for s in range(len(picked)):
            exp = c.ref.polymul(c1 % qq, np.ascontiguousarray(np.broadcast_to(sh[s] % qq, c1.shape)))
            assert (exp.any(axis=1) == live).all(), picked[s]
            bad = np.nonzero((got[s] != exp).any(axis=1))[0]
            assert bad.size == 0, (picked[s], bad.tolist())


_DOT_PLAIN = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_dot_plain_references():
    yield
    _DOT_PLAIN.clear()


def dot_plain_operands(c, is_ntt):
    """cts [3, 3, 2, n], pts [3, 3, n] (the adversarial rows at another shift)
    and the oracle's fold (test_gpu_dot_plain.py's fold()), computed once for
    both split settings."""
    key = (c.n, c.q, is_ntt)
    if key not in _DOT_PLAIN:
        groups, count, n, q = 3, 3, c.n, c.q
        qq = np.uint64(q)
        # group g takes ballots g, g + 3, g + 6 of the cut: the rows 0, q, 2q, 3q at its
        # start are dealt to all three groups, so no component of a group sums to zero
        deal = [g + groups * i for g in range(groups) for i in range(count)]
        cts = np.ascontiguousarray(c.cts(groups * count, 2)[deal]).reshape(groups, count, 2, n)
        pts = np.ascontiguousarray(c.cts(groups * count, 1, shift=7)[deal, 0]).reshape(groups, count, n)
        exp = np.empty((groups, 2, n), dtype=np.uint64)
        for g in range(groups):
            acc = np.zeros(2 * n, dtype=np.uint64)
            for i in range(count):
                pi, ci = np.ascontiguousarray(pts[g, i] % qq), np.ascontiguousarray(cts[g, i] % qq)
                if is_ntt:
                    fp = c.ref.forward(pi)
                    term = np.stack([oracle.pointwise(q, ci[j], fp) for j in range(2)])
                else:
                    term = np.stack([c.ref.polymul(ci[j], pi) for j in range(2)])
                acc = oracle.poly_add(q, acc, np.ascontiguousarray(term).ravel())
            exp[g] = acc.reshape(2, n)
            assert exp[g, 0].any() and exp[g, 1].any(), (g, is_ntt)
        _DOT_PLAIN[key] = (cts, pts, exp)
    return _DOT_PLAIN[key]


def check_dot_plain(c, monkeypatch, split, is_ntt):
    cts, pts, exp = dot_plain_operands(c, is_ntt)
    if split is None:
        monkeypatch.delenv("FHE_DOT_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_DOT_SPLIT", split)
    got = c.eng.dot_plain(cts, pts, is_ntt=is_ntt)
    assert (got == exp).all(), np.nonzero((got != exp).reshape(3, -1).any(axis=1))[0].tolist()


@every_degree
def test_fused_square(fg, n, name):
    check_square(Ctx(fg, n, name))


@every_degree
def test_fused_squared_difference(fg, n, name):
    check_squared_difference(Ctx(fg, n, name))


@fused
def test_fused_square_relin(fg, n, name):
    check_square_relin(fg, Ctx(fg, n, name))


@every_degree
def test_fused_partial_decrypt(fg, n, name):
    check_partial_decrypt(fg, Ctx(fg, n, name))


@every_degree
@pytest.mark.parametrize("split", [None, "2"])
@pytest.mark.parametrize("is_ntt", [False, True])
def test_fused_dot_plain(fg, monkeypatch, n, name, split, is_ntt):
    check_dot_plain(Ctx(fg, n, name), monkeypatch, split, is_ntt)


@composed
def test_composed_square(fg, n, q):
    c = Ctx(fg, n, q)
    check_square(c, few=True)
    check_squared_difference(c, few=True)


@pytest.mark.parametrize("n,q", COEFF_COMPOSED)
def test_composed_square_relin_and_partial_decrypt(fg, n, q):
    c = Ctx(fg, n, q)
    check_square_relin(fg, c, few=True)
    check_partial_decrypt(fg, c, few=True)


@composed
@pytest.mark.parametrize("split", [None, "2"])
def test_composed_dot_plain(fg, monkeypatch, n, q, split):
    c = Ctx(fg, n, q)
    for is_ntt in domains(q):
        check_dot_plain(c, monkeypatch, split, is_ntt)
