"""The Galois key switch and the trace at the edges of the range analysis
(k_dmac MODE 4 of ntt_ext.hip, galois.hip, fhe_ct_galois_batch /
fhe_ct_trace_batch / fhe_poly_galois_batch), word for word against the header
formula restated in tests/galois_ref.py over ring products that do not use
the library: the CPU oracle's transforms in compat mode, one big-integer
product per row (oracle/pyref.py) in negacyclic mode.

MODE 4 changes both ends of k_dmac -- the digit load gathers sigma_g(c1), the
store epilogue adds sigma_g(c0) (+ c0) and (c1 | 0) -- in three accumulator
layouts, the 32-bit key-prefetch variant and lazy and non-lazy transforms:
the sweep of test_gpu_ranges.py's test_fused_relinearize (every fused degree
class, the primes on either side of each threshold) with operands cut from the
rows that fill the unreduced input window, every row once as c0 and once as
c1, and the first key row all q - 1.  The composed path (q >= 2^62) runs at
the primes around 2^62 and 2^63 and at the last prime of the word, against
exact products and not only against the chain that shares its code.

Run on an MI355X with ``pytest -m gpu``."""
import numpy as np
import pytest

import galois_ref as R
import ntt_primes as P
import oracle
import range_inputs as I
from oracle import pyref
from test_gpu_ranges import FUSED_N, FUSED_PRIMES, Ctx, digits

pytestmark = pytest.mark.gpu


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


def compat_mul(n, q):
    ref = oracle.NTT(n, q)
    return lambda a, b: ref.polymul(np.ascontiguousarray(a), np.ascontiguousarray(b))


def nega_mul(q):
    def mul(a, b):
        return np.array([pyref.negacyclic_multiply(x.tolist(), y.tolist(), q) for x, y in zip(a, b)], dtype=np.uint64)

    return mul


def decomposition(q):
    lv = 3 if q < 1 << 30 else 4
    return digits(q, lv), lv


def operands(c, shift, bl):
    """The rows as ciphertexts and the two digit-edge ciphertexts; the names of
    the rows behind each ciphertext, for the messages."""
    ct = np.concatenate([I.galois_operands(c, shift), I.galois_digit_edges(c.n, c.q, bl)])
    rows = I.operand_rows(c, shift) + [("const q-1", "digits all ones"), ("const q-1", "digits 0")]
    return np.ascontiguousarray(ct), rows


def bad_rows(got, want, rows):
    return [rows[i] for i in np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]]


def sweep(fg, c, ring, mode, mul, combos, split=False):
    """apply_galois over both shifts and every (g, add_input) of combos;
    split: combo i at shift i only."""
    q = c.q
    bl, lv = decomposition(q)
    key = c.keys(31, lv, 2)
    assert (key[0, 0] == np.uint64(q - 1)).all()
    eng = fg.EncryptionEngine(ring)
    sk = fg.SwitchKey(ring, D(key), bl, lv)
    for shift in (0, 1):
        ct, rows = operands(c, shift, bl)
        dct = D(ct)
        for g, add_input in combos[shift:shift + 1] if split else combos:
            sk.g = g
            got = H(eng.apply_galois(dct, sk, bool(add_input)))
            want = R.ct_galois(q, bl, lv, g, key, ct, add_input, mul)
            assert (got == want).all(), (c.n, q, mode, shift, g, add_input, bad_rows(got, want, rows))
        assert (H(dct) == ct).all(), "the input is not written"


# ------------------------------------------------------------ the fused kernel
@pytest.mark.parametrize("n,name", [(n, p) for n in FUSED_N for p in FUSED_PRIMES])
def test_fused_galois(fg, n, name):
    c = Ctx(fg, n, name)
    if n <= 1024:
        combos = [(g, a) for g in (3, n + 1, 2 * n - 1) for a in (0, 1)]
    else:  # the exact products are the cost
        combos = [(3, 1), (2 * n - 1, 0)]
    # n = 16384: one combination per shift (every row is still a c0 and a c1 once), which keeps the
    # test below the slowest one of test_gpu_ranges.py
    sweep(fg, c, c.ring, "compat", compat_mul(n, c.q), combos, split=n > 4096)


@pytest.mark.parametrize("n,name", [(n, p) for n in (16, 256) for p in FUSED_PRIMES])
def test_fused_galois_negacyclic(fg, n, name):
    c = I.Rows(n, P.sweep_primes(n)[name])
    c.keys = lambda seed, *lead: Ctx.keys(c, seed, *lead)
    ring = fg.PolynomialRing(n, c.q, mode="negacyclic")
    combos = [(g, a) for g in (3, n + 1, 2 * n - 1) for a in (0, 1)]
    sweep(fg, c, ring, "negacyclic", nega_mul(c.q), combos)


@pytest.mark.parametrize("n,name", [(n, p) for n in (16, 1024) for p in FUSED_PRIMES])
def test_fused_trace(fg, n, name):
    c = Ctx(fg, n, name)
    q, steps = c.q, 2
    bl, lv = decomposition(q)
    keys = c.keys(37, steps, lv, 2)
    mul = compat_mul(n, q)
    gk = fg.SwitchKey(c.ring, D(keys), bl, lv, R.trace_elements(n, steps))
    for shift in (0, 1):
        ct, rows = operands(c, shift, bl)
        dct = D(ct)
        got = H(c.eng.trace(dct, gk))
        want = R.trace(q, bl, lv, steps, keys, ct, mul)
        assert (got == want).all(), (n, q, shift, bad_rows(got, want, rows))
        assert (H(dct) == ct).all()


# ------------------------------------------------------------ decomposition edges
def test_galois_decomposition_edges(fg):
    """(base_log, level) at both ends: one bit per digit, one 63-bit digit, the
    32-bit digit boundary, and a decomposition that truncates (8 x 4 < 62 bits)."""
    n = 16
    q = P.stream_primes(n)["u64_top"]
    c = I.Rows(n, q)
    ring = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(ring)
    for bl, lv in [(1, 62), (63, 1), (63, 2), (32, 2), (31, 2), (8, 4)]:
        assert (lv - 1) * bl < 64
        key = Ctx.keys(c, 41 + bl, lv, 2)
        sk = fg.SwitchKey(ring, D(key), bl, lv)
        few = lv > 8  # the integer reference costs level n^2 per ciphertext
        for shift in (0,) if few else (0, 1):
            ct, rows = operands(c, shift, bl)
            for g, add_input in ((3, 1), (2 * n - 1, 0)) if few else ((3, 1), (2 * n - 1, 0), (n + 1, 1)):
                sk.g = g
                got = H(eng.apply_galois(D(ct), sk, bool(add_input)))
                want = np.array([R.ct_galois_int(q, bl, lv, g, key.tolist(), x.tolist(), add_input, R.negacyclic_schoolbook)
                                 for x in ct], dtype=np.uint64)
                assert (got == want).all(), (bl, lv, shift, g, add_input, bad_rows(got, want, rows))
    # rejected decompositions: code -9 and nothing written
    ct, _ = operands(c, 0, 16)
    for bl, lv in [(32, 3), (63, 3), (1, 65), (16, 5), (0, 2), (64, 1), (64, 2)]:
        key = Ctx.keys(c, 43, lv, 2)
        sk = fg.SwitchKey(ring, D(key), bl, lv, 3)
        out = D(np.full(ct.shape, 7, dtype=np.uint64))
        with pytest.raises(fg.FHEError) as e:
            eng.apply_galois(D(ct), sk, True, out=out)
        assert e.value.code == -9 and "invalid decomposition" in str(e.value), (bl, lv)
        assert (H(out) == 7).all(), (bl, lv)


# ------------------------------------------------------------ the composed path
@pytest.mark.parametrize("mode", ["compat", "negacyclic"])
@pytest.mark.parametrize("name", ["wide_bottom", "shoup_top", "wmont_bottom", "u64_max"])
def test_composed_galois_wide_moduli(fg, name, mode):
    n = 256
    q = P.stream_primes(n)[name]
    assert q >> 62
    c = I.Rows(n, q)
    bl, lv = 16, 4
    key = Ctx.keys(c, 47, lv, 2)
    ring = fg.PolynomialRing(n, q, mode=mode)
    assert ring.info.word_bits == 64
    eng = fg.EncryptionEngine(ring)
    mul = compat_mul(n, q) if mode == "compat" else nega_mul(q)
    sk = fg.SwitchKey(ring, D(key), bl, lv)
    for shift in (0, 1):
        ct, rows = operands(c, shift, bl)
        # the window is q here: every word of the streaming edge list, in c0 and in c1
        ct = np.concatenate([ct, I.plant_words(ct[-1:], P.stream_words(q))])
        rows = rows + [("stream words", "stream words")]
        dct = D(ct)
        for g, add_input in ((3, 1), (n + 1, 0), (2 * n - 1, 1)):
            sk.g = g
            got = H(eng.apply_galois(dct, sk, bool(add_input)))
            want = R.ct_galois(q, bl, lv, g, key, ct, add_input, mul)
            assert (got == want).all(), (name, mode, shift, g, add_input, bad_rows(got, want, rows))
        assert (H(dct) == ct).all()


# ------------------------------------------------------------ sigma_g alone
@pytest.mark.parametrize("name", P.STREAM_NAMES)
def test_poly_galois_stream_edges(fg, name):
    """Every odd g at n = 16; a lane owns two adjacent words, so every edge
    word sits at an even and at an odd index."""
    n = 16
    q = P.stream_primes(n)[name]
    W = P.stream_words(q)
    m = len(W)
    rows = np.array([[W[(i + r) % m] for i in range(n)] for r in range(m + 1)], dtype=np.uint64)
    for w in W:
        at = np.nonzero(rows == np.uint64(w))[1]
        assert (at % 2 == 0).any() and (at % 2 == 1).any()
    ring = fg.PolynomialRing(n, q)
    drows = D(rows)
    for g in range(1, 2 * n, 2):
        got = H(ring.galois(drows, g))
        want = np.array([R.sigma_int(row.tolist(), g, q) for row in rows], dtype=np.uint64)
        assert (got == want).all(), (name, g, np.nonzero((got != want).any(axis=1))[0].tolist())
    assert (H(drows) == rows).all()
