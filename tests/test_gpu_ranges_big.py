"""GPU parity of the two-pass degrees, N = 32768 and 65536 (ntt_big.hip), at
the modulus edges of tests/ntt_primes.py and on the rows that fill the
unreduced input windows.  The other suites run these degrees with the 27-bit
benchmark prime, which is past the lazy bound here (test_ntt_primes.py,
test_two_pass_degrees_premise), with a 62-bit prime or with wide moduli, and
on canonical or uniform u64 rows: the lazy row kernel
(k_big_fwd_rows<M, uint32_t, true>), the 32-bit modulus just under 2^30, the
first and the last modulus of the 64-bit lanes and the wrap prime run only
here, as do the in-window loads of the strided row kernels, of the inverse's
column kernel and of the w operand of the fused forward + modmul.

Compat mode bit-exact against the CPU oracle (oracle/ref_cpu.c), negacyclic
mode against the big-integer reference (oracle/pyref.py) through
test_gpu_negacyclic.py's own test body.  Wide moduli at these degrees are in
test_gpu_wide.py.

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import ntt_primes as P
import oracle
import test_gpu_negacyclic as neg
import test_gpu_ranges as ranges

pytestmark = pytest.mark.gpu

BIG_N = (32768, 65536)


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    neg._CACHE.clear()


# ------------------------------------------------------------ compat transforms vs the C oracle
@pytest.mark.parametrize("name", P.SWEEP_NAMES)
@pytest.mark.parametrize("n", BIG_N)
def test_window_rows_vs_oracle(fg, n, name):
    """test_gpu_ranges.check_window_rows with two tiles of the base rows and
    one row more: 37 rows in 32-bit lanes, 31 in 64-bit ones.  big_map pads
    the batch to 8 polynomials per XCD round, so the last round is partly
    filled."""
    q = P.sweep_primes(n)[name]
    assert P.word_bits(q) == (64 if name in ("u64_bottom", "u64_top") else 32)
    assert P.is_lazy(n, q) == (name == "lazy_top")
    rows = 2 * len(P.base_rows(n, q)[0]) + 1
    assert rows % 8 != 0
    ranges.check_window_rows(fg, n, q, tiles=2, ragged_for=8)


# ------------------------------------------------------------ XCD mapping and chunk loop
XCD_CASES = [(32768, "lazy_top"), (65536, "u64_bottom")]
# the rows a transform is most likely to break on come first, so that the
# batch of one is the top-of-window row
ROW_ORDER = ("const lim-1", "mixed one slow word per 16", "sparse alternating", "const 2^64-1", "mixed in-window",
             "const lim", "sparse last", "const q-1", "canonical")


def ordered_rows(n, q):
    names, base = P.base_rows(n, q)
    rest = [x for x in names if x not in ROW_ORDER]
    order = list(ROW_ORDER) + rest
    return order, base[[names.index(x) for x in order]]


@pytest.mark.parametrize("batch", [1, 7, 8, 9])
@pytest.mark.parametrize("n,name", XCD_CASES)
def test_xcd_rounds(fg, n, name, batch):
    """Batches below, at and above one XCD round of 8 polynomials: forward and
    multiply, every row against the oracle."""
    q = P.sweep_primes(n)[name]
    r = fg.PolynomialRing(n, q)
    t = oracle.NTT(n, q)
    order, base = ordered_rows(n, q)
    x = np.ascontiguousarray(P.tile_rows(base, batch)[:batch])
    y = np.ascontiguousarray(np.roll(x, 1, axis=0))  # (batch 1: the square of the top-of-window row)
    got, exp = r.forward_ntt(x), t.forward(x)
    assert (got == exp).all(), ("forward", ranges.bad_rows(got, exp, order))
    got, exp = r.multiply(x, y), t.polymul(x, y)
    assert exp.any() and (got == exp).all(), ("multiply", ranges.bad_rows(got, exp, order))


def test_chunk_boundary_lazy(fg):
    """One polynomial more than the scratch chunk (plan.big_chunk = 2^25 / N)
    at the lazy modulus: device tensors in, the rows on either side of the
    boundary, the first rows and the slow-word row nearest the middle against
    the oracle; w changes kind (canonical, q-1, raw q, raw 2^64-1) every row."""
    import torch

    n = 32768
    q = P.sweep_primes(n)["lazy_top"]
    chunk = (1 << 25) // n
    b = chunk + 1
    assert b == 1025 and P.is_lazy(n, q)
    r = fg.PolynomialRing(n, q)
    t = oracle.NTT(n, q)
    names, base = P.base_rows(n, q)
    x = P.tile_rows(base, b)
    w = P.weight_rows(n, q, b, 1)
    assert x.shape == w.shape == (b, n)
    slow = names.index("mixed one slow word per 16")
    mid = min((i for i in range(b) if i % len(names) == slow), key=lambda i: abs(i - b // 2))
    rows = [0, names.index("const lim-1"), mid, chunk - 1, chunk]
    live = ("const lim-1", "sparse alternating", "mixed in-window", "mixed one slow word per 16")
    for kind in set(range(4)) - {i % 4 for i in rows}:  # every kind of w meets a nonzero row
        rows.append(next(i for i in range(b) if i % 4 == kind and names[i % len(names)] in live))
    assert {i % 4 for i in rows} == {0, 1, 2, 3} and len(rows) <= 7
    dx = torch.from_numpy(x.view(np.int64)).cuda()
    dw = torch.from_numpy(w.view(np.int64)).cuda()
    f = r.forward_ntt(dx)
    fm = r.forward_ntt_mul(dx, dw)
    torch.cuda.synchronize()
    got_f = f[rows].cpu().numpy().view(np.uint64)
    got_fm = fm[rows].cpu().numpy().view(np.uint64)
    assert (dx.cpu().numpy().view(np.uint64) == x).all() and (dw.cpu().numpy().view(np.uint64) == w).all()
    del dx, dw, f, fm
    torch.cuda.empty_cache()
    xs, ws = np.ascontiguousarray(x[rows]), np.ascontiguousarray(w[rows])
    exp_f, exp_fm = t.forward(xs), t.fwd_mul(xs, ws)
    assert (got_f == exp_f).all(), ("forward", [rows[i] for i in np.nonzero((got_f != exp_f).any(axis=1))[0]])
    assert (got_fm == exp_fm).all(), ("forward_ntt_mul", [rows[i] for i in np.nonzero((got_fm != exp_fm).any(axis=1))[0]])


# ------------------------------------------------------------ negacyclic vs oracle.pyref
NEG_OPS = ("forward", "inverse", "multiply rolled", "forward_ntt_mul")


@pytest.mark.parametrize("op", NEG_OPS)
@pytest.mark.parametrize("name", ["lazy_top", "nonlazy_bottom", "u64_bottom", "u64_top"])
@pytest.mark.parametrize("n", BIG_N)
def test_negacyclic_vs_pyref(fg, n, name, op):
    """test_gpu_negacyclic.test_transforms_vs_pyref's body on the two rows it
    picks above n = 16384: every word at the top of the window, and one slow
    word per 16 among in-window ones."""
    assert neg.operand_rows(n, P.sweep_primes(n)[name], op == "inverse", 1)[1].shape == (2, n)
    neg.test_transforms_vs_pyref(fg, n, name, op)


# ------------------------------------------------------------ composed ciphertext paths
def few_cts(c, comps):
    """Two ciphertexts of `comps` components from the two rows of
    test_gpu_ranges.cut(c, few=True): each row in every position."""
    two = ranges.cut(c, few=True)
    if comps == 2:
        return two
    top, slow = two[0]
    return np.ascontiguousarray(np.stack([np.stack([top, slow, top]), np.stack([slow, top, slow])]))


big_composed = pytest.mark.parametrize("n,q", ranges.BIG_COMPOSED)


@big_composed
def test_composed_ct_multiply(fg, n, q):
    c = ranges.Ctx(fg, n, q)
    x = few_cts(c, 2)
    ranges.check_ct_multiply(c, x, (np.ascontiguousarray(x[::-1]), x))


@big_composed
def test_composed_relinearize(fg, n, q):
    c = ranges.Ctx(fg, n, q)
    ranges.check_relinearize(fg, c, few_cts(c, 3))


@big_composed
@pytest.mark.parametrize("comps", [2, 3])
def test_composed_decrypt(fg, n, q, comps):
    c = ranges.Ctx(fg, n, q)
    ranges.check_decrypt(fg, c, few_cts(c, comps))
