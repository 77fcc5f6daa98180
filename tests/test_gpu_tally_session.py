"""The context's tally buffers shared by the four reduction families
(fhe_ct_sum_ptrs, fhe_ct_dot_ptrs, fhe_ct_sum_scaled_ptrs,
fhe_ct_dot_plain_ptrs): the pointer table with its pinned upload buffer and
the partial rows belong to the context, not to a family.  The per-family tests
synchronise between calls and stay within one family; here calls of all four
are enqueued back to back, so that the buffers grow and are refilled while
earlier work is still queued, and calls on two streams hand the buffers over.

Expected values: the sequential oracle folds of the per-family tests
(poly_add over the ballots, over ct_multiply, poly_mul_scalar and polymul).
Only the result words are asserted: a passing run does not prove the stream
ordering correct.

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

from test_gpu_dot import fold as fold_dot
from test_gpu_dot import pairs as dot_pairs
from test_gpu_dot_plain import fold as fold_dot_plain
from test_gpu_dot_plain import pairs as plain_pairs
from test_gpu_sum_scaled import ballots as scaled_ballots
from test_gpu_sum_scaled import fold as fold_scaled
from test_gpu_tally import ballots, fold as fold_sum

pytestmark = pytest.mark.gpu

P62 = 4611686018326724609


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


def W(t):
    """The words of a device tensor (the caller has synchronised)."""
    return t.cpu().numpy().view(np.uint64)


def bufs(a):
    """Every ciphertext (or plaintext) of group 0 in its own allocation."""
    return [D(a[0, i]) for i in range(a.shape[1])]


@pytest.mark.parametrize("n,q", [(16, 97), (1024, P62)])
def test_buffers_shared_across_families(fg, n, q, monkeypatch):
    """Six calls of four families with no host synchronisation between them.
    The table and its pinned twin grow at calls 2 and 5, the partial rows grow
    at call 2 and are reused at a smaller size afterwards; with both splits
    forced to 2 every call goes through the partial rows."""
    import torch

    monkeypatch.setenv("FHE_TALLY_SPLIT", "2")
    monkeypatch.setenv("FHE_DOT_SPLIT", "2")
    monkeypatch.delenv("FHE_DOT_COMPONENTS", raising=False)
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    s3 = ballots(1, q, 1, 3, 2, n)
    a33, b33 = dot_pairs(2, q, 1, 33, n)
    c7, w7 = scaled_ballots(3, q, 1, 7, 2, n)
    c64, p64 = plain_pairs(4, q, 1, 64, n)
    s257 = ballots(5, q, 1, 257, 2, n)
    a3, b3 = dot_pairs(6, q, 1, 3, n)
    want = [fold_sum(q, s3)[0], fold_dot(q, n, a33, b33)[0], fold_scaled(q, c7, w7)[0],
            fold_dot_plain(q, n, c64, p64)[0], fold_sum(q, s257)[0], fold_dot(q, n, a3, b3)[0]]
    dev = [bufs(x) for x in (s3, a33, b33, c7, c64, p64, s257, a3, b3)]
    d_s3, d_a33, d_b33, d_c7, d_c64, d_p64, d_s257, d_a3, d_b3 = dev
    torch.cuda.synchronize()
    got = [ring.sum_buffers(d_s3),
           eng.dot_buffers(d_a33, d_b33),
           ring.sum_scaled_buffers(d_c7, [int(x) for x in w7[0]]),
           eng.dot_plain_buffers(d_c64, d_p64),
           ring.sum_buffers(d_s257),
           eng.dot_buffers(d_a3, d_b3)]
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert W(g).shape == w.shape, i
        assert (W(g) == w).all(), i


def test_another_stream(fg, monkeypatch):
    """Calls on a side stream, then at once on the default stream, then on the
    side stream again: each hand-over waits for the other stream's last use of
    the buffers, and a buffer is regrown only once that use has completed.
    One device synchronisation at the end."""
    import torch

    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    monkeypatch.delenv("FHE_DOT_SPLIT", raising=False)
    monkeypatch.delenv("FHE_DOT_COMPONENTS", raising=False)
    n, q = 1024, P62
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    s64 = ballots(11, q, 1, 64, 2, n)
    a7, b7 = dot_pairs(12, q, 1, 7, n)
    s7 = ballots(13, q, 1, 7, 2, n)
    c7, p7 = plain_pairs(14, q, 1, 7, n)
    s3 = ballots(15, q, 1, 3, 2, n)
    want = [fold_sum(q, s64)[0], fold_dot(q, n, a7, b7)[0], fold_sum(q, s7)[0], fold_dot_plain(q, n, c7, p7)[0],
            fold_sum(q, s3)[0]]
    d_s64, d_a7, d_b7, d_s7, d_c7, d_p7, d_s3 = [bufs(x) for x in (s64, a7, b7, s7, c7, p7, s3)]
    out = [torch.empty((polys, n), dtype=torch.int64, device="cuda:0") for polys in (2, 3, 2, 2, 2)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ring.sum_buffers(d_s64, out=out[0])
        eng.dot_buffers(d_a7, d_b7, out=out[1])
    ring.sum_buffers(d_s7, out=out[2])
    eng.dot_plain_buffers(d_c7, d_p7, out=out[3])
    with torch.cuda.stream(side):
        ring.sum_buffers(d_s3, out=out[4])
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(out, want)):
        assert (W(g) == w).all(), i
