"""GPU parity of the scaled ciphertext sum (csrc/tally.hip k_ct_sum_scaled,
fhe_ct_sum_scaled_batch / fhe_ct_sum_scaled_ptrs):
out = sum_i multiply_scalar(ct_i, s_i) folded by add().

Expected value: the sequential oracle.poly_add fold of
oracle.poly_mul_scalar(q, ct_i % q, s_i % q).  In every case the result is
also compared bit for bit with the device chain that existed before:
ring.multiply_scalar per ballot, then sum_batch.

Run on an MI355X with ``pytest -m gpu``.
"""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
QG = 18446744069414584321     # 2^64 - 2^32 + 1 > 2^63: the product's intermediate carries
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


def set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_TALLY_SPLIT", split)


def ballots(seed, q, groups, count, polys, n):
    """cts [groups, count, polys, n] of full-range u64 words with the edge
    words planted in the first and the last ballot; scalars [groups, count]
    with the edge scalars planted (as many as fit) and otherwise random."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    a = rng.integers(0, 1 << 64, size=(groups, count, polys, n), dtype=np.uint64)
    a[:, 0, 0, :4] = edge
    a[:, -1, -1, -4:] = edge[::-1]
    s = rng.integers(0, 1 << 64, size=(groups, count), dtype=np.uint64)
    es = np.array([0, 1, q - 1, q, M64], dtype=np.uint64)
    for g in range(groups):  # rotate so that small counts see every edge scalar across the groups
        k = min(count, len(es))
        s[g, :k] = np.roll(es, -g)[:k]
    return a, s


def prior_words(seed, q, groups, polys, n):
    p = np.random.default_rng(seed).integers(0, 1 << 64, size=(groups, polys, n), dtype=np.uint64)
    p[:, 0, :4] = np.array([0, q - 1, q, M64], dtype=np.uint64)
    return p


def fold(q, a, s, prior=None):
    """Sequential poly_add fold of the oracle's poly_mul_scalar over the ballots."""
    qq = np.uint64(q)
    groups, count, polys, n = a.shape
    out = np.empty((groups, polys, n), dtype=np.uint64)
    for g in range(groups):
        acc = np.zeros(polys * n, dtype=np.uint64)
        if prior is not None:
            acc = oracle.poly_add(q, acc, np.ascontiguousarray(prior[g]).ravel())
        for i in range(count):
            term = oracle.poly_mul_scalar(q, np.ascontiguousarray(a[g, i].ravel() % qq), int(s[g, i]) % q)
            acc = oracle.poly_add(q, acc, term)
        out[g] = acc.reshape(polys, n)
    return out


def chain(ring, da, s, prior=None):
    """The pre-existing entry points: multiply_scalar per ballot, then one tally."""
    import torch

    groups, count = da.shape[:2]
    prod = torch.empty_like(da)
    for g in range(groups):
        for i in range(count):
            ring.multiply_scalar(da[g, i], int(s[g, i]), out=prod[g, i])
    if prior is None:
        return H(ring.sum_batch(prod, grouped=True))
    out = D(prior.copy())
    ring.sum_batch(prod, out=out, accumulate=True, grouped=True)
    return H(out)


COUNTS = [1, 2, 7, 8, 9, 33]          # around kUnroll = 8
SPLITS = [None, "1", "2", "5", "1000"]


@pytest.mark.parametrize("polys", [1, 2, 3])
def test_small_ring_every_count_and_split(fg, polys, monkeypatch):
    """n = 4, q = 17: every count around the unroll boundary, one and three
    groups, every forced split (1000 is clamped to count), with and without a
    raw-u64 prior `out`, device and host resident."""
    n, q = 4, 17
    ring = fg.PolynomialRing(n, q)
    for count in COUNTS:
        for groups in (1, 3):
            a, s = ballots(100 * count + groups, q, groups, count, polys, n)
            prior = prior_words(7, q, groups, polys, n)
            da, ds = D(a), D(s)
            set_split(monkeypatch, None)
            exp, exp_acc = fold(q, a, s), fold(q, a, s, prior)
            assert (chain(ring, da, s) == exp).all(), (count, groups)
            assert (chain(ring, da, s, prior) == exp_acc).all(), (count, groups)
            for split in SPLITS:
                set_split(monkeypatch, split)
                got = H(ring.sum_scaled(da, ds, grouped=True))
                assert got.shape == (groups, polys, n)
                assert (got == exp).all(), (count, groups, split)
                out = D(prior.copy())
                ring.sum_scaled(da, ds, out=out, accumulate=True, grouped=True)
                assert (H(out) == exp_acc).all(), (count, groups, split)
                if split in (None, "2"):  # FHE_HOST
                    assert (ring.sum_scaled(a, s, grouped=True) == exp).all(), (count, groups, split)
                    hout = prior.copy()
                    ring.sum_scaled(a, s, out=hout, accumulate=True, grouped=True)
                    assert (hout == exp_acc).all(), (count, groups, split)


@pytest.mark.parametrize("q", [P27, P62, QG])
def test_every_modulus_width_and_pointer_tables(fg, q, monkeypatch):
    """n = 1024, count 33: q < 2^32, q < 2^62 and q > 2^63 (the carry case),
    contiguous and pointer tables in reversed order with one buffer listed
    twice under different scalars."""
    n, count, groups, polys = 1024, 33, 2, 2
    ring = fg.PolynomialRing(n, q)
    a, s = ballots(q % 1000, q, groups, count, polys, n)
    prior = prior_words(9, q, groups, polys, n)
    da, ds = D(a), D(s)
    exp = fold(q, a, s)
    set_split(monkeypatch, None)
    assert (chain(ring, da, s) == exp).all()
    for split in (None, "1", "5"):
        set_split(monkeypatch, split)
        assert (H(ring.sum_scaled(da, ds, grouped=True)) == exp).all(), split
        assert (ring.sum_scaled(a, s, grouped=True) == exp).all(), split
        order = list(reversed(range(count))) + [count // 2]
        bufs = [D(a[0, i]) for i in range(count)]
        tab = [bufs[i] for i in order]
        sc = [int(s[0, i]) for i in order[:-1]] + [int(s[1, 0])]  # the repeated buffer under another scalar
        terms = np.stack([a[0, i] for i in order])[None]
        want = fold(q, terms, np.array([sc], dtype=np.uint64))[0]
        assert (H(ring.sum_scaled_buffers(tab, sc)) == want).all(), split
        pout = D(prior[0].copy())
        ring.sum_scaled_buffers(tab, sc, out=pout, accumulate=True)
        assert (H(pout) == fold(q, terms, np.array([sc], dtype=np.uint64), prior[:1])[0]).all(), split


def test_degree_above_the_fused_family(fg, monkeypatch):
    set_split(monkeypatch, None)
    n, q = 32768, P27
    ring = fg.PolynomialRing(n, q)
    a, s = ballots(5, q, 1, 3, 2, n)
    exp = fold(q, a, s)
    da = D(a)
    got = H(ring.sum_scaled(da, D(s), grouped=True))
    assert (got == exp).all()
    assert (got == chain(ring, da, s)).all()


def test_multi_device_context_splits_groups(fg, monkeypatch):
    set_split(monkeypatch, None)
    n, q = 4, 17
    ring = fg.PolynomialRing(n, q, devices=[0, 0])
    a, s = ballots(11, q, 3, 9, 2, n)
    exp = fold(q, a, s)
    assert (ring.sum_scaled(a, s, grouped=True) == exp).all()        # FHE_HOST: the groups are split
    assert (H(ring.sum_scaled(D(a), D(s), grouped=True)) == exp).all()
    bufs = [D(a[1, i]) for i in range(9)]
    assert (H(ring.sum_scaled_buffers(bufs, [int(x) for x in s[1]])) == exp[1]).all()


def test_engine_tally_scalar_weighted(fg, monkeypatch):
    set_split(monkeypatch, None)
    n, q = 1024, P27
    eng = fg.EncryptionEngine(fg.PolynomialRing(n, q))
    a, s = ballots(3, q, 1, 7, 2, n)
    exp = fold(q, a, s)[0]
    w = [int(x) for x in s[0]]
    assert (H(eng.tally_scalar_weighted(D(a[0]), w)) == exp).all()
    assert (H(eng.tally_scalar_weighted([D(a[0, i]) for i in range(7)], w)) == exp).all()
    assert (eng.tally_scalar_weighted(a[0], w) == exp).all()
    with pytest.raises(fg.FHEError, match="Ballots and weights must have the same size"):
        eng.tally_scalar_weighted(D(a[0]), w[:-1])
    with pytest.raises(fg.FHEError, match="Cannot add empty vector of ciphertexts"):
        eng.tally_scalar_weighted([], [])


def test_errors(fg):
    import torch

    n, q = 4, 17
    ring = fg.PolynomialRing(n, q)
    L = fg.lib()
    a, s = ballots(1, q, 1, 4, 2, n)
    da, ds = D(a), D(s)
    out = torch.empty((2, n), dtype=torch.int64, device="cuda:0")
    pa, ps, po = da.data_ptr(), ds.data_ptr(), out.data_ptr()
    dev = fg.FHE_DEVICE

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return L.fhe_last_error().decode()

    empty = "Cannot add empty vector of ciphertexts"
    assert err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 2, 0, 1, 0, po, dev)) == empty
    assert err(L.fhe_ct_sum_scaled_batch(ring._h, None, ps, 2, 4, 1, 0, po, dev)) == "null buffer"
    assert err(L.fhe_ct_sum_scaled_batch(ring._h, pa, None, 2, 4, 1, 0, po, dev)) == "null buffer"
    assert err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 2, 4, 1, 0, None, dev)) == "null buffer"
    err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 2, 4, 1, 0, po, 7))
    err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 0, 4, 1, 0, po, dev))
    err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 4, 4, 1, 0, po, dev))
    assert "16-byte aligned" in err(L.fhe_ct_sum_scaled_batch(ring._h, pa + 8, ps, 2, 3, 1, 0, po, dev))
    assert "16-byte aligned" in err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 2, 4, 1, 0, po + 8, dev))
    assert "overlap" in err(L.fhe_ct_sum_scaled_batch(ring._h, pa, ps, 2, 4, 1, 0, pa + 8 * 2 * n * 3, dev))
    tab = (C.c_void_p * 4)(*[pa + 8 * 2 * n * i for i in range(4)])
    hs = (C.c_uint64 * 4)(1, 2, 3, 4)
    assert err(L.fhe_ct_sum_scaled_ptrs(ring._h, tab, hs, 2, 0, 0, po)) == empty
    assert err(L.fhe_ct_sum_scaled_ptrs(ring._h, None, hs, 2, 4, 0, po)) == "null buffer"
    assert err(L.fhe_ct_sum_scaled_ptrs(ring._h, tab, None, 2, 4, 0, po)) == "null buffer"
    assert err(L.fhe_ct_sum_scaled_ptrs(ring._h, tab, hs, 2, 4, 0, None)) == "null buffer"
    err(L.fhe_ct_sum_scaled_ptrs(ring._h, tab, hs, 0, 4, 0, po))
    err(L.fhe_ct_sum_scaled_ptrs(ring._h, tab, hs, 4, 4, 0, po))
    hole = (C.c_void_p * 4)(pa, None, pa, pa)
    assert err(L.fhe_ct_sum_scaled_ptrs(ring._h, hole, hs, 2, 4, 0, po)) == "null buffer"
    bad = (C.c_void_p * 4)(pa, pa + 8, pa, pa)  # entry 1 is 8-byte aligned only
    assert "16-byte aligned" in err(L.fhe_ct_sum_scaled_ptrs(ring._h, bad, hs, 2, 4, 0, po))
    assert "overlap" in err(L.fhe_ct_sum_scaled_ptrs(ring._h, tab, hs, 2, 4, 0, pa + 8 * 2 * n))
    with pytest.raises(fg.FHEError, match=empty):
        ring.sum_scaled_buffers([], [])
    with pytest.raises(fg.FHEError, match="Ballots and weights must have the same size"):
        ring.sum_scaled_buffers([da[0, 0], da[0, 1]], [1])
    # the failed calls enqueued nothing: a good call still works
    assert (H(ring.sum_scaled(da, ds, grouped=True)) == fold(q, a, s)).all()
