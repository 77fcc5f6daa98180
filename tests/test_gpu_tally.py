"""GPU parity of the single-launch ciphertext tally (csrc/tally.hip,
fhe_ct_sum_batch / fhe_ct_sum_ptrs): the sum of many ciphertexts against a
sequential fold of the oracle's poly_add over the ballots (the reference's
batch_add, encryption.cpp:1327-1364), bit-exact, plus sum(x % q) % q in Python
integers on a handful of columns as an independent check.

Run on an MI355X with ``pytest -m gpu``.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
Q63 = 9223370937344327681     # just below 2^63
QG = 18446744069414584321     # 2^64 - 2^32 + 1 (above 2^63: sums carry out of 64 bits)
M64 = (1 << 64) - 1
SMALL = [(4, 17), (16, 97)]
MID = [(1024, P27), (1024, P62), (1024, Q63), (1024, QG)]
COUNTS = [1, 2, 3, 7, 64, 257]
SPLITS = [None, "1", "2", "5"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def ballots(seed, q, groups, count, polys, n):
    """Full-range random u64 words with the edge words planted in the first
    and the last ballot of every group."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(groups, count, polys, n), dtype=np.uint64)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    a[:, 0, 0, :4] = edge
    a[:, -1, -1, -4:] = edge[::-1]
    return a


def fold(q, a, prior=None):
    """Sequential poly_add fold of a [groups, count, ...] over the ballots."""
    groups, count = a.shape[:2]
    out = np.empty((groups,) + a.shape[2:], dtype=np.uint64)
    for g in range(groups):
        acc = np.zeros(a[g, 0].size, dtype=np.uint64)
        if prior is not None:
            acc = oracle.poly_add(q, acc, np.ascontiguousarray(prior[g]).ravel())
        for i in range(count):
            acc = oracle.poly_add(q, acc, np.ascontiguousarray(a[g, i]).ravel())
        out[g] = acc.reshape(a.shape[2:])
    return out


def check_columns(q, a, got, prior=None):
    """sum(int(x) % q) % q on a few columns, in Python integers."""
    groups, count = a.shape[:2]
    fa, fo = a.reshape(groups, count, -1), got.reshape(groups, -1)
    fp = None if prior is None else prior.reshape(groups, -1)
    words = fa.shape[2]
    for g in range(groups):
        for w in {0, 1, 2, 3, words // 2, words - 2, words - 1}:
            want = sum(int(x) % q for x in fa[g, :, w]) + (0 if fp is None else int(fp[g, w]) % q)
            assert int(fo[g, w]) == want % q, (g, w)


def check(fg, ring, q, a, seed_note=""):
    exp = fold(q, a)
    got = H(ring.sum_batch(D(a), grouped=True))
    assert got.shape == exp.shape
    assert (got == exp).all(), seed_note
    check_columns(q, a, got)
    return exp


@pytest.mark.parametrize("n,q", SMALL)
def test_sum_smallest_sizes_full_sweep(fg, n, q, monkeypatch):
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    ring = fg.PolynomialRing(n, q)
    for polys in (1, 2, 3):
        for count in COUNTS:
            for groups in (1, 3):
                a = ballots(1000 * polys + 10 * count + groups, q, groups, count, polys, n)
                exp = check(fg, ring, q, a, (polys, count, groups))
                if count in (1, 7, 257):  # host-resident ballots
                    assert (ring.sum_batch(a, grouped=True) == exp).all(), (polys, count, groups)


# every polys, count and groups value at n = 1024
MID_SHAPES = [(1, 1, 3), (2, 2, 1), (3, 3, 3), (1, 7, 1), (2, 64, 3), (3, 257, 1), (2, 257, 3)]


@pytest.mark.parametrize("n,q", MID)
def test_sum_1024(fg, n, q, monkeypatch):
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    ring = fg.PolynomialRing(n, q)
    for polys, count, groups in MID_SHAPES:
        check(fg, ring, q, ballots(7 * count + polys + groups, q, groups, count, polys, n), (polys, count, groups))


@pytest.mark.parametrize("polys,count,groups", [(2, 64, 1), (3, 7, 3), (1, 257, 1)])
def test_sum_16384_natural_split(fg, polys, count, groups, monkeypatch):
    """One group at N = 16384 is 64 workgroups: with the switch unset the split
    rule cuts 64 ballots into slices.  Only the result is asserted."""
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    ring = fg.PolynomialRing(16384, P27)
    check(fg, ring, P27, ballots(count, P27, groups, count, polys, 16384))


@pytest.mark.parametrize("polys,groups", [(2, 1), (3, 3)])
def test_sum_65536(fg, polys, groups, monkeypatch):
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    ring = fg.PolynomialRing(65536, P27)
    check(fg, ring, P27, ballots(65, P27, groups, 3, polys, 65536))


@pytest.mark.parametrize("split", SPLITS)
def test_every_word_q_minus_1_at_qg(fg, split, monkeypatch):
    """257 terms of q - 1 at q > 2^63: every addition carries out of 64 bits."""
    if split is None:
        monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_TALLY_SPLIT", split)
    n, count = 1024, 257
    ring = fg.PolynomialRing(n, QG)
    a = np.full((1, count, 2, n), QG - 1, dtype=np.uint64)
    got = H(ring.sum_batch(D(a), grouped=True))
    assert (got == np.uint64(count * (QG - 1) % QG)).all()
    assert (got == fold(QG, a)).all()


@pytest.mark.parametrize("n,q", [(16, 97)] + MID)
def test_every_word_all_ones(fg, n, q, monkeypatch):
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    ring = fg.PolynomialRing(n, q)
    for count in (1, 64, 257):
        a = np.full((1, count, 3, n), M64, dtype=np.uint64)
        got = H(ring.sum_batch(D(a), grouped=True))
        assert (got == np.uint64(count * (M64 % q) % q)).all(), count
        assert (got == fold(q, a)).all(), count


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("count", [7, 257])
def test_forced_split_paths(fg, split, count, monkeypatch):
    """FHE_TALLY_SPLIT forces the slices (5 is clamped to ceil-sized slices of
    7 ballots): one-launch and two-launch paths, both addressing forms."""
    import torch

    if split is None:
        monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_TALLY_SPLIT", split)
    for n, q in [(16, 97), (1024, P27), (1024, QG)]:
        ring = fg.PolynomialRing(n, q)
        for groups in (1, 3):
            a = ballots(count + groups, q, groups, count, 2, n)
            exp = check(fg, ring, q, a, (n, q, groups))
        bufs = [D(a[0, i]) for i in range(count)]
        got = H(ring.sum_buffers(bufs))
        assert (got == exp[0]).all(), (n, q)
        del bufs
    torch.cuda.synchronize()


@pytest.mark.parametrize("split", [None, "2"])
@pytest.mark.parametrize("n,q", [(16, 97), (1024, P62), (1024, QG)])
def test_accumulate(fg, n, q, split, monkeypatch):
    """accumulate: the prior `out` (raw words) is one more term of the fold."""
    if split is None:
        monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_TALLY_SPLIT", split)
    ring = fg.PolynomialRing(n, q)
    for count, groups in [(1, 1), (7, 3), (64, 1)]:
        a = ballots(count, q, groups, count, 2, n)
        prior = ballots(99, q, groups, 1, 2, n)[:, 0]
        exp = fold(q, a, prior)
        out = D(prior.copy())
        ring.sum_batch(D(a), out=out, accumulate=True, grouped=True)
        got = H(out)
        assert (got == exp).all(), (count, groups)
        check_columns(q, a, got, prior)
        hout = prior.copy()
        ring.sum_batch(a, out=hout, accumulate=True, grouped=True)
        assert (hout == exp).all(), (count, groups)
        bufs = [D(a[0, i]) for i in range(count)]
        pout = D(prior[0].copy())
        ring.sum_buffers(bufs, out=pout, accumulate=True)
        assert (H(pout) == exp[0]).all(), (count, groups)


def test_host_chunks_over_ballots(fg, monkeypatch):
    """FHE_HOST with a 1 MiB stage: 64 ballots of 256 KiB go through the
    pipeline four at a time and fold with the accumulate flag; FHE_DEVICE
    gives the same words."""
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    n, q = 16384, P27
    ring = fg.PolynomialRing(n, q)
    a = ballots(5, q, 2, 64, 2, n)
    exp = fold(q, a)
    monkeypatch.setenv("FHE_STAGE_MB", "1")
    got = ring.sum_batch(a, grouped=True)
    assert (got == exp).all()
    prior = ballots(6, q, 2, 1, 2, n)[:, 0]
    hout = prior.copy()
    ring.sum_batch(a, out=hout, accumulate=True, grouped=True)
    assert (hout == fold(q, a, prior)).all()
    monkeypatch.delenv("FHE_STAGE_MB")
    assert (ring.sum_batch(a, grouped=True) == exp).all()
    assert (H(ring.sum_batch(D(a), grouped=True)) == exp).all()


@pytest.mark.parametrize("n,q,polys", [(16, 97, 2), (1024, QG, 3), (16384, P27, 2)])
def test_pointer_form(fg, n, q, polys, monkeypatch):
    """Every ciphertext in its own allocation, not adjacent and not in order,
    one of them listed twice."""
    import torch

    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    for count in (1, 2, 7, 64):
        a = ballots(count + polys, q, 1, count, polys, n)
        bufs, spacers = [], []
        for i in range(count):
            bufs.append(D(a[0, i]))
            spacers.append(torch.empty(1000 + 37 * i, dtype=torch.int64, device="cuda:0"))
        order = list(reversed(range(count))) + [count // 2]
        terms = np.stack([a[0, i] for i in order])[None]
        exp = fold(q, terms)[0]
        lst = [bufs[i] for i in order]
        got = H(eng.batch_add(lst)) if polys > 1 else H(ring.sum_buffers(lst))
        assert (got == exp).all(), count
        check_columns(q, terms, got[None])
    # the engine's array form and its aliases
    if polys > 1:
        assert (eng.tally_votes(a[0]) == fold(q, a)[0]).all()
        assert (eng.tally_multi_candidate(a[0], n) == fold(q, a)[0]).all()
        with pytest.raises(fg.FHEError, match="Number of candidates exceeds polynomial degree"):
            eng.tally_multi_candidate(a[0], n + 1)


def test_multi_device_context_splits_groups(fg, monkeypatch):
    monkeypatch.delenv("FHE_TALLY_SPLIT", raising=False)
    n, q = 1024, P62
    ring = fg.PolynomialRing(n, q, devices=[0, 0])
    a = ballots(11, q, 3, 7, 2, n)
    exp = fold(q, a)
    assert (ring.sum_batch(a, grouped=True) == exp).all()
    assert (H(ring.sum_batch(D(a), grouped=True)) == exp).all()
    bufs = [D(a[1, i]) for i in range(7)]
    assert (H(ring.sum_buffers(bufs)) == exp[1]).all()


def test_errors(fg):
    import torch

    n, q = 16, 97
    ring = fg.PolynomialRing(n, q)
    L = fg.lib()
    a = D(ballots(1, q, 1, 4, 2, n))
    out = torch.empty((2, n), dtype=torch.int64, device="cuda:0")
    pa, po = a.data_ptr(), out.data_ptr()

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return L.fhe_last_error().decode()

    assert err(L.fhe_ct_sum_batch(ring._h, pa, 2, 0, 1, 0, po, fg.FHE_DEVICE)) == "Cannot add empty vector of ciphertexts"
    for polys in (0, 4):
        err(L.fhe_ct_sum_batch(ring._h, pa, polys, 4, 1, 0, po, fg.FHE_DEVICE))
    err(L.fhe_ct_sum_batch(ring._h, None, 2, 4, 1, 0, po, fg.FHE_DEVICE))
    err(L.fhe_ct_sum_batch(ring._h, pa, 2, 4, 1, 0, None, fg.FHE_DEVICE))
    err(L.fhe_ct_sum_batch(ring._h, pa, 2, 4, 1, 0, po, 7))
    tab = (C.c_void_p * 4)(*[pa + 8 * 2 * n * i for i in range(4)])
    assert err(L.fhe_ct_sum_ptrs(ring._h, tab, 2, 0, 0, po)) == "Cannot add empty vector of ciphertexts"
    for polys in (0, 4):
        err(L.fhe_ct_sum_ptrs(ring._h, tab, polys, 4, 0, po))
    err(L.fhe_ct_sum_ptrs(ring._h, None, 2, 4, 0, po))
    err(L.fhe_ct_sum_ptrs(ring._h, tab, 2, 4, 0, None))
    bad = (C.c_void_p * 4)(pa, pa + 8, pa, pa)  # entry 1 is 8-byte aligned only
    assert "16-byte aligned" in err(L.fhe_ct_sum_ptrs(ring._h, bad, 2, 4, 0, po))
    hole = (C.c_void_p * 4)(pa, None, pa, pa)
    err(L.fhe_ct_sum_ptrs(ring._h, hole, 2, 4, 0, po))
    with pytest.raises(fg.FHEError, match="Cannot add empty vector of ciphertexts"):
        fg.EncryptionEngine(ring).batch_add([])
    # the failed calls enqueued nothing: a good call still works
    assert (H(ring.sum_batch(a[0])) == fold(q, H(a))[0]).all()


def test_tally_votes_end_to_end(fg):
    """Nine packed ballots, negacyclic ring, t = 65537: decrypting the tally
    gives the slot-wise plaintext sum mod t."""
    n, q, t, b = 1024, P62, 65537, 9
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)

    def rnd(seed, m, *shape):
        return oracle.splitmix_fill(seed, m, int(np.prod(shape))).reshape(shape)

    def tern(seed, *shape):
        x = rnd(seed, 3, *shape)
        return np.where(x == 2, np.uint64(q - 1), x).astype(np.uint64)

    a, s = rnd(901, q, n), tern(902, n)
    pk = fg.PublicKey(r, D(np.stack([a, r.multiply(a, s)])))
    key = fg.SecretKey(r, D(s))
    m = rnd(903, t, b, n)
    e = rnd(905, 7, 2, b, n).astype(np.int64) - 3
    e = np.where(e < 0, np.uint64(q) - (-e).astype(np.uint64), e.astype(np.uint64)).astype(np.uint64)
    ct = eng.encrypt(D(m), pk, D(tern(904, b, n)), D(e[0]), D(e[1]))
    want = (m.astype(object).sum(axis=0) % t).astype(np.uint64)
    for tally in (eng.tally_votes(ct), eng.tally_votes([ct[i] for i in range(b)]),
                  eng.tally_multi_candidate(ct, n)):
        assert tuple(tally.shape) == (2, n)
        res = eng.decrypt(tally, key)
        assert res.success.all()
        assert (H(res.values).reshape(n) == want).all()


def test_tally_js_engine(fg):
    """batchAdd / tallyVotes / tallyMultiCandidate / tallyWeightedVotes of the
    JS engine over the addon's sumAsync (tests/js/tally_test.js)."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "tally_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
