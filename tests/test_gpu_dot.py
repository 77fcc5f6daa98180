"""GPU parity of the fused ciphertext inner product (csrc/dot.hip,
fhe_ct_dot_batch / fhe_ct_dot_ptrs): out = sum_i multiply(a_i, b_i).

Expected value in compat mode: the sequential oracle.poly_add fold over
oracle.NTT(n, q).ct_multiply(a_i, b_i) (inputs read as x mod q).  In every
case, and as the only check in negacyclic mode (the oracle is compat), the
result is also compared bit for bit with the composition of the entry points
that existed before: fhe_ct_multiply_batch, then fhe_ct_sum_batch with polys
= 3.

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
QG = 18446744069414584321     # 2^64 - 2^32 + 1: outside the fused family
M64 = (1 << 64) - 1
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


def set_split(monkeypatch, split, components=None):
    """FHE_DOT_SPLIT forces the slices; FHE_DOT_COMPONENTS forces whole pairs
    ("0") or one workgroup per component of a slice's sum ("1"), which the
    library otherwise picks by the number of slices."""
    for name, val in (("FHE_DOT_SPLIT", split), ("FHE_DOT_COMPONENTS", components)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def pairs(seed, q, groups, count, n):
    """Two operands [groups, count, 2, n] of full-range random u64 words with
    the edge words planted in the first and the last pair of every group."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    out = []
    for _ in range(2):
        a = rng.integers(0, 1 << 64, size=(groups, count, 2, n), dtype=np.uint64)
        a[:, 0, 0, :4] = edge
        a[:, -1, -1, -4:] = edge[::-1]
        out.append(a)
    return out


def prior_words(seed, q, groups, n):
    """A prior `out` [groups, 3, n] of raw u64 words, the edge words included."""
    p = np.random.default_rng(seed).integers(0, 1 << 64, size=(groups, 3, n), dtype=np.uint64)
    p[:, 0, :4] = np.array([0, q - 1, q, M64], dtype=np.uint64)
    return p


def fold(q, n, a, b, prior=None, is_ntt=False):
    """Sequential poly_add fold of the oracle's ct_multiply over the pairs."""
    ref = oracle.NTT(n, q)
    qq = np.uint64(q)
    groups, count = a.shape[:2]
    out = np.empty((groups, 3, n), dtype=np.uint64)
    for g in range(groups):
        acc = np.zeros(3 * n, dtype=np.uint64)
        if prior is not None:
            acc = oracle.poly_add(q, acc, np.ascontiguousarray(prior[g]).ravel())
        for i in range(count):
            acc = oracle.poly_add(q, acc, ref.ct_multiply(a[g, i] % qq, b[g, i] % qq, is_ntt).ravel())
        out[g] = acc.reshape(3, n)
    return out


def composed(eng, da, db, is_ntt=False, prior=None):
    """The pre-existing entry points: multiply every pair, then one tally."""
    prod = eng.multiply(da, db, is_ntt=is_ntt)
    if prior is None:
        return H(eng.ring.sum_batch(prod, grouped=True))
    out = D(prior.copy())
    eng.ring.sum_batch(prod, out=out, accumulate=True, grouped=True)
    return H(out)


SMALL_COUNTS = [1, 2, 3, 7, 33]
SMALL_SPLITS = [None, "1", "2", "5", "1000"]


@pytest.mark.parametrize("mode", ["compat", "negacyclic"])
@pytest.mark.parametrize("n,q", [(4, 17), (16, 97)])
def test_several_polynomials_per_workgroup(fg, n, q, mode, monkeypatch):
    """n = 4 and 16: a workgroup holds 64 / 16 slices.  Counts below and not a
    multiple of that, every forced split (1000 is clamped to count), with and
    without a raw-u64 prior `out`, device and host resident."""
    ring = fg.PolynomialRing(n, q, mode=mode)
    eng = fg.EncryptionEngine(ring)
    for count in SMALL_COUNTS:
        for groups in (1, 3):
            a, b = pairs(100 * count + groups, q, groups, count, n)
            prior = prior_words(7, q, groups, n)
            da, db = D(a), D(b)
            set_split(monkeypatch, None)
            exp, exp_acc = composed(eng, da, db), composed(eng, da, db, prior=prior)
            if mode == "compat":
                assert (exp == fold(q, n, a, b)).all(), (count, groups)
                assert (exp_acc == fold(q, n, a, b, prior)).all(), (count, groups)
            for split, comp in [(s, c) for s in SMALL_SPLITS for c in ("0", "1")] + [(None, None)]:
                set_split(monkeypatch, split, comp)
                got = H(eng.dot(da, db))
                assert got.shape == (groups, 3, n)
                assert (got == exp).all(), (count, groups, split, comp)
                out = D(prior.copy())
                eng.dot(da, db, out=out, accumulate=True)
                assert (H(out) == exp_acc).all(), (count, groups, split, comp)
                if count in (1, 7, 33) and split in (None, "2"):  # FHE_HOST
                    assert (eng.dot(a, b) == exp).all(), (count, groups, split)
                    hout = prior.copy()
                    eng.dot(a, b, out=hout, accumulate=True)
                    assert (hout == exp_acc).all(), (count, groups, split)


@pytest.mark.parametrize("split", [None, "2"])
@pytest.mark.parametrize("q", [P27, P62])
def test_both_word_widths(fg, q, split, monkeypatch):
    """n = 1024 with 32-bit lanes (q < 2^30) and 64-bit lanes: coefficient and
    NTT-domain inputs, contiguous and pointer tables (one pointer repeated, one
    pair with a[i] is b[i])."""
    n, groups = 1024, 3
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    for count in (1, 3, 33):
        a, b = pairs(count, q, groups, count, n)
        da, db = D(a), D(b)
        for is_ntt in (False, True):
            set_split(monkeypatch, None)
            exp = composed(eng, da, db, is_ntt)
            assert (exp == fold(q, n, a, b, is_ntt=is_ntt)).all(), (count, is_ntt)
            for comp in ("0", "1"):
                set_split(monkeypatch, split, comp)
                assert (H(eng.dot(da, db, is_ntt=is_ntt)) == exp).all(), (count, is_ntt, comp)
            # pointer tables over group 0: reversed order, one pair listed twice, one square
            order = list(reversed(range(count))) + [count // 2]
            la = [D(a[0, i]) for i in range(count)]
            lb = [D(b[0, i]) for i in range(count)]
            ta, tb = [la[i] for i in order] + [la[0]], [lb[i] for i in order] + [la[0]]
            terms_a = np.stack([a[0, i] for i in order] + [a[0, 0]])[None]
            terms_b = np.stack([b[0, i] for i in order] + [a[0, 0]])[None]
            want = fold(q, n, terms_a, terms_b, is_ntt=is_ntt)[0]
            set_split(monkeypatch, split, "0")
            assert (H(eng.dot_buffers(ta, tb, is_ntt=is_ntt)) == want).all(), (count, is_ntt)
            pout = D(exp[1].copy())
            set_split(monkeypatch, split, "1")
            eng.dot_buffers(ta, tb, is_ntt=is_ntt, out=pout, accumulate=True)
            assert (H(pout) == fold(q, n, terms_a, terms_b, exp[1][None], is_ntt=is_ntt)[0]).all(), (count, is_ntt)


@pytest.mark.parametrize("n,q,count", [(8192, P27, 5), (16384, P27, 5), (16384, P62, 3)])
def test_largest_fused_sizes(fg, n, q, count, monkeypatch):
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    a, b = pairs(n + count, q, 1, count, n)
    da, db = D(a), D(b)
    exp = fold(q, n, a, b)
    assert (composed(eng, da, db) == exp).all()
    for comp in ("0", "1"):
        set_split(monkeypatch, "2", comp)
        assert (H(eng.dot(da, db)) == exp).all(), comp


@pytest.mark.parametrize("n,q", [(32768, P27), (1024, QG)])
def test_composed_shapes(fg, n, q, monkeypatch):
    """Outside the fused family (n > 16384, q >= 2^62) the call runs composed:
    same words, contiguous, pointer-table and host-resident."""
    set_split(monkeypatch, None)
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    a, b = pairs(n, q, 1, 3, n)
    da, db = D(a), D(b)
    exp = fold(q, n, a, b)
    got = H(eng.dot(da, db))
    assert (got == exp).all()
    assert (got == composed(eng, da, db)).all()
    if n == 1024:
        prior = exp[0].copy()
        out = D(prior)
        eng.dot_buffers([D(a[0, i]) for i in range(3)], [D(b[0, i]) for i in range(3)], out=out, accumulate=True)
        assert (H(out) == fold(q, n, a, b, prior[None])[0]).all()
        assert (eng.dot(a, b) == exp).all()
        assert (H(eng.dot(da, db, is_ntt=True)) == fold(q, n, a, b, is_ntt=True)).all()


def test_multi_device_context_splits_groups(fg, monkeypatch):
    set_split(monkeypatch, None)
    n, q = 16, 97
    eng = fg.EncryptionEngine(fg.PolynomialRing(n, q, devices=[0, 0]))
    a, b = pairs(11, q, 3, 7, n)
    exp = fold(q, n, a, b)
    assert (eng.dot(a, b) == exp).all()          # FHE_HOST: the groups are split
    assert (H(eng.dot(D(a), D(b))) == exp).all()
    la, lb = [D(a[1, i]) for i in range(7)], [D(b[1, i]) for i in range(7)]
    assert (H(eng.dot_buffers(la, lb)) == exp[1]).all()


def test_errors(fg):
    import torch

    n, q = 16, 97
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    L = fg.lib()
    a, b = pairs(1, q, 1, 4, n)
    da, db = D(a), D(b)
    out = torch.empty((3, n), dtype=torch.int64, device="cuda:0")
    pa, pb, po = da.data_ptr(), db.data_ptr(), out.data_ptr()
    dev = fg.FHE_DEVICE

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return L.fhe_last_error().decode()

    assert err(L.fhe_ct_dot_batch(ring._h, pa, pb, 0, 1, 0, 0, po, dev)) == "Cannot tally empty ballot list"
    assert err(L.fhe_ct_dot_batch(ring._h, None, pb, 4, 1, 0, 0, po, dev)) == "null buffer"
    assert err(L.fhe_ct_dot_batch(ring._h, pa, None, 4, 1, 0, 0, po, dev)) == "null buffer"
    assert err(L.fhe_ct_dot_batch(ring._h, pa, pb, 4, 1, 0, 0, None, dev)) == "null buffer"
    err(L.fhe_ct_dot_batch(ring._h, pa, pb, 4, 1, 0, 0, po, 7))
    assert "16-byte aligned" in err(L.fhe_ct_dot_batch(ring._h, pa + 8, pb, 3, 1, 0, 0, po, dev))
    assert "16-byte aligned" in err(L.fhe_ct_dot_batch(ring._h, pa, pb, 4, 1, 0, 0, po + 8, dev))
    # out inside an input: the last three polynomials of a / the first three of b
    assert "overlap" in err(L.fhe_ct_dot_batch(ring._h, pa, pb, 4, 1, 0, 0, pa + 8 * 5 * n, dev))
    assert "overlap" in err(L.fhe_ct_dot_batch(ring._h, pa, pb, 4, 1, 0, 0, pb, dev))
    ta = (C.c_void_p * 4)(*[pa + 8 * 2 * n * i for i in range(4)])
    tb = (C.c_void_p * 4)(*[pb + 8 * 2 * n * i for i in range(4)])
    assert err(L.fhe_ct_dot_ptrs(ring._h, ta, tb, 0, 0, 0, po)) == "Cannot tally empty ballot list"
    assert err(L.fhe_ct_dot_ptrs(ring._h, None, tb, 4, 0, 0, po)) == "null buffer"
    assert err(L.fhe_ct_dot_ptrs(ring._h, ta, tb, 4, 0, 0, None)) == "null buffer"
    hole = (C.c_void_p * 4)(pa, None, pa, pa)
    assert err(L.fhe_ct_dot_ptrs(ring._h, ta, hole, 4, 0, 0, po)) == "null buffer"
    bad = (C.c_void_p * 4)(pa, pa + 8, pa, pa)  # entry 1 is 8-byte aligned only
    assert "16-byte aligned" in err(L.fhe_ct_dot_ptrs(ring._h, bad, tb, 4, 0, 0, po))
    assert "overlap" in err(L.fhe_ct_dot_ptrs(ring._h, ta, tb, 4, 0, 0, pb + 8 * 2 * n))
    with pytest.raises(fg.FHEError, match="Cannot tally empty ballot list"):
        eng.dot_buffers([], [])
    with pytest.raises(fg.FHEError, match="Ballots and weights must have the same size"):
        eng.tally_weighted_votes([da[0, 0], da[0, 1]], [db[0, 0]], None)
    with pytest.raises(fg.FHEError, match="Cannot tally empty ballot list"):
        eng.tally_weighted_votes([], [], None)
    # the failed calls enqueued nothing: a good call still works
    assert (H(eng.dot(da, db)) == fold(q, n, a, b)).all()


def test_weighted_tally_decrypts_and_matches_the_reference_fold(fg):
    """The parameters of the weighted-tally JS test (q = j t^2 + t + 1,
    noise-free, negacyclic, digits covering all of c2): the degree-2 dot
    product and the lazily relinearised tally decode to sum w_i b_i mod t;
    relinearize="each" gives the words of the oracle's relinearise-per-ballot
    fold (compat ring: the oracle is compat; the words need no key relation)."""
    n, t, q, base_log, level = 1024, 2048, 2305843009276610561, 16, 4
    bs, ws = [1, 0, 1], [3, 5, 7]
    want = sum(x * w for x, w in zip(bs, ws)) % t
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    kg = fg.KeyGenerator(r, bytes(range(32)), noise_std=3.2e-11)
    s = kg.secret_key(1)
    pk, key = fg.PublicKey(r, D(kg.public_key(s, 2))), fg.SecretKey(r, D(s))
    rlk = kg.eval_key(s, base_log, level, 3)
    ek = fg.EvaluationKey(r, D(rlk), base_log)
    u = oracle.splitmix_fill(31, 3, 6 * n).reshape(6, n)
    u = np.where(u == 2, np.uint64(q - 1), u).astype(np.uint64)
    zero = np.zeros((6, n), dtype=np.uint64)
    vals = np.zeros((6, n), dtype=np.uint64)
    vals[:, 0] = bs + ws
    ct = eng.encrypt(D(vals), pk, D(u), D(zero), D(zero))
    ballots, weights = ct[:3].contiguous(), ct[3:].contiguous()

    def slot0(c):
        res = eng.decrypt(c, key)
        assert res.success.all()
        return int(H(res.values).reshape(-1)[0])

    d2 = eng.dot(ballots, weights)
    assert tuple(d2.shape) == (3, n)
    # The phase of a tensor product is c0 - c1 s + c2 s^2; the reference's
    # degree-2 decrypt (encryption.cpp:268-286), which decrypt() reproduces,
    # subtracts c2 s^2.  Decrypt (c0, c1, -c2).
    d2[2] = r.negate(d2[2].clone())
    assert slot0(d2) == want
    once = eng.tally_weighted_votes(ballots, weights, ek, relinearize="once")
    assert tuple(once.shape) == (2, n)
    assert slot0(once) == want
    assert slot0(eng.tally_weighted_votes([ballots[i] for i in range(3)], [weights[i] for i in range(3)], ek,
                                          relinearize="once")) == want
    each = eng.tally_weighted_votes(ballots, weights, ek, relinearize="each")
    assert slot0(each) == want
    assert (H(each) == H(eng.tally_weighted_votes(ballots, weights, ek))).all()  # the default
    # word for word against the oracle's fold, compat ring, same ciphertext and key words
    rc = fg.PolynomialRing(n, q)
    engc = fg.EncryptionEngine(rc, t)
    ref = oracle.NTT(n, q)
    hb, hw = H(ballots), H(weights)
    acc = np.zeros(2 * n, dtype=np.uint64)
    for i in range(3):
        acc = oracle.poly_add(q, acc, ref.relinearize(base_log, level, ref.ct_multiply(hb[i], hw[i]), rlk).ravel())
    got = engc.tally_weighted_votes(ballots, weights, fg.EvaluationKey(rc, D(rlk), base_log), relinearize="each")
    assert (H(got) == acc.reshape(2, n)).all()


def test_dot_js_engine(fg):
    """dotProduct and tallyWeightedVotes(..., { relinearize: 'once' }) of the
    JS engine over the addon's dotAsync (tests/js/dot_test.js)."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "dot_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
