"""GPU parity of the fused plaintext-weighted inner product
(csrc/dot_plain.hip, fhe_ct_dot_plain_batch / fhe_ct_dot_plain_ptrs):
out = sum_i multiply_plain(ct_i, p_i) folded by add().

Expected value in compat mode: the sequential oracle.poly_add fold of
(ref.polymul(c0 % q, p % q), ref.polymul(c1 % q, p % q)), or with is_ntt of
oracle.pointwise(q, c_j % q, ref.forward(p % q)).  In every case, and as the
only check in negacyclic mode (the oracle is compat), the result is also
compared bit for bit with the device chain of the entry points that existed
before: ring.multiply (or ring.forward_ntt + ring.pointwise_multiply) per
component, then sum_batch with polys = 2.

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


def set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("FHE_DOT_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FHE_DOT_SPLIT", split)


def pairs(seed, q, groups, count, n):
    """cts [groups, count, 2, n] and pts [groups, count, n] of full-range
    random u64 words with the edge words planted in the first and the last
    pair of every group."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    c = rng.integers(0, 1 << 64, size=(groups, count, 2, n), dtype=np.uint64)
    c[:, 0, 0, :4] = edge
    c[:, -1, -1, -4:] = edge[::-1]
    p = rng.integers(0, 1 << 64, size=(groups, count, n), dtype=np.uint64)
    p[:, 0, :4] = edge[::-1]
    p[:, -1, -4:] = edge
    return c, p


def prior_words(seed, q, groups, n):
    """A prior `out` [groups, 2, n] of raw u64 words, the edge words included."""
    p = np.random.default_rng(seed).integers(0, 1 << 64, size=(groups, 2, n), dtype=np.uint64)
    p[:, 0, :4] = np.array([0, q - 1, q, M64], dtype=np.uint64)
    return p


def fold(q, n, c, p, prior=None, is_ntt=False):
    """Sequential poly_add fold of the oracle's multiply_plain over the pairs."""
    ref = oracle.NTT(n, q)
    qq = np.uint64(q)
    groups, count = c.shape[:2]
    out = np.empty((groups, 2, n), dtype=np.uint64)
    for g in range(groups):
        acc = np.zeros(2 * n, dtype=np.uint64)
        if prior is not None:
            acc = oracle.poly_add(q, acc, np.ascontiguousarray(prior[g]).ravel())
        for i in range(count):
            pi = np.ascontiguousarray(p[g, i] % qq)
            ci = np.ascontiguousarray(c[g, i] % qq)
            if is_ntt:
                fp = ref.forward(pi)
                term = np.stack([oracle.pointwise(q, ci[j], fp) for j in range(2)])
            else:
                term = np.stack([ref.polymul(ci[j], pi) for j in range(2)])
            acc = oracle.poly_add(q, acc, np.ascontiguousarray(term).ravel())
        out[g] = acc.reshape(2, n)
    return out


def chain(ring, dc, dp, is_ntt=False, prior=None):
    """The pre-existing entry points: every component times its plaintext
    (the plaintext replicated over the two components), then one tally."""
    pb = dp.unsqueeze(-2).expand(dc.shape).contiguous()
    if is_ntt:
        prod = ring.pointwise_multiply(dc, ring.forward_ntt(pb.clone()))
    else:
        prod = ring.multiply(dc, pb)
    if prior is None:
        return H(ring.sum_batch(prod, grouped=True))
    out = D(prior.copy())
    ring.sum_batch(prod, out=out, accumulate=True, grouped=True)
    return H(out)


SMALL_COUNTS = [1, 2, 3, 7, 33]
SMALL_SPLITS = [None, "1", "2", "5", "1000"]


@pytest.mark.parametrize("mode", ["compat", "negacyclic"])
@pytest.mark.parametrize("n,q", [(4, 17), (16, 97)])
def test_several_polynomials_per_workgroup(fg, n, q, mode, monkeypatch):
    """n = 4 and 16: a workgroup holds 64 / 16 slices.  Counts below and not a
    multiple of that, every forced split (1000 is clamped to count), both
    domains, with and without a raw-u64 prior `out`, device and host."""
    ring = fg.PolynomialRing(n, q, mode=mode)
    eng = fg.EncryptionEngine(ring)
    for count in SMALL_COUNTS:
        for groups in (1, 3):
            c, p = pairs(100 * count + groups, q, groups, count, n)
            prior = prior_words(7, q, groups, n)
            dc, dp = D(c), D(p)
            for is_ntt in (False, True):
                set_split(monkeypatch, None)
                exp, exp_acc = chain(ring, dc, dp, is_ntt), chain(ring, dc, dp, is_ntt, prior)
                if mode == "compat":
                    assert (exp == fold(q, n, c, p, is_ntt=is_ntt)).all(), (count, groups, is_ntt)
                    assert (exp_acc == fold(q, n, c, p, prior, is_ntt)).all(), (count, groups, is_ntt)
                for split in SMALL_SPLITS:
                    set_split(monkeypatch, split)
                    got = H(eng.dot_plain(dc, dp, is_ntt=is_ntt))
                    assert got.shape == (groups, 2, n)
                    assert (got == exp).all(), (count, groups, is_ntt, split)
                    out = D(prior.copy())
                    eng.dot_plain(dc, dp, is_ntt=is_ntt, out=out, accumulate=True)
                    assert (H(out) == exp_acc).all(), (count, groups, is_ntt, split)
                    if count in (1, 7, 33) and split in (None, "2"):  # FHE_HOST
                        assert (eng.dot_plain(c, p, is_ntt=is_ntt) == exp).all(), (count, groups, is_ntt, split)
                        hout = prior.copy()
                        eng.dot_plain(c, p, is_ntt=is_ntt, out=hout, accumulate=True)
                        assert (hout == exp_acc).all(), (count, groups, is_ntt, split)


@pytest.mark.parametrize("split", [None, "2"])
@pytest.mark.parametrize("q", [P27, P62])
def test_both_word_widths(fg, q, split, monkeypatch):
    """n = 1024 with 32-bit lanes (q < 2^30) and 64-bit lanes: coefficient and
    NTT-domain ciphertexts, contiguous and pointer tables (one ciphertext
    repeated, one plaintext shared by two ballots)."""
    n, groups = 1024, 3
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    for count in (1, 3, 33):
        c, p = pairs(count, q, groups, count, n)
        dc, dp = D(c), D(p)
        for is_ntt in (False, True):
            set_split(monkeypatch, None)
            exp = chain(ring, dc, dp, is_ntt)
            assert (exp == fold(q, n, c, p, is_ntt=is_ntt)).all(), (count, is_ntt)
            set_split(monkeypatch, split)
            assert (H(eng.dot_plain(dc, dp, is_ntt=is_ntt)) == exp).all(), (count, is_ntt)
            # pointer tables over group 0: reversed order, ciphertext 0 listed
            # again under plaintext count // 2 (so shared by two ballots)
            order = list(reversed(range(count))) + [0]
            porder = list(reversed(range(count))) + [count // 2]
            lc = [D(c[0, i]) for i in range(count)]
            lp = [D(p[0, i]) for i in range(count)]
            tc, tp = [lc[i] for i in order], [lp[i] for i in porder]
            terms_c = np.stack([c[0, i] for i in order])[None]
            terms_p = np.stack([p[0, i] for i in porder])[None]
            want = fold(q, n, terms_c, terms_p, is_ntt=is_ntt)[0]
            assert (H(eng.dot_plain_buffers(tc, tp, is_ntt=is_ntt)) == want).all(), (count, is_ntt)
            pout = D(exp[1].copy())
            eng.dot_plain_buffers(tc, tp, is_ntt=is_ntt, out=pout, accumulate=True)
            assert (H(pout) == fold(q, n, terms_c, terms_p, exp[1][None], is_ntt)[0]).all(), (count, is_ntt)


@pytest.mark.parametrize("n,q,count", [(8192, P27, 5), (16384, P27, 5), (16384, P62, 3)])
def test_largest_fused_sizes(fg, n, q, count, monkeypatch):
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    c, p = pairs(n + count, q, 1, count, n)
    dc, dp = D(c), D(p)
    for is_ntt in (False, True):
        set_split(monkeypatch, None)
        exp = fold(q, n, c, p, is_ntt=is_ntt)
        assert (chain(ring, dc, dp, is_ntt) == exp).all(), is_ntt
        set_split(monkeypatch, "2")
        assert (H(eng.dot_plain(dc, dp, is_ntt=is_ntt)) == exp).all(), is_ntt


@pytest.mark.parametrize("n,q", [(32768, P27), (1024, QG)])
def test_composed_shapes(fg, n, q, monkeypatch):
    """Outside the fused family (n > 16384, q >= 2^62) the call runs composed:
    same words, contiguous, pointer-table and host-resident."""
    set_split(monkeypatch, None)
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    c, p = pairs(n, q, 1, 3, n)
    dc, dp = D(c), D(p)
    exp = fold(q, n, c, p)
    got = H(eng.dot_plain(dc, dp))
    assert (got == exp).all()
    assert (got == chain(ring, dc, dp)).all()
    if n == 1024:
        prior = exp[0].copy()
        out = D(prior)
        eng.dot_plain_buffers([D(c[0, i]) for i in range(3)], [D(p[0, i]) for i in range(3)], out=out, accumulate=True)
        assert (H(out) == fold(q, n, c, p, prior[None])[0]).all()
        assert (eng.dot_plain(c, p) == exp).all()
        exp_ntt = fold(q, n, c, p, is_ntt=True)
        assert (H(eng.dot_plain(dc, dp, is_ntt=True)) == exp_ntt).all()
        assert (chain(ring, dc, dp, True) == exp_ntt).all()


def test_multi_device_context_splits_groups(fg, monkeypatch):
    set_split(monkeypatch, None)
    n, q = 16, 97
    eng = fg.EncryptionEngine(fg.PolynomialRing(n, q, devices=[0, 0]))
    c, p = pairs(11, q, 3, 7, n)
    exp = fold(q, n, c, p)
    assert (eng.dot_plain(c, p) == exp).all()          # FHE_HOST: the groups are split
    assert (H(eng.dot_plain(D(c), D(p))) == exp).all()
    lc, lp = [D(c[1, i]) for i in range(7)], [D(p[1, i]) for i in range(7)]
    assert (H(eng.dot_plain_buffers(lc, lp)) == exp[1]).all()


def test_errors(fg):
    import torch

    n, q = 16, 97
    ring = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(ring)
    L = fg.lib()
    c, p = pairs(1, q, 1, 4, n)
    dc, dp = D(c), D(p)
    out = torch.empty((2, n), dtype=torch.int64, device="cuda:0")
    pc, pp, po = dc.data_ptr(), dp.data_ptr(), out.data_ptr()
    dev = fg.FHE_DEVICE

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return L.fhe_last_error().decode()

    assert err(L.fhe_ct_dot_plain_batch(ring._h, pc, pp, 0, 1, 0, 0, po, dev)) == "Cannot tally empty ballot list"
    assert err(L.fhe_ct_dot_plain_batch(ring._h, None, pp, 4, 1, 0, 0, po, dev)) == "null buffer"
    assert err(L.fhe_ct_dot_plain_batch(ring._h, pc, None, 4, 1, 0, 0, po, dev)) == "null buffer"
    assert err(L.fhe_ct_dot_plain_batch(ring._h, pc, pp, 4, 1, 0, 0, None, dev)) == "null buffer"
    err(L.fhe_ct_dot_plain_batch(ring._h, pc, pp, 4, 1, 0, 0, po, 7))
    assert "16-byte aligned" in err(L.fhe_ct_dot_plain_batch(ring._h, pc + 8, pp, 3, 1, 0, 0, po, dev))
    assert "16-byte aligned" in err(L.fhe_ct_dot_plain_batch(ring._h, pc, pp, 4, 1, 0, 0, po + 8, dev))
    # out inside an input: the last two polynomials of cts / the first two of pts
    assert "overlap" in err(L.fhe_ct_dot_plain_batch(ring._h, pc, pp, 4, 1, 0, 0, pc + 8 * 6 * n, dev))
    assert "overlap" in err(L.fhe_ct_dot_plain_batch(ring._h, pc, pp, 4, 1, 0, 0, pp, dev))
    tc = (C.c_void_p * 4)(*[pc + 8 * 2 * n * i for i in range(4)])
    tp = (C.c_void_p * 4)(*[pp + 8 * n * i for i in range(4)])
    assert err(L.fhe_ct_dot_plain_ptrs(ring._h, tc, tp, 0, 0, 0, po)) == "Cannot tally empty ballot list"
    assert err(L.fhe_ct_dot_plain_ptrs(ring._h, None, tp, 4, 0, 0, po)) == "null buffer"
    assert err(L.fhe_ct_dot_plain_ptrs(ring._h, tc, tp, 4, 0, 0, None)) == "null buffer"
    hole = (C.c_void_p * 4)(pp, None, pp, pp)
    assert err(L.fhe_ct_dot_plain_ptrs(ring._h, tc, hole, 4, 0, 0, po)) == "null buffer"
    bad = (C.c_void_p * 4)(pc, pc + 8, pc, pc)  # entry 1 is 8-byte aligned only
    assert "16-byte aligned" in err(L.fhe_ct_dot_plain_ptrs(ring._h, bad, tp, 4, 0, 0, po))
    assert "overlap" in err(L.fhe_ct_dot_plain_ptrs(ring._h, tc, tp, 4, 0, 0, pp + 8 * n))
    with pytest.raises(fg.FHEError, match="Cannot tally empty ballot list"):
        eng.dot_plain_buffers([], [])
    with pytest.raises(fg.FHEError, match="Ballots and weights must have the same size"):
        eng.dot_plain_buffers([dc[0, 0], dc[0, 1]], [dp[0, 0]])
    # the failed calls enqueued nothing: a good call still works
    assert (H(eng.dot_plain(dc, dp)) == fold(q, n, c, p)).all()


def test_public_weight_tallies_decrypt(fg):
    """The parameters of test_weighted_tally_decrypts_and_matches_the_reference_fold
    (n = 1024, t = 2048, q = 2305843009276610561, negacyclic, noise-free):
    ballots (1, 0, 1) under the public weights (3, 5, 7) tally to 10 in slot
    0, by integer scalars and by the constant plaintext polynomials encode(w_i);
    with pts = encode(1) X^k the tally of the ballots moves from slot 0 to
    slot k."""
    n, t, q = 1024, 2048, 2305843009276610561
    bs, ws = [1, 0, 1], [3, 5, 7]
    want = sum(x * w for x, w in zip(bs, ws)) % t
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    kg = fg.KeyGenerator(r, bytes(range(32)), noise_std=3.2e-11)
    s = kg.secret_key(1)
    pk, key = fg.PublicKey(r, D(kg.public_key(s, 2))), fg.SecretKey(r, D(s))
    u = oracle.splitmix_fill(31, 3, 3 * n).reshape(3, n)
    u = np.where(u == 2, np.uint64(q - 1), u).astype(np.uint64)
    zero = np.zeros((3, n), dtype=np.uint64)
    vals = np.zeros((3, n), dtype=np.uint64)
    vals[:, 0] = bs
    ballots = eng.encrypt(D(vals), pk, D(u), D(zero), D(zero))

    def slots(c):
        res = eng.decrypt(c, key)
        assert res.success.all()
        return H(res.values).reshape(-1)

    tally = eng.tally_scalar_weighted(ballots, ws)
    assert tuple(tally.shape) == (2, n)
    assert int(slots(tally)[0]) == want
    assert int(slots(eng.tally_scalar_weighted([ballots[i] for i in range(3)], ws))[0]) == want
    # constant plaintext polynomials: the integer w_i itself (a scalar of the
    # ring), which scales the encoded message as multiply_scalar does
    pts = np.zeros((3, n), dtype=np.uint64)
    pts[:, 0] = ws
    dpl = eng.dot_plain(ballots, D(pts))
    assert tuple(dpl.shape) == (2, n)
    assert int(slots(dpl)[0]) == want
    assert (H(dpl) == H(tally)).all()  # the same ring elements: the same words
    # the encoded plaintexts multiply_plain takes (delta w_i): delta^2 m w decodes to m w at this q
    enc = oracle.encode(q, t, pts.ravel()).reshape(3, n)
    assert int(enc[0, 0]) == ws[0] * (q // t) and not enc[:, 1:].any()
    assert int(slots(eng.dot_plain(ballots, D(enc)))[0]) == want
    # X^k: slot 0 moves to slot k
    k = 5
    mono = np.zeros((3, n), dtype=np.uint64)
    mono[:, k] = 1
    moved = slots(eng.dot_plain(ballots, D(mono)))
    assert int(moved[k]) == sum(bs) % t and int(moved[0]) == 0
    lists = eng.dot_plain_buffers([ballots[i] for i in range(3)], [D(mono[i]) for i in range(3)])
    assert (slots(lists) == moved).all()


def test_weighted_js_engine(fg):
    """tallyScalarWeightedVotes, dotPlain and the rerouted multiplyPlain of the
    JS engine over the addon's sumScaledAsync / dotPlainAsync
    (tests/js/weighted_test.js)."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "weighted_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
