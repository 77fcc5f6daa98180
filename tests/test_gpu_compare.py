"""Encrypted comparisons on the GPU (fhe_slot_extract_batch, fhe_lwe_sum_batch,
fhe_gpu.Comparisons):

- the extraction, word for word, against the formula of include/fhe_gpu.h in
  exact integer arithmetic and against the chain of existing entry points
  (subtract / negate, multiply_glwe_by_monomial by -slot, sample_extract, a
  modular add on the body), in both modes, both residences and on a
  multi-device context;
- its meaning: the LWE phase under a ternary key is the coefficient of the
  RLWE phase;
- fhe_lwe_sum_batch against Python integers;
- the comparison pipelines, word for word, against the explicit chain and the
  oracle's bootstrap;
- their truth tables under all-zero keys;
- the JS engine (tests/js/compare_test.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from ntt_primes import prime_above

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
QG = 18446744069414584321     # 2^64 - 2^32 + 1
M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q63 = prime_above(1 << 63, 512)


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


def raw_cts(seed, q, shape):
    """Full-range u64 ciphertexts [..., 2, n] with 0, q - 1, q, 2^64 - 1 planted
    at both ends of c0 and c1 (a zero word in c1 among them)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    a[..., :4] = edge
    a[..., -4:] = edge[::-1]
    return a


def full_offsets(seed, q, count):
    rng = np.random.default_rng(seed)
    offs = [int(v) for v in rng.integers(0, 1 << 64, size=count, dtype=np.uint64)]
    for i, v in enumerate((M64, q, q - 1, 0)):
        if i < count:
            offs[i] = v
    return offs


def difference(q, ct, ref, negate):
    """D [batch, 2, n] of the contract, in exact u64 arithmetic on reduced words."""
    Q = np.uint64(q)
    x = ct % Q
    y = np.broadcast_to(ref % Q, x.shape) if ref is not None else np.zeros_like(x)
    if negate:
        x, y = y, x
    with np.errstate(over="ignore"):
        return np.where(x >= y, x - y, Q - (y - x))


def expected(q, ct, ref, negate, slots, offsets):
    """(a [batch, S, n], b [batch, S]) of the contract."""
    Q = np.uint64(q)
    d = difference(q, ct, ref, negate)
    d0, d1 = d[:, 0], d[:, 1]
    nd1 = np.where(d1 == 0, np.uint64(0), Q - d1)
    batch, n = d1.shape
    j = np.arange(n)
    a = np.empty((batch, len(slots), n), np.uint64)
    b = np.empty((batch, len(slots)), np.uint64)
    for s, h in enumerate(slots):
        idx = (h - j) % n
        a[:, s] = np.where(j <= h, d1[:, idx], nd1[:, idx])
        off = (offsets[s] if offsets is not None else 0) % q
        b[:, s] = np.array([(int(v) + off) % q for v in d0[:, h]], dtype=np.uint64)
    return a, b


def expected_python(q, ct, ref, negate, slots, offsets):
    """The same in Python integers, word by word (small shapes)."""
    batch, _, n = ct.shape
    out_a, out_b = [], []
    for c in range(batch):
        rc = None if ref is None else (ref if ref.ndim == 2 else ref[c])
        d = [[0] * n, [0] * n]
        for p in range(2):
            for i in range(n):
                x, y = int(ct[c, p, i]) % q, (int(rc[p, i]) % q if rc is not None else 0)
                d[p][i] = (y - x) % q if negate else (x - y) % q
        for s, h in enumerate(slots):
            out_a.append([d[1][h - j] if j <= h else (q - d[1][n + h - j]) % q for j in range(n)])
            out_b.append((d[0][h] + (offsets[s] if offsets is not None else 0) % q) % q)
    S = len(slots)
    return (np.array(out_a, dtype=np.uint64).reshape(batch, S, n), np.array(out_b, dtype=np.uint64).reshape(batch, S))


def chain(fg, r, be, q, ct, ref, negate, slots, offsets):
    """The chain of existing entry points on device tensors."""
    batch = ct.shape[0]
    dct = D(ct)
    if ref is None:  # fhe_poly_neg_batch takes the reduced words
        d = r.negate(D(ct % np.uint64(q))) if negate else r.subtract(dct, D(np.zeros_like(ct)))
    else:
        dref = D(np.broadcast_to(ref, ct.shape).copy())
        d = r.subtract(dref, dct) if negate else r.subtract(dct, dref)
    glwe = d.flip(-2).contiguous()  # (mask D1, body D0)
    out_a, out_b = [], []
    for s, h in enumerate(slots):
        a, b = be.sample_extract(be.multiply_glwe_by_monomial(glwe, [-h] * batch))
        off = (offsets[s] if offsets is not None else 0) % q
        out_a.append(H(a))
        out_b.append(np.array([(int(v) + off) % q for v in H(b)], dtype=np.uint64))
    return np.stack(out_a, axis=1), np.stack(out_b, axis=1)


def slot_lists(n, all_slots):
    lists = [[0], [n - 1], [0, n - 1, n // 2, n // 2]]
    if all_slots:
        lists.append(list(range(n)))
    return lists


def sweep(fg, n, q, batches, lists, chain_every):
    """Every (mode, batch, slot list, ref_count, negate, offsets) combination
    against the formula; the device chain in compat mode for the combinations
    chain_every picks (the all-slots list: one of them)."""
    rings = {m: fg.PolynomialRing(n, q, mode=m) for m in ("compat", "negacyclic")}
    engines = {m: fg.BootstrapEngine(r, 4, 1, 1) for m, r in rings.items()}
    calls = 0
    for batch in batches:
        ct = raw_cts([n, batch, 1], q, (batch, 2, n))
        refs = {0: None, 1: raw_cts([n, batch, 2], q, (2, n)), batch: raw_cts([n, batch, 3], q, (batch, 2, n))}
        for slots in lists:
            for ref_count, ref in refs.items():
                for negate in (False, True):
                    for offsets in (None, full_offsets([n, batch, len(slots)], q, len(slots))):
                        want_a, want_b = expected(q, ct, ref, negate, slots, offsets)
                        tag = (n, q, batch, len(slots), ref_count, negate, offsets is not None)
                        if n <= 16:
                            pa, pb = expected_python(q, ct, ref, negate, slots, offsets)
                            assert (pa == want_a).all() and (pb == want_b).all(), tag
                        assert (want_a < np.uint64(q)).all() and (want_b < np.uint64(q)).all()
                        for mode, be in engines.items():
                            a, b = be.slot_extract(D(ct), slots, offsets, None if ref is None else D(ref), negate)
                            assert tuple(a.shape) == (batch, len(slots), n) and tuple(b.shape) == (batch, len(slots))
                            assert (H(a) == want_a).all(), tag + (mode,)
                            assert (H(b) == want_b).all(), tag + (mode,)
                            calls += 1
                        if chain_every(len(slots), batch, ref_count, negate, offsets):
                            ca, cb = chain(fg, rings["compat"], engines["compat"], q, ct, ref, negate, slots, offsets)
                            assert (ca == want_a).all() and (cb == want_b).all(), tag + ("chain",)
    return calls


@pytest.mark.parametrize("n,q", [(4, 97), (16, 97), (256, 7681), (1024, P27), (1024, P62), (1024, QG), (512, Q63)])
def test_slot_extract_words(fg, n, q):
    def chain_every(nslots, batch, ref_count, negate, offsets):
        if nslots > 4:  # all n slots: one combination
            return batch == 3 and ref_count == batch and negate and offsets is not None
        return offsets is not None or batch == 3

    calls = sweep(fg, n, q, (1, 3, 17), slot_lists(n, n <= 256), chain_every)
    # modes x slot lists x negate x offsets x (ref_count 0 / 1 / batch per batch; 1 = batch at batch 1)
    assert calls == 2 * (4 if n <= 256 else 3) * 2 * 2 * (2 + 3 + 3)


@pytest.mark.parametrize("n,q,batch,slots", [(16384, P62, 3, "four"), (32768, P27, 2, "three")])
def test_slot_extract_words_large_degrees(fg, n, q, batch, slots):
    lst = [0, n - 1, n // 2, n // 2] if slots == "four" else [0, n - 1, n // 2]
    sweep(fg, n, q, (batch,), [lst], lambda ns, b, rc, neg, offs: rc == b and offs is not None)


def test_slot_extract_host_and_multi_device(fg):
    n, q, batch = 1024, P62, 17
    slots = [0, n - 1, n // 2, n // 2] + list(range(20))  # beyond the inline table
    offsets = full_offsets(5, q, len(slots))
    ct, ref = raw_cts(41, q, (batch, 2, n)), raw_cts(42, q, (batch, 2, n))
    one = raw_cts(43, q, (2, n))
    for devices in (None, [0, 0]):
        r = fg.PolynomialRing(n, q, devices=devices) if devices else fg.PolynomialRing(n, q)
        be = fg.BootstrapEngine(r, 4, 1, 1)
        for rf, negate in ((ref, True), (one, False), (None, True)):
            want_a, want_b = expected(q, ct, rf, negate, slots, offsets)
            a, b = be.slot_extract(ct, slots, offsets, rf, negate)  # host arrays
            assert isinstance(a, np.ndarray) and (a == want_a).all() and (b == want_b).all(), (devices, negate)
        if devices:  # a device tensor on a multi-device context runs where it lives
            a, b = be.slot_extract(D(ct), slots, offsets, D(ref), False)
            want_a, want_b = expected(q, ct, ref, False, slots, offsets)
            assert (H(a) == want_a).all() and (H(b) == want_b).all()


def test_slot_extract_argument_errors(fg):
    n, q, batch = 256, 7681, 3
    r = fg.PolynomialRing(n, q)
    be = fg.BootstrapEngine(r, 4, 1, 1)
    ct = D(raw_cts(1, q, (batch, 2, n)))
    with pytest.raises(fg.FHEError, match="slot index out of range") as e:
        be.slot_extract(ct, [0, n])
    assert e.value.code == -9
    with pytest.raises(fg.FHEError, match="ciphertext shapes differ"):
        be.slot_extract(ct, [0], ref=D(raw_cts(2, q, (2, 2, n))))
    # the library's own checks, on device pointers
    import ctypes as C

    ref = D(raw_cts(3, q, (2, 2, n)))
    a, b = D(np.zeros((batch, 1, n), np.uint64)), D(np.zeros((batch, 1), np.uint64))
    slot0 = (C.c_uint32 * 1)(0)

    def call(ct_p, ref_p, ref_count, a_p, b_p):
        rc = fg.lib().fhe_slot_extract_batch(r._h, ct_p, ref_p, ref_count, 0, slot0, None, 1, a_p, b_p, batch, fg.FHE_DEVICE)
        assert rc == -9, rc
        return fg.lib().fhe_last_error().decode()

    assert "ref_count must be 0, 1 or the batch size" in call(ct.data_ptr(), ref.data_ptr(), 2, a.data_ptr(), b.data_ptr())
    # an output inside the input ciphertexts, or inside the reference
    assert "overlap" in call(ct.data_ptr(), None, 0, ct.data_ptr() + 8 * n, b.data_ptr())
    assert "overlap" in call(ct.data_ptr(), None, 0, a.data_ptr(), ct.data_ptr() + 8 * (batch * 2 * n - 1))
    assert "overlap" in call(ct.data_ptr(), ref.data_ptr(), 1, a.data_ptr(), ref.data_ptr() + 8)
    torch_sync = H(ct)  # nothing ran: the inputs are untouched
    assert (torch_sync == raw_cts(1, q, (batch, 2, n))).all()


def test_slot_extract_is_the_coefficient_of_the_phase(fg):
    n, q, t, batch = 1024, P27, 16, 3
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    be = fg.BootstrapEngine(r, 4, 1, 1)
    rng = np.random.default_rng(2026)
    s = rng.integers(-1, 2, size=n).astype(np.int64)
    key = fg.SecretKey(r, D(np.where(s < 0, q - 1, s).astype(np.uint64)))
    ct = rng.integers(0, q, size=(batch, 2, n), dtype=np.uint64)
    phase = H(eng.decrypt(D(ct), key, with_phase=True).phase)
    slots = [0, n - 1, n // 2, 5, 700]
    a, b = be.slot_extract(D(ct), slots)
    _, ph = fg.lwe_decrypt(q, t, D(s), a.reshape(-1, n), b.reshape(-1))
    assert (H(ph).reshape(batch, len(slots)) == phase[:, slots]).all()
    # and of the difference with a reference
    ref = rng.integers(0, q, size=(batch, 2, n), dtype=np.uint64)
    diff = H(eng.decrypt(r.subtract(D(ct), D(ref)), key, with_phase=True).phase)
    a, b = be.slot_extract(D(ct), slots, ref=D(ref))
    _, ph = fg.lwe_decrypt(q, t, D(s), a.reshape(-1, n), b.reshape(-1))
    assert (H(ph).reshape(batch, len(slots)) == diff[:, slots]).all()


@pytest.mark.parametrize("q", [2, 97, P62, Q63])
def test_lwe_sum_words(fg, q):
    rng = np.random.default_rng(q % 1000)
    for dim in (0, 1, 37, 742):
        for terms in (1, 2, 9):
            for batch in (1, 5):
                la = rng.integers(0, 1 << 64, size=(terms, batch, dim), dtype=np.uint64)
                lb = rng.integers(0, 1 << 64, size=(terms, batch), dtype=np.uint64)
                if dim:
                    la[0, 0, 0], la[-1, -1, -1] = M64, q
                lb[0, 0], lb[-1, -1] = M64, q - 1
                for off in (0, M64, int(rng.integers(0, 1 << 64, dtype=np.uint64))):
                    want_a = (la.astype(object) % q).sum(axis=0) % q
                    want_b = ((lb.astype(object) % q).sum(axis=0) + off % q) % q
                    a, b = fg.BootstrapEngine.lwe_sum(q, la, lb, off)
                    assert a.shape == (batch, dim) and b.shape == (batch,)
                    assert (a.astype(object) == want_a).all() and (b.astype(object) == want_b).all(), (q, dim, terms, batch)
    # device tensors give the same words
    la = rng.integers(0, 1 << 64, size=(9, 5, 37), dtype=np.uint64)
    lb = rng.integers(0, 1 << 64, size=(9, 5), dtype=np.uint64)
    a, b = fg.BootstrapEngine.lwe_sum(q, D(la), D(lb), M64)
    ha, hb = fg.BootstrapEngine.lwe_sum(q, la, lb, M64)
    assert (H(a) == ha).all() and (H(b) == hb).all()


def rnd(seed, q, *shape):
    return np.random.default_rng(seed).integers(0, q, size=shape, dtype=np.uint64)


@pytest.mark.parametrize("n,q,bl,lv,dim", [(256, 7681, 4, 3, 8), (1024, P62, 23, 1, 12)])
def test_comparison_pipelines_equal_the_explicit_chain(fg, n, q, bl, lv, dim):
    t, batch, slots = 16, 3, [0, 5]
    ks_bl, ks_lv = 4, 3
    r = fg.PolynomialRing(n, q)
    o = oracle.NTT(n, q)
    be = fg.BootstrapEngine(r, bl, lv, 1)
    bsk = rnd(71, q, dim, 2 * lv, 2, n)
    bsk_ntt = be.prepare_ggsw(bsk)
    ksk_a, ksk_b = rnd(72, q, n * ks_lv, dim), rnd(73, q, n * ks_lv)
    cmp_ = fg.Comparisons(r, t, bsk_ntt, ksk_a, ksk_b, bl, lv, ks_bl, ks_lv)
    delta = q // t
    half = delta // 2
    assert (cmp_.delta, cmp_.half, cmp_.dim) == (delta, half, dim)
    tp = np.full(n, half, dtype=np.uint64)
    x, y = rnd(74, q, batch, 2, n), rnd(75, q, batch, 2, n)
    zero = np.zeros_like(x)

    def sign(d, offs):
        """subtract -> rotate -> sample_extract -> body offset -> key_switch -> bootstrap, per slot"""
        glwe = np.ascontiguousarray(d[:, ::-1])
        outs = []
        for h, off in zip(slots, offs):
            a, b = be.sample_extract(be.multiply_glwe_by_monomial(glwe, [-h] * batch))
            b = np.array([(int(v) + off) % q for v in b], dtype=np.uint64)
            la, lb = fg.BootstrapEngine.key_switch(q, ks_bl, ks_lv, ksk_a, ksk_b, a, b)
            outs.append((la, lb) + be.bootstrap(la, lb, bsk_ntt, tp, ksk_a, ksk_b, ks_bl, ks_lv))
        return outs

    def add(terms, body):
        """the sum of SIGN terms per slot with a body offset, in Python integers -> (a [batch, S, dim], b [batch, S])"""
        a = np.stack([sum(tm[s][2].astype(object) for tm in terms) % q for s in range(len(slots))], axis=1)
        b = np.stack([(sum(tm[s][3].astype(object) for tm in terms) + body) % q for s in range(len(slots))], axis=1)
        return a, b

    def same(got, want):
        return (got[0].astype(object) == want[0]).all() and (got[1].astype(object) == want[1]).all()

    ge = sign(r.subtract(x, y), [half, half])
    assert same(cmp_.greater_equal(x, y, slots), add([ge], half))
    eq_neg = sign(r.subtract(y, x), [half, half])
    assert same(cmp_.equal(x, y, slots), add([ge, eq_neg], 0))
    lo, hi = 2, 6
    enc = lambda v: ((v * delta) & M64) % q
    assert cmp_.encode(hi) == enc(hi)
    rng_lo = sign(r.subtract(x, zero), [(half - enc(lo)) % q] * 2)
    rng_hi = sign(r.negate(x), [(half + enc(hi)) % q] * 2)
    assert same(cmp_.check_range(x, lo, hi, slots), add([rng_lo, rng_hi], 0))
    # device tensors give the same words
    dcmp = fg.Comparisons(r, t, D(bsk_ntt), D(ksk_a), D(ksk_b), bl, lv, ks_bl, ks_lv)
    da, db = dcmp.equal(D(x), D(y), slots)
    ha, hb = cmp_.equal(x, y, slots)
    assert (H(da) == ha).all() and (H(db) == hb).all()
    # one ciphertext of the chain against the oracle's bootstrap
    la, lb, oa, ob = ge[1]
    ea, eb = o.bootstrap(1, bl, lv, la[0], int(lb[0]), q, bsk, tp, ks_bl, ks_lv, ksk_a, ksk_b)
    assert (oa[0] == ea).all() and int(ob[0]) == eb


@pytest.mark.parametrize("n,q,t", [(1024, P27, 16), (512, 12289, 4)])
def test_truth_tables_under_zero_keys(fg, n, q, t):
    assert q * 2 * n < 1 << 64  # the reference's rotation amount b * 2n wraps above that
    assert n >= t
    bl, lv, ks_bl, ks_lv, dim = 4, 3, 4, 3, 4
    r = fg.PolynomialRing(n, q)
    be = fg.BootstrapEngine(r, bl, lv, 1)
    bsk_ntt = np.zeros((dim, 2 * lv, 2, n), np.uint64)
    ksk_a, ksk_b = np.zeros((n * ks_lv, dim), np.uint64), np.zeros(n * ks_lv, np.uint64)
    cmp_ = fg.Comparisons(r, t, D(bsk_ntt), D(ksk_a), D(ksk_b), bl, lv, ks_bl, ks_lv)
    delta = q // t
    half_t = t // 2
    slots = [0, 3, n - 1]
    vals = list(range(half_t))
    pairs = [(a, b) for a in vals for b in vals]
    assert all(v < t // 2 for v in vals)
    rng = np.random.default_rng(n)

    def encrypt(rows):
        """c0 = encode(values) (the row's value at slot 0, value + 1 and value + 2 mod t/2 at
        the other two), c1 random"""
        ct = rng.integers(0, q, size=(len(rows), 2, n), dtype=np.uint64)
        ct[:, 0] = 0
        for i, v in enumerate(rows):
            for k, h in enumerate(slots):
                ct[i, 0, h] = ((((v + k) % half_t) * delta) & M64) % q
        return ct

    def at(v, k):
        return (v + k) % half_t

    def decode(res):
        a, b = res
        v, _ = fg.lwe_decrypt(q, t, D(np.zeros(dim, np.int64)), a.reshape(-1, dim), b.reshape(-1))
        return H(v).reshape(tuple(b.shape)).astype(np.int64)

    ca, cb = D(encrypt([a for a, _ in pairs])), D(encrypt([b for _, b in pairs]))
    S = range(len(slots))
    for name, pred in (("greater_equal", lambda a, b: a >= b), ("greater_than", lambda a, b: a > b),
                       ("less_than", lambda a, b: a < b), ("equal", lambda a, b: a == b)):
        got = decode(getattr(cmp_, name)(ca, cb, slots))
        want = np.array([[int(pred(at(a, k), at(b, k))) for k in S] for a, b in pairs])
        assert (got == want).all(), name
    cv = D(encrypt(vals))
    for thr in vals:
        thrs = [thr, (thr + 1) % half_t, 0]
        got = decode(cmp_.check_threshold(cv, thrs, slots))
        assert (got == np.array([[int(at(a, k) >= thrs[k]) for k in S] for a in vals])).all(), thr
    for lo in vals:
        for hi in vals:
            if lo > hi:  # both sign terms would be -h: the sum leaves the {0, delta} encoding
                with pytest.raises(fg.FHEError, match="min <= max"):
                    cmp_.check_range(cv, lo, hi, slots)
                continue
            got = decode(cmp_.check_range(cv, lo, hi, slots))
            assert (got == np.array([[int(lo <= at(a, k) <= hi) for k in S] for a in vals])).all(), (lo, hi)
    existing_vals = [vals[-1], 0, vals[-1], 1 % half_t, vals[-1]]
    existing = [D(encrypt([e])[0]) for e in existing_vals]
    got = decode(cmp_.detect_duplicate(cv, existing, slots))
    want = np.array([[sum(at(a, k) == at(e, k) for e in existing_vals) % t for k in S] for a in vals])
    assert (got == want).all()
    za, zb = cmp_.detect_duplicate(cv, [], slots)
    assert tuple(za.shape) == (len(vals), len(slots), dim) and not H(za).any() and not H(zb).any()


def test_js_engine():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "compare_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 passed" in r.stdout
