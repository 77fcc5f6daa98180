"""Hoisted rotations on the GPU: the words of fhe_ct_hoist_batch,
fhe_ct_hoisted_galois_batch and fhe_ct_hoisted_linear_batch against the model
of tests/hoist_ref.py (numpy sigma_g and digits around the library's older
ring product) and against the chain of older entry points the header names
(poly_galois, ntt_fwd, pointwise, poly_add, ntt_inv; polymul and ct_sum for the
linear transform), on the fused path, with FHE_HOIST_FUSED=0, host resident,
and on the two composed-only contexts; g = 1 against fhe_ct_galois_batch; and
the meaning with real keys: rotate_many decodes to the rotated vectors, matvec
to M v mod t, with the derived worst-case noise bound asserted.  The word
tests never compare the new entry points with themselves."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hoist_ref as Hr
import simd_ref as S

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
QG = 18446744069414584321     # 2^64 - 2^32 + 1, a modulus above 2^62
M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS_CAP = 28  # Box-Muller on 53-bit uniforms at std_dev 3.2 (tests/test_gpu_galois.py)


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


def raw_words(seed, q, shape):
    """Full-range u64 words with 0, q - 1, q, 2q - 1 and 2^64 - 1 planted at both ends of the last axis."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = [0, q - 1, q, M64] + ([2 * q - 1] if 2 * q - 1 <= M64 else [])
    edge = np.array(edge, dtype=np.uint64)
    k = min(len(edge), shape[-1])
    a[..., :k] = edge[:k]
    if shape[-1] >= 16:
        a[..., -len(edge):] = edge[::-1]
    return a


def canonical(seed, q, shape):
    return np.random.default_rng(seed).integers(0, q, size=shape, dtype=np.uint64)


def u32(xs):
    return (C.c_uint32 * len(xs))(*xs)


def ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


class Calls:
    """The three entry points through ctypes, on device tensors or host arrays."""

    def __init__(self, fg, ring, bl, lv):
        self.fg, self.L, self.r, self.bl, self.lv, self.n = fg, fg.lib(), ring, bl, lv, ring.degree

    def _run(self, fn, bufs, call):
        dev = hasattr(bufs[0], "data_ptr")
        self.r._bind_stream(self.fg.FHE_DEVICE if dev else self.fg.FHE_HOST)
        rc = call(self.fg.FHE_DEVICE if dev else self.fg.FHE_HOST)
        assert rc == 0, (rc, self.L.fhe_last_error().decode())

    def hoist(self, ct, make):
        out = make((ct.shape[0], 1 + self.lv, self.n))
        self._run("hoist", [ct], lambda w: self.L.fhe_ct_hoist_batch(self.r._h, self.bl, self.lv, ptr(ct), ptr(out),
                                                                     ct.shape[0], w))
        return out

    def galois(self, gs, idx, key_ntt, hoisted, make):
        out = make((hoisted.shape[0], len(gs), 2, self.n))
        self._run("galois", [hoisted], lambda w: self.L.fhe_ct_hoisted_galois_batch(
            self.r._h, self.lv, len(gs), u32(gs), u32(idx) if idx is not None else None, ptr(key_ntt), ptr(hoisted),
            ptr(out), hoisted.shape[0], w))
        return out

    def linear(self, gs, idx, key_ntt, pts_ntt, hoisted, out, accumulate):
        self._run("linear", [hoisted], lambda w: self.L.fhe_ct_hoisted_linear_batch(
            self.r._h, self.lv, len(gs), u32(gs), u32(idx) if idx is not None else None, ptr(key_ntt), ptr(pts_ntt),
            ptr(hoisted), int(accumulate), ptr(out), hoisted.shape[0], w))
        return out


def dev_zeros(shape):
    return D(np.zeros(shape, np.uint64))


def host_zeros(shape):
    return np.zeros(shape, np.uint64)


# (n, q, base_log, level, batches, composed only)
WORD_SHAPES = [(16, P27, 9, 3, (1, 3, 37), False), (16, P62, 16, 4, (3,), False),
               (256, P27, 9, 3, (3, 37), False), (256, P62, 16, 4, (1, 3, 37), False),
               (4096, P27, 9, 3, (1, 3, 37), False), (4096, P62, 16, 4, (3, 37), False),
               (16384, P27, 9, 3, (3, 37), False), (16384, P62, 16, 4, (1, 3, 37), False),
               (32768, P27, 9, 3, (2,), True), (1024, QG, 16, 4, (3,), True)]


@pytest.mark.parametrize("n,q,bl,lv,batches,composed_only", WORD_SHAPES)
def test_words(fg, n, q, bl, lv, batches, composed_only, monkeypatch):
    """g in {1, 3, n + 1, 2n - 1, 3^5}, key indices repeated and out of order,
    5 and 1 rotations / terms, accumulate 0 and 1, raw u64 ciphertext words."""
    ring = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(ring)
    call = Calls(fg, ring, bl, lv)
    gs = [1, 3, n + 1, 2 * n - 1, pow(3, 5, 2 * n)]
    idx = [2, 0, 2, 1, 3]
    keys = canonical([n, 1], q, (4, lv, 2, n))
    dkeys = D(keys)
    sk = fg.SwitchKey(ring, dkeys, bl, lv, [3, 5, 7, 9])
    key_ntt = sk.key_ntt
    pts = canonical([n, 2], q, (5, n))
    pts_ntt = ring.forward_ntt(D(pts))

    def mul(a, b):  # the library's older ring product
        return H(ring.multiply(D(a), D(np.ascontiguousarray(b))))

    paths = ("",) if composed_only else ("1", "0", "")  # forced fused, forced composed, the library's own rule
    for batch in batches:
        ct = raw_words([n, batch, 3], q, (batch, 2, n))
        acc = raw_words([n, batch, 4], q, (batch, 2, n))
        rows = Hr.hoist_rows(q, bl, lv, ct)
        want_h = H(ring.forward_ntt(D(rows.reshape(-1, n)))).reshape(batch, 1 + lv, n)
        want_g = Hr.hoisted_galois(q, bl, lv, gs, idx, keys, ct, mul)
        want_l = {a: Hr.hoisted_linear(q, want_g, pts, mul, acc if a else None) for a in (0, 1)}
        for fused in paths:
            if fused:
                monkeypatch.setenv("FHE_HOIST_FUSED", fused)
            else:
                monkeypatch.delenv("FHE_HOIST_FUSED", raising=False)
            hoisted = call.hoist(D(ct), dev_zeros)
            assert (H(hoisted) == want_h).all(), (batch, fused, "hoist")
            hoisted = D(want_h)  # each call is checked from the reference's rows
            assert (H(call.galois(gs, idx, key_ntt, hoisted, dev_zeros)) == want_g).all(), (batch, fused, "galois")
            for a in (0, 1):
                out = D(acc) if a else dev_zeros((batch, 2, n))
                got = H(call.linear(gs, idx, key_ntt, pts_ntt, hoisted, out, a))
                assert (got == want_l[a]).all(), (batch, fused, "linear", a)
        monkeypatch.delenv("FHE_HOIST_FUSED", raising=False)
        if batch != 3:
            continue
        # host resident, staged
        hkey, hpts = H(key_ntt), H(pts_ntt)
        assert (call.hoist(ct, host_zeros) == want_h).all()
        assert (call.galois(gs, idx, hkey, want_h, host_zeros) == want_g).all()
        assert (call.linear(gs, idx, hkey, hpts, want_h, acc.copy(), 1) == want_l[1]).all()
        # one rotation / one term, the identity key index
        one = Hr.hoisted_galois(q, bl, lv, [3], [0], keys, ct, mul)
        assert (H(call.galois([3], None, key_ntt, D(want_h), dev_zeros)) == one).all()
        got = H(call.linear([3], None, key_ntt, pts_ntt, D(want_h), dev_zeros((batch, 2, n)), 0))
        assert (got == Hr.hoisted_linear(q, one, pts[:1], mul)).all()
        # g = 1 is fhe_ct_galois_batch(g = 1, add_input = 0), word for word
        rekey = fg.SwitchKey(ring, dkeys[idx[0]], bl, lv, 1)
        assert (H(eng.apply_galois(D(ct), rekey, False)) == want_g[:, 0]).all()
        # the chain of older entry points the header names
        fk = H(ring.forward_ntt(D(keys.reshape(-1, n)))).reshape(4, lv, 2, n)
        for r, (g, ki) in enumerate(zip(gs, idx)):
            f = ring.forward_ntt(ring.galois(D(rows.reshape(-1, n)), g)).reshape(batch, 1 + lv, n)
            s0, s1 = f[:, 0].contiguous(), None
            for l in range(lv):
                d = f[:, 1 + l].contiguous()
                t0 = ring.pointwise_multiply(d, D(np.broadcast_to(fk[ki, l, 1], (batch, n))))
                t1 = ring.pointwise_multiply(d, D(np.broadcast_to(fk[ki, l, 0], (batch, n))))
                s0 = ring.add(s0, t0)
                s1 = t1 if s1 is None else ring.add(s1, t1)
            assert (H(ring.inverse_ntt(s0)) == want_g[:, r, 0]).all(), (r, g)
            assert (H(ring.inverse_ntt(s1)) == want_g[:, r, 1]).all(), (r, g)
        # linear = hoisted_galois + polymul + fhe_ct_sum_batch
        prods = ring.multiply(D(want_g), D(np.ascontiguousarray(np.broadcast_to(pts[None, :, None, :], want_g.shape))))
        assert (H(ring.sum_batch(prods, grouped=True)) == want_l[0]).all()


@pytest.mark.parametrize("n,q,bl,lv", [(16, P27, 9, 3), (256, P62, 16, 4)])
def test_more_than_one_table_chunk(fg, n, q, bl, lv, monkeypatch):
    """70 and 130 rotations / terms: the (g, key index) table reaches the device in
    chunks of 64 entries, so these counts take two and three chunks, the last one partial."""
    ring = fg.PolynomialRing(n, q, mode="negacyclic")
    call = Calls(fg, ring, bl, lv)
    batch = 3
    keys = canonical([n, 11], q, (5, lv, 2, n))
    key_ntt = fg.SwitchKey(ring, D(keys), bl, lv, [3, 5, 7, 9, 11]).key_ntt
    ct = raw_words([n, 12], q, (batch, 2, n))
    acc = raw_words([n, 13], q, (batch, 2, n))

    def mul(a, b):
        return H(ring.multiply(D(a), D(np.ascontiguousarray(b))))

    for count in (70, 130):
        gs = [(2 * (3 * i + i // 64 + 1) + 1) % (2 * n) for i in range(count)]  # odd; entry 64 + i differs from entry i
        idx = [(3 * i + 1) % 5 for i in range(count)]
        assert all(gs[64 + i] != gs[i] for i in range(count - 64)) and idx[64] != idx[0]
        pts = canonical([n, 14, count], q, (count, n))
        pts_ntt = ring.forward_ntt(D(pts))
        hoisted = D(H(ring.forward_ntt(D(Hr.hoist_rows(q, bl, lv, ct).reshape(-1, n)))).reshape(batch, 1 + lv, n))
        want_g = Hr.hoisted_galois(q, bl, lv, gs, idx, keys, ct, mul)
        want_l = Hr.hoisted_linear(q, want_g, pts, mul, acc)
        for fused in ("1", "0"):
            monkeypatch.setenv("FHE_HOIST_FUSED", fused)
            assert (H(call.galois(gs, idx, key_ntt, hoisted, dev_zeros)) == want_g).all(), (count, fused)
            assert (H(call.linear(gs, idx, key_ntt, pts_ntt, hoisted, D(acc), 1)) == want_l).all(), (count, fused)
        monkeypatch.delenv("FHE_HOIST_FUSED")
        # the identity key index beyond the first chunk: key block r for rotation r
        wide = canonical([n, 15], q, (count, lv, 2, n))
        wide_ntt = fg.SwitchKey(ring, D(wide), bl, lv, gs).key_ntt
        want = Hr.hoisted_galois(q, bl, lv, gs, list(range(count)), wide, ct, mul)
        assert (H(call.galois(gs, None, wide_ntt, hoisted, dev_zeros)) == want).all(), count


# ---- meaning ------------------------------------------------------------------
def test_meaning_with_real_keys(fg):
    """t = 257 = 1 (mod 2n) admits n <= 128, so the device model runs at
    (128, the 62-bit prime, t = 257, 2^16 x 4), the largest degree of that
    plaintext modulus.  Bounds: a fresh ciphertext carries at most 28 (2 n + 1),
    a hoisted key switch adds at most level n (2^16 - 1) 28, a negated or
    wrapped message coefficient moves the phase by q mod t < t; a plaintext
    product multiplies by at most n (t / 2) and the D terms add up."""
    n, q, t, bl, lv, batch, Dm = 128, P62, 257, 16, 4, 3, 16
    half = n // 2
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    kg = fg.KeyGenerator(r, seed=20261021)
    s = kg.secret_key(1)
    sk, pk = fg.SecretKey(r, s), fg.PublicKey(r, kg.public_key(s, 2))
    steps = list(range(1, Dm)) + [half - 1]
    keys = kg.rotation_keys_for(s, steps, bl, lv, 100)
    assert keys.key.shape == (len(steps), lv, 2, n) and keys.g == [S.rotation_element(n, st) for st in steps]
    switch = lv * n * ((1 << bl) - 1) * GAUSS_CAP
    fresh = GAUSS_CAP * (2 * n + 1)
    rot_bound = fresh + switch + t
    lin_bound = Dm * n * (t // 2) * (fresh + switch + t)
    assert lin_bound < q // (2 * t)
    rng = np.random.default_rng(20261021)
    vec = rng.integers(0, t, size=(batch, Dm), dtype=np.uint64)
    v = np.tile(vec, (1, n // Dm))
    ct = eng.encrypt_sampled(eng.encode_simd(v), pk, 20261021, 100)
    hoisted = eng.hoist(ct, bl, lv)
    many = [1, 5, Dm - 1, half - 1]
    rots = eng.rotate_many(hoisted, many, keys)
    assert rots.shape == (batch, len(many), 2, n)
    for i, st in enumerate(many):
        res = eng.decrypt_simd(np.ascontiguousarray(rots[:, i]), sk)
        assert (res.values == v[:, np.array(S.rotate(list(range(n)), st))]).all(), st
        print("rotate", st, "max_noise", np.asarray(res.max_noise).tolist(), "bound", rot_bound)
        assert (np.asarray(res.max_noise).astype(object) <= rot_bound).all()
    # on the device: the same words
    dkeys = fg.SwitchKey(r, D(keys.key), bl, lv, keys.g)
    assert (H(eng.rotate_many(D(ct), many, dkeys)) == rots).all()
    # the matrix
    M = rng.integers(0, t, size=(Dm, Dm), dtype=np.int64)
    want = (M.astype(object) @ vec.astype(object).T % t).T.astype(np.uint64)
    for got in (eng.matvec(ct, M, keys), H(eng.matvec(D(ct), M, dkeys))):
        res = eng.decrypt_simd(got, sk)
        assert (res.values == np.tile(want, (1, n // Dm))).all()
        print("matvec max_noise", np.asarray(res.max_noise).tolist(), "bound", lin_bound)
        assert (np.asarray(res.max_noise).astype(object) <= lin_bound).all()
    # a missing step is refused
    with pytest.raises(fg.FHEError, match="no key for rotation step"):
        eng.rotate_many(hoisted, [Dm + 1], keys)


def test_errors_that_need_a_context(fg):
    n, q, bl, lv = 256, P27, 9, 3
    L = fg.lib()
    dev = fg.FHE_DEVICE

    def err(rc, code=-9):
        assert rc == code, rc
        return L.fhe_last_error().decode()

    ct = D(raw_words(1, q, (2, 2, n)))
    hoisted = dev_zeros((2, 1 + lv, n))
    key = D(canonical(2, q, (2, lv, 2, n)))
    pts = D(canonical(3, q, (2, n)))
    out = dev_zeros((2, 2, 2, n))
    lout = dev_zeros((2, 2, n))
    g2 = u32([3, 5])

    def gal(ring, gs, idx, o=None):
        return L.fhe_ct_hoisted_galois_batch(ring._h, lv, 2, gs, idx, key.data_ptr(), hoisted.data_ptr(),
                                             o if o is not None else out.data_ptr(), 2, dev)

    def lin(ring, gs, idx, o=None):
        return L.fhe_ct_hoisted_linear_batch(ring._h, lv, 2, gs, idx, key.data_ptr(), pts.data_ptr(), hoisted.data_ptr(), 0,
                                             o if o is not None else lout.data_ptr(), 2, dev)

    compat = fg.PolynomialRing(n, q, mode="compat")
    multi = fg.PolynomialRing(n, q, mode="negacyclic", devices=[0, 0])
    for ring, text in ((compat, "FHE_MODE_NEGACYCLIC"), (multi, "single-device")):
        assert text in err(L.fhe_ct_hoist_batch(ring._h, bl, lv, ct.data_ptr(), hoisted.data_ptr(), 2, dev), -10)
        assert text in err(gal(ring, g2, None), -10)
        assert text in err(lin(ring, g2, None), -10)
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    assert err(gal(r, u32([3, 4]), None)) == "Galois element must be odd"
    assert err(gal(r, u32([3, 2 * n + 1]), None)) == "Galois element out of range"
    assert err(lin(r, u32([2 * n + 1, 4]), None)) == "Galois element must be odd"  # parity first
    assert err(lin(r, u32([3, 2 * n + 1]), None)) == "Galois element out of range"
    assert err(gal(r, g2, u32([0, n]))) == "key index out of range"
    assert err(lin(r, g2, u32([n + 7, 0]))) == "key index out of range"
    assert "overlap" in err(gal(r, g2, None, o=hoisted.data_ptr() + 16))
    assert "overlap" in err(lin(r, g2, None, o=key.data_ptr()))
    assert "overlap" in err(lin(r, g2, None, o=pts.data_ptr()))
    assert "overlap" in err(L.fhe_ct_hoist_batch(r._h, bl, lv, ct.data_ptr(), ct.data_ptr() + 8 * n, 1, dev))
    assert "16-byte aligned" in err(L.fhe_ct_hoist_batch(r._h, bl, lv, ct.data_ptr() + 8, hoisted.data_ptr(), 1, dev))
    assert "where must be" in err(L.fhe_ct_hoist_batch(r._h, bl, lv, ct.data_ptr(), hoisted.data_ptr(), 1, 7))
    assert not H(hoisted).any() and not H(out).any() and not H(lout).any()  # nothing ran


def test_js_engine():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "hoist_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 passed" in r.stdout
