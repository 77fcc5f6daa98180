"""SIMD batching on the GPU: the words of fhe_simd_encode_batch /
fhe_simd_decode_batch against the chain (numpy scatter by the model's k(s),
then the batched transforms of a negacyclic (n, t) context), against the
composed path and, at n <= 64, against the Horner model; the laws on the
device (round trip, slot-wise product, rotation); fhe_ct_galois_chain_batch
against repeated apply_galois calls; and the meaning with real keys: rotations,
slot sums and the encrypted inner product decode to what the model says, with
the worst-case noise bounds of tests/test_gpu_galois.py asserted."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import simd_ref as S
from ntt_primes import prime_above

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
P62B = 4611686018425815041    # another prime below 2^62, = 1 mod 2^17
QG = 18446744069414584321     # 2^64 - 2^32 + 1
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


def raw_words(seed, t, shape):
    """Full-range u64 words with 0, t - 1, t, 2t - 1 and 2^64 - 1 planted at
    both ends of the last axis."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = [0, t - 1, t, M64] + ([2 * t - 1] if 2 * t - 1 <= M64 else [])
    edge = np.array(edge, dtype=np.uint64)
    k = min(len(edge), shape[-1])
    a[..., :k] = edge[:k]
    if shape[-1] >= 16:
        a[..., -len(edge):] = edge[::-1]
    return a


def canonical(seed, q, shape):
    return np.random.default_rng(seed).integers(0, q, size=shape, dtype=np.uint64)


def mod_t(a, t):
    return a % np.uint64(t)


def lifted(c, t, q):
    return np.where(c <= np.uint64((t - 1) // 2), c, c + np.uint64(q - t))


# (n, t, q): q any negacyclic modulus above t at that degree
CODEC_SHAPES = [(4, 17, 97), (8, 17, 97), (256, 7681, P27), (2048, 65537, P27), (16384, 65537, P27),
                (4096, P62, P62B), (16384, P62, P62B), (32768, 65537, P27), (1024, QG, None)]


@pytest.mark.parametrize("n,t,q", CODEC_SHAPES)
def test_codec_words(fg, n, t, q, monkeypatch):
    """Batches 1, 3 and 37 (multi-polynomial workgroups have an invalid tail),
    raw u64 inputs, lift 0 and 1; fused (where it exists), composed, host
    resident; the chain everywhere and the Horner model at n <= 64."""
    if q is None:
        q = prime_above(t, n)  # t >= 2^62: the main modulus sits between t and 2^64
        assert t < q <= M64
    ring = fg.PolynomialRing(n, q, mode="negacyclic")
    ref = fg.NTTProcessor(n, t, mode="negacyclic")
    enc = fg.SimdEncoder(ring, t)
    k_of = np.array(S.slot_index(n))
    assert (enc.slot_index() == k_of).all()
    assert enc.info["psi"] == ref.primitive_root and enc.info["wordBits"] == (32 if t < 1 << 30 else 64)
    assert (enc.info["q"], enc.info["t"], enc.info["n"]) == (q, t, n)
    for batch in (1, 3, 37):
        vals = raw_words([n, batch, 1], t, (batch, n))
        polys = raw_words([n, batch, 2], t, (batch, n))
        X = np.zeros_like(vals)
        X[:, k_of] = mod_t(vals, t)
        want_enc = ref.inverse_ntt(X)
        want_dec = np.ascontiguousarray(ref.forward_ntt(polys)[:, k_of])
        assert (want_enc < t).all() and (want_dec < t).all()
        for fused in ("1", "0"):
            monkeypatch.setenv("FHE_SIMD_FUSED", fused)
            assert (H(enc.encode(D(vals))) == want_enc).all(), (batch, fused)
            assert (H(enc.encode(D(vals), lift=True)) == lifted(want_enc, t, q)).all(), (batch, fused)
            assert (H(enc.decode(D(polys))) == want_dec).all(), (batch, fused)
        monkeypatch.delenv("FHE_SIMD_FUSED")
        if batch == 3:  # host residence, staged
            assert (enc.encode(vals, lift=True) == lifted(want_enc, t, q)).all()
            assert (enc.decode(polys) == want_dec).all()
        if n <= 64 and batch == 3:
            psi = enc.info["psi"]
            for row, e, d in zip(range(batch), want_enc, want_dec):
                assert S.encode(vals[row].tolist(), t, psi) == e.tolist()
                assert S.decode(polys[row].tolist(), t, psi) == d.tolist()
    # a short vector is zero-padded
    short = np.arange(1, 4, dtype=np.uint64)
    full = np.zeros(n, np.uint64)
    full[:3] = short
    assert (enc.encode(short) == enc.encode(full)).all()
    enc.close()


@pytest.mark.parametrize("n,t", [(2048, 65537), (256, 7681)])
def test_laws_on_the_device(fg, n, t):
    ring = fg.PolynomialRing(n, P27, mode="negacyclic")
    tring = fg.PolynomialRing(n, t, mode="negacyclic")
    enc = fg.SimdEncoder(ring, t)
    half = n // 2
    v, w = raw_words([n, 5], t, (3, n)), raw_words([n, 6], t, (3, n))
    mv, mw = enc.encode(D(v)), enc.encode(D(w))
    assert (H(enc.decode(mv)) == mod_t(v, t)).all()
    prod = (mod_t(v, t).astype(object) * mod_t(w, t).astype(object) % t).astype(np.uint64)
    assert (H(enc.decode(tring.multiply(mv, mw))) == prod).all()
    for steps in (1, -1, half - 1):
        for swap in (False, True):
            g = fg.rotation_element(n, steps, swap)
            idx = np.array(S.rotate(list(range(n)), steps, swap))
            assert (H(enc.decode(tring.galois(mv, g))) == mod_t(v, t)[:, idx]).all(), (steps, swap)


CHAIN_SHAPES = [(256, P62, 16, 4, 8), (16384, P27, 9, 3, 2), (32768, P27, 9, 3, 2)]


@pytest.mark.parametrize("n,q,bl,lv,steps", CHAIN_SHAPES)
def test_chain_words_equal_repeated_calls(fg, n, q, bl, lv, steps):
    batch = 2
    ct = raw_words([n, 7], q, (batch, 2, n))
    keys = canonical([n, 8], q, (steps, lv, 2, n))
    gs = S.slot_sum_elements(n)[:steps - 1] + [2 * n - 1]
    idx = [(3 * i + 1) % steps for i in range(steps)]
    idx[-1] = idx[0]  # repeats and reorders
    for mode in (("negacyclic", "compat") if n == 256 else ("negacyclic",)):
        r = fg.PolynomialRing(n, q, mode=mode)
        eng = fg.EncryptionEngine(r)
        dkeys = D(keys)
        ks = fg.SwitchKey(r, dkeys, bl, lv, gs)
        for add_input in (False, True):
            for key_idx in (None, idx):
                got = H(eng.galois_chain(D(ct), gs, ks, key_idx, add_input))
                x = D(ct)
                for i, g in enumerate(gs):
                    one = fg.SwitchKey(r, dkeys[key_idx[i] if key_idx else i], bl, lv, g)
                    x = eng.apply_galois(x, one, add_input)
                assert (got == H(x)).all(), (n, mode, add_input, key_idx)
        # one step is fhe_ct_galois_batch itself
        one = fg.SwitchKey(r, dkeys[1], bl, lv, 3)
        assert (H(eng.galois_chain(D(ct), [3], ks, [1], True)) == H(eng.apply_galois(D(ct), one, True))).all()


def test_chain_host_device_and_multi_device_give_the_same_words(fg):
    n, q, bl, lv, batch = 1024, P62, 16, 4, 5
    gs = [3, 2 * n - 1, 9]
    idx = [2, 0, 2]
    ct = raw_words(77, q, (batch, 2, n))
    keys = canonical(78, q, (3, lv, 2, n))
    want = {}
    for devices in (None, [0, 0]):
        r = fg.PolynomialRing(n, q, mode="negacyclic", devices=devices) if devices else fg.PolynomialRing(n, q, mode="negacyclic")
        eng = fg.EncryptionEngine(r)
        for device in (False, True):
            w = D if device else (lambda a: a)
            back = H if device else (lambda a: a)
            ks = fg.SwitchKey(r, w(keys), bl, lv, gs)
            for add_input in (False, True):
                got = back(eng.galois_chain(w(ct), gs, ks, idx, add_input))
                assert (got == want.setdefault(add_input, got)).all(), (devices, device, add_input)
    assert (want[False] != want[True]).any()


# ---- meaning ------------------------------------------------------------------
def real_keys(fg, r, bl, lv, seed):
    kg = fg.KeyGenerator(r, seed=seed)
    s = kg.secret_key(1)
    return kg, s, fg.SecretKey(r, s), fg.PublicKey(r, kg.public_key(s, 2)), fg.EvaluationKey(r, kg.eval_key(s, bl, lv, 10), bl)


def check_noise(res, bound, what):
    print(what, "max_noise", np.asarray(res.max_noise).tolist(), "bound", bound)
    assert (np.asarray(res.max_noise).astype(object) <= bound).all()


def test_meaning_with_real_keys(fg):
    """n = 64, the 62-bit prime, t = 257, base 2^16 x 4.  Bounds: a fresh
    ciphertext carries |e1 + e u + e2 s| <= 28 (2 n + 1); a key switch adds at
    most level n (2^base_log - 1) 28; a negated or wrapped message coefficient
    moves the phase by q mod t < t per step."""
    n, q, t, bl, lv, batch = 64, P62, 257, 16, 4, 3
    half, k = n // 2, 6
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    kg, s, sk, pk, ek = real_keys(fg, r, bl, lv, 20261021)
    keys = kg.rotation_keys(s, bl, lv, 100)
    assert keys.key.shape == (k, lv, 2, n) and keys.g == S.slot_sum_elements(n)
    step_bound = lv * n * ((1 << bl) - 1) * GAUSS_CAP + t
    fresh = GAUSS_CAP * (2 * n + 1) + t
    sum_bound = (1 << k) * fresh + ((1 << k) - 1) * step_bound
    assert sum_bound < q // (2 * t)
    rng = np.random.default_rng(20261021)
    v = rng.integers(0, t, size=(batch, n), dtype=np.uint64)
    w = rng.integers(0, t, size=(batch, n), dtype=np.uint64)
    cv = eng.encrypt_sampled(eng.encode_simd(v), pk, 20261021, 100)
    cw = eng.encrypt_sampled(eng.encode_simd(w), pk, 20261021, 200)
    res = eng.decrypt_simd(cv, sk)
    assert (res.values == v).all()
    check_noise(res, fresh, "fresh")
    for steps in (1, -1, 5, half - 1):
        switches = bin(steps % half).count("1")
        res = eng.decrypt_simd(eng.rotate_rows(cv, steps, keys), sk)
        assert (res.values == v[:, np.array(S.rotate(list(range(n)), steps))]).all(), steps
        check_noise(res, switches * step_bound + fresh, "rotate_rows %d" % steps)
    res = eng.decrypt_simd(eng.rotate_columns(cv, keys), sk)
    assert (res.values == v[:, np.array(S.rotate(list(range(n)), 0, True))]).all()
    check_noise(res, step_bound + fresh, "rotate_columns")
    assert (eng.decrypt_simd(eng.rotate_rows(cv, half, keys), sk).values == v).all()  # a full turn
    # on the device too
    dkeys = fg.SwitchKey(r, D(keys.key), bl, lv, keys.g)
    got = eng.rotate_rows(D(cv), 5, dkeys)
    assert (H(got) == eng.rotate_rows(cv, 5, keys)).all()
    # slot sums
    total = (v.astype(object).sum(axis=1) % t).astype(np.uint64)
    res = eng.decrypt_simd(eng.sum_slots(cv, keys), sk)
    assert (res.values == total[:, None]).all()
    check_noise(res, sum_bound, "sum_slots")
    rows = eng.decrypt_simd(eng.sum_slots(cv, keys, rows_only=True), sk).values
    for rr in range(2):
        want = (v[:, rr * half:(rr + 1) * half].astype(object).sum(axis=1) % t).astype(np.uint64)
        assert (rows[:, rr * half:(rr + 1) * half] == want[:, None]).all()
    # the encrypted inner product
    ip = ((v.astype(object) * w.astype(object)).sum(axis=1) % t).astype(np.uint64)
    res = eng.decrypt_simd(eng.inner_product_scaled(cv, cw, ek, keys), sk)
    assert (res.values == ip[:, None]).all()
    assert (np.asarray(res.max_noise).astype(object) * 4 < q // (2 * t)).all()


def test_slot_wise_product_at_t_65537(fg):
    """(1024, P62, 65537, 2^16 x 4), the parameter set whose product noise
    tests/test_scaled_abi.py bounds."""
    n, q, t, bl, lv = 1024, P62, 65537, 16, 4
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    kg, s, sk, pk, ek = real_keys(fg, r, bl, lv, 20261022)
    rng = np.random.default_rng(n)
    v = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    w = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    cv = eng.encrypt_sampled(eng.encode_simd(v), pk, 20261022, 100)
    cw = eng.encrypt_sampled(eng.encode_simd(w), pk, 20261022, 200)
    res = eng.decrypt_simd(eng.multiply_relin_scaled(cv, cw, ek), sk)
    assert (res.values == (v.astype(object) * w.astype(object) % t).astype(np.uint64)).all()
    assert (np.asarray(res.max_noise).astype(object) * 4 < q // (2 * t)).all()
    # multiply_plain with the lifted encoding multiplies slot by slot as well
    res = eng.decrypt_simd(eng.multiply_plain(cv, eng.encode_simd(w, lift=True)), sk)
    assert (res.values == (v.astype(object) * w.astype(object) % t).astype(np.uint64)).all()


def test_errors_that_need_a_context(fg):
    n, q, t = 256, P27, 7681
    L = fg.lib()
    h = C.c_void_p()

    def err(rc, code=-9):
        assert rc == code, rc
        return L.fhe_last_error().decode()

    compat = fg.PolynomialRing(n, q, mode="compat")
    assert "FHE_MODE_NEGACYCLIC" in err(L.fhe_simd_ctx_create(compat._h, t, C.byref(h)), -10)
    multi = fg.PolynomialRing(n, q, mode="negacyclic", devices=[0, 0])
    assert "single-device" in err(L.fhe_simd_ctx_create(multi._h, t, C.byref(h)), -10)
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    for bad in (0, 1, 2, q, q + 2, M64):
        assert "3 <= t < q" in err(L.fhe_simd_ctx_create(r._h, bad, C.byref(h))), bad
    # the inner context's own answers, unchanged
    assert err(L.fhe_simd_ctx_create(r._h, 7680, C.byref(h)), -3) == "Modulus must be odd"
    assert "not NTT-friendly" in err(L.fhe_simd_ctx_create(r._h, 257, C.byref(h)), -4)  # 257 = 1 mod 256 only
    assert h.value is None
    with pytest.raises(fg.FHEError, match="NTT-friendly"):
        fg.SimdEncoder(r, 257)
    enc = fg.SimdEncoder(r, t)
    buf = D(raw_words(1, t, (4, n)))
    out = D(np.zeros((4, n), np.uint64))
    dev = fg.FHE_DEVICE
    assert "overlap" in err(L.fhe_simd_encode_batch(enc._h, buf.data_ptr(), 0, buf.data_ptr() + 8 * n, 3, dev))
    assert "overlap" in err(L.fhe_simd_decode_batch(enc._h, buf.data_ptr(), buf.data_ptr(), 1, dev))
    assert "16-byte aligned" in err(L.fhe_simd_encode_batch(enc._h, buf.data_ptr() + 8, 0, out.data_ptr(), 1, dev))
    assert "where must be" in err(L.fhe_simd_decode_batch(enc._h, buf.data_ptr(), out.data_ptr(), 1, 7))
    # a bad element anywhere in a chain stops it before any launch
    bl, lv = 9, 3
    ct, key = D(raw_words(2, q, (2, 2, n))), D(canonical(3, q, (2, lv, 2, n)))
    cout = D(np.zeros((2, 2, n), np.uint64))
    gs = (C.c_uint32 * 2)(3, 2 * n + 1)
    assert err(L.fhe_ct_galois_chain_batch(r._h, bl, lv, 2, gs, None, key.data_ptr(), ct.data_ptr(), 0, cout.data_ptr(),
                                           2, dev)) == "Galois element out of range"
    gs = (C.c_uint32 * 2)(3, 5)
    assert "overlap" in err(L.fhe_ct_galois_chain_batch(r._h, bl, lv, 2, gs, None, key.data_ptr(), ct.data_ptr(), 0,
                                                        ct.data_ptr() + 8 * n, 1, dev))
    assert not H(out).any() and not H(cout).any()  # nothing ran
    eng = fg.EncryptionEngine(r, t)
    with pytest.raises(fg.FHEError, match="out of range"):
        eng.galois_chain(ct, [3, 2 * n + 1], fg.SwitchKey(r, key, bl, lv, [3, 5]))


def test_js_engine():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "simd_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 passed" in r.stdout
