"""Galois automorphisms, ciphertext key switching and the trace on the GPU
(fhe_poly_galois_batch, fhe_switch_key_generate, fhe_ct_galois_batch,
fhe_ct_trace_batch and their Python bindings):

- the words of the fused key switch against the formula of include/fhe_gpu.h
  (tests/galois_ref.py over exact, GPU-independent ring products) and against
  the chain of existing entry points (galois x 2, add, relinearize), in both
  modes, with raw u64 words in the ciphertexts, batch 3;
- the composed shapes (n > 16384, q >= 2^63) against the chain;
- sigma_g against numpy; the keys against their chain; the trace against its
  chain of calls;
- the meaning, with Gaussian keys from KeyGenerator: apply_galois decrypts to
  sigma_g of the values, rekey decrypts under the second key, the trace and
  isolate_slot keep the promised slots -- each after asserting its worst-case
  noise bound;
- the pipeline: packed comparison bits, one slot isolated, opened by trustees;
- host, device and multi-device contexts, the argument errors that need a
  context, and the JS engine (tests/js/galois_test.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import galois_ref as R
import oracle
from ntt_primes import prime_above
from oracle import pyref

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
QG = 18446744069414584321     # 2^64 - 2^32 + 1
M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q63 = prime_above(1 << 63, 2048)
GAUSS_CAP = 28  # Box-Muller on 53-bit uniforms at std_dev 3.2: |x| <= 3.2 sqrt(2 * 53 ln 2) < 28


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
    """Full-range u64 words with 0, q - 1, q, 2^64 - 1 planted at both ends of
    the last axis (as raw_words of tests/test_gpu_pack.py)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    k = min(4, shape[-1])
    a[..., :k] = edge[:k]
    if shape[-1] >= 8:
        a[..., -4:] = edge[::-1]
    return a


def canonical(seed, q, shape):
    return np.random.default_rng(seed).integers(0, q, size=shape, dtype=np.uint64)


def elements(n):
    return sorted({1, 3, n // 2 + 1, n + 1, 2 * n - 1, 5 ** 7 % (2 * n)})


def exact_products(n, q):
    """The two ring products without the GPU: the oracle's transforms (compat)
    and one big-integer multiplication per row (the true ring product)."""
    ref = oracle.NTT(n, q)

    def nega(a, b):
        return np.array([pyref.negacyclic_multiply(x.tolist(), y.tolist(), q) for x, y in zip(a, b)], dtype=np.uint64)

    return {"compat": lambda a, b: ref.polymul(np.ascontiguousarray(a), np.ascontiguousarray(b)), "negacyclic": nega}


def chain(fg, r, eng, bl, g, ek, ct, add_input):
    """The chain of existing entry points on host arrays: sigma_g of both
    components, the add, relinearisation of (sigma(c0) [+ c0], [c1 | 0], sigma(c1))."""
    s = r.galois(ct, g)
    row0 = r.add(s[:, 0], ct[:, 0]) if add_input else s[:, 0]
    row1 = r.galois(ct[:, 1], 1) if add_input else np.zeros_like(s[:, 1])
    ct3 = np.ascontiguousarray(np.stack([row0, row1, s[:, 1]], axis=1))
    return eng.relinearize(ct3, ek)


WORD_SHAPES = [(4, 97, 2, 4), (256, 7681, 5, 3), (1024, P27, 7, 4), (4096, P62, 16, 4), (16384, P27, 9, 3),
               (16384, P62, 21, 3)]


@pytest.mark.parametrize("n,q,bl,lv", WORD_SHAPES)
def test_key_switch_words(fg, n, q, bl, lv):
    """Batch 3 (a multi-polynomial workgroup has an invalid tail), every g of
    elements(n), add_input 0 and 1, both modes.  The chain everywhere; the
    formula over exact products for every g below n = 4096, and from there on
    (the exact products are the cost) for g = 3 and 5^7 mod 2n in compat mode
    and for 5^7 mod 2n with add_input = 1 in negacyclic mode."""
    batch = 3
    ct = raw_words([n, 1], q, (batch, 2, n))
    key = canonical([n, 2], q, (lv, 2, n))
    mul = exact_products(n, q)
    for mode in ("compat", "negacyclic"):
        r = fg.PolynomialRing(n, q, mode=mode)
        eng = fg.EncryptionEngine(r)
        ek = fg.EvaluationKey(r, key, bl)
        sk = fg.SwitchKey(r, D(key), bl, lv)
        dct = D(ct)
        for g in elements(n):
            sk.g = g
            for add_input in (0, 1):
                got = H(eng.apply_galois(dct, sk, bool(add_input)))
                assert (got < np.uint64(q)).all()
                assert (got == chain(fg, r, eng, bl, g, ek, ct, add_input)).all(), (n, q, mode, g, add_input, "chain")
                odd = 5 ** 7 % (2 * n)
                if n < 4096 or (mode == "compat" and g in (3, odd)) or (g == odd and add_input):
                    want = R.ct_galois(q, bl, lv, g, key, ct, add_input, mul[mode])
                    assert (got == want).all(), (n, q, mode, g, add_input, "formula")
        assert (H(dct) == ct).all()  # the input is not written
    if n == 4:  # word by word in Python integers
        for g in elements(n):
            want = [R.ct_galois_int(q, bl, lv, g, key.tolist(), c.tolist(), 1, R.negacyclic_schoolbook) for c in ct]
            sk.g = g
            assert H(eng.apply_galois(dct, sk, True)).tolist() == want, g


@pytest.mark.parametrize("n,q,bl", [(4, 97, 2), (1024, P27, 7), (16384, P62, 21), (32768, P27, 9)])
def test_key_switch_without_levels_copies_the_rows(fg, n, q, bl):
    batch = 3
    ct = raw_words([n, 3], q, (batch, 2, n))
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r)
    key = fg.SwitchKey(r, D(np.zeros((0, 2, n), np.uint64)), bl, 0)
    ek = fg.EvaluationKey(r, np.zeros((0, 2, n), np.uint64), bl)
    for g in (1, 3, 2 * n - 1):
        key.g = g
        for add_input in (0, 1):
            got = H(eng.apply_galois(D(ct), key, bool(add_input)))
            assert (got == R.ct_galois(q, bl, 0, g, np.zeros((0, 2, n), np.uint64), ct, add_input, None)).all(), (g, add_input)
            assert (got == chain(fg, r, eng, bl, g, ek, ct, add_input)).all(), (g, add_input)


@pytest.mark.parametrize("n,q,bl,lv", [(32768, P27, 9, 3), (1024, Q63, 16, 4)])
def test_key_switch_words_composed_shapes(fg, n, q, bl, lv):
    """n > 16384 and q >= 2^62: the permutation kernel into a temporary and the
    composed relinearisation, against the chain."""
    batch = 2
    ct = raw_words([n, 4], q, (batch, 2, n))
    key = canonical([n, 5], q, (lv, 2, n))
    for mode in ("compat", "negacyclic"):
        r = fg.PolynomialRing(n, q, mode=mode)
        eng = fg.EncryptionEngine(r)
        ek = fg.EvaluationKey(r, key, bl)
        sk = fg.SwitchKey(r, D(key), bl, lv)
        for g in (3, n + 1, 5 ** 7 % (2 * n)):
            sk.g = g
            for add_input in (0, 1):
                got = H(eng.apply_galois(D(ct), sk, bool(add_input)))
                assert (got == chain(fg, r, eng, bl, g, ek, ct, add_input)).all(), (n, q, mode, g, add_input)


@pytest.mark.parametrize("n,q", [(4, 97), (1024, QG), (65536, P27)])
def test_poly_galois_against_numpy(fg, n, q):
    r = fg.PolynomialRing(n, q)
    p = raw_words([n, 6], q, (3, n))
    gs = range(1, 2 * n, 2) if n == 4 else elements(n) + [n - 1, 2 * n - 3]
    for g in gs:
        want = R.sigma(p, g, q)
        assert (H(r.galois(D(p), g)) == want).all(), (n, q, g, "device")
        if g in (1, 3, 2 * n - 1):
            assert (r.galois(p, g) == want).all(), (n, q, g, "host")
    if n == 4:
        for g in gs:
            assert r.galois(p, g).tolist() == [R.sigma_int(row.tolist(), g, q) for row in p]
    assert (r.galois(p, 1) == p % np.uint64(q)).all()  # a copy of the reduced words


@pytest.mark.parametrize("n,q,bl,lv", [(256, P27, 7, 4), (1024, P62, 16, 4)])
def test_switch_key_equals_the_chain(fg, n, q, bl, lv):
    seed, stream = 2026, 11
    for mode in ("compat", "negacyclic"):
        r = fg.PolynomialRing(n, q, mode=mode)
        kg = fg.KeyGenerator(r, seed=seed)
        sk_to, sk_from = kg.secret_key(3), kg.secret_key(4)
        for g, src in ((1, sk_from), (n + 1, sk_to)):  # a re-keying key and a Galois key
            key = kg.switch_key(sk_to, src, bl, lv, stream, g=g)
            assert (key.base_log, key.level, key.g) == (bl, lv, g) and key.key.shape == (lv, 2, n)
            m = r.negate(r.galois(src, g))
            power = 1
            for l in range(lv):
                a = fg.sample(r, fg.SAMPLE_UNIFORM, seed, stream + 2 * l, n)
                e = fg.sample(r, fg.SAMPLE_GAUSSIAN, seed, stream + 2 * l + 1, n, 3.2)
                b = r.add(r.add(r.multiply(a, sk_to), e), r.multiply_scalar(m, power % q))
                assert (key.key[l, 0] == a).all(), (mode, g, l)
                assert (key.key[l, 1] == b).all(), (mode, g, l)
                assert e.any()
                power = ((power * (1 << bl)) & M64) % q
            again = kg.switch_key(D(sk_to), D(src), bl, lv, stream, g=g)  # one seed, one key -- on the device too
            assert (H(again.key) == key.key).all()
        assert kg.switch_key(sk_to, sk_from, bl, 0, stream).key.shape == (0, 2, n)  # level 0 writes nothing


def test_argument_errors_that_need_a_context(fg):
    import ctypes as C

    n, q, bl, lv, batch = 256, 7681, 5, 3, 3
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r)
    L = fg.lib()
    ct, key = raw_words(9, q, (batch, 2, n)), canonical(10, q, (lv, 2, n))
    dct, dkey, dout = D(ct), D(key), D(np.zeros((batch, 2, n), np.uint64))
    seed = (C.c_uint64 * 4)(1, 2, 3, 4)

    def err(rc):
        assert rc == -9, rc
        return L.fhe_last_error().decode()

    dev = fg.FHE_DEVICE
    for g in (2 * n + 1, 4 * n - 1):
        assert err(L.fhe_poly_galois_batch(r._h, g, dct.data_ptr(), dout.data_ptr(), 1, dev)) == "Galois element out of range"
        assert err(L.fhe_ct_galois_batch(r._h, bl, lv, g, dkey.data_ptr(), dct.data_ptr(), 0, dout.data_ptr(), batch,
                                         dev)) == "Galois element out of range"
        assert err(L.fhe_switch_key_generate(r._h, dct.data_ptr(), dct.data_ptr(), g, bl, lv, seed, 0, 3.2,
                                             dout.data_ptr(), dev)) == "Galois element out of range"
    with pytest.raises(fg.FHEError, match="out of range"):
        r.galois(ct, 2 * n + 1)
    assert "steps must be between" in err(L.fhe_ct_trace_batch(r._h, bl, lv, 9, dkey.data_ptr(), dct.data_ptr(),
                                                               dout.data_ptr(), batch, dev))
    words = batch * 2 * n
    assert "overlap" in err(L.fhe_poly_galois_batch(r._h, 3, dct.data_ptr(), dct.data_ptr() + 8 * (words - 1), 2 * batch, dev))
    assert "overlap" in err(L.fhe_ct_galois_batch(r._h, bl, lv, 3, dkey.data_ptr(), dct.data_ptr(), 0,
                                                  dct.data_ptr() + 8 * n, batch - 1, dev))
    assert "overlap" in err(L.fhe_ct_trace_batch(r._h, bl, lv, 1, dkey.data_ptr(), dct.data_ptr(), dct.data_ptr(), batch, dev))
    # swk overlapping either key
    assert "overlap" in err(L.fhe_switch_key_generate(r._h, dkey.data_ptr() + 8 * n, dct.data_ptr(), 3, bl, lv, seed, 0, 3.2,
                                                      dkey.data_ptr(), dev))
    assert "overlap" in err(L.fhe_switch_key_generate(r._h, dct.data_ptr(), dkey.data_ptr() + 8 * (lv * 2 * n - 1), 3, bl, lv,
                                                      seed, 0, 3.2, dkey.data_ptr(), dev))
    assert (H(dct) == ct).all() and (H(dkey) == key).all() and not H(dout).any()  # nothing ran
    with pytest.raises(fg.FHEError, match="g = 1"):
        eng.rekey(dct, fg.SwitchKey(r, dkey, bl, lv, 3))


@pytest.mark.parametrize("n,q,bl,lv,steps", [(256, P62, 16, 4, 8), (16384, P27, 9, 3, 2)])
def test_trace_words_equal_the_chain_of_calls(fg, n, q, bl, lv, steps):
    batch = 2
    ct = raw_words([n, 7], q, (batch, 2, n))
    keys = canonical([n, 8], q, (steps, lv, 2, n))
    inv = pow(pow(2, steps, q), -1, q)
    for mode in ("compat", "negacyclic"):
        r = fg.PolynomialRing(n, q, mode=mode)
        eng = fg.EncryptionEngine(r)
        gk = fg.SwitchKey(r, D(keys), bl, lv, R.trace_elements(n, steps))
        got = H(eng.trace(D(ct), gk))
        x = r.multiply_scalar(D(ct), inv)
        for i, g in enumerate(R.trace_elements(n, steps)):
            x = eng.apply_galois(x, fg.SwitchKey(r, D(keys[i]), bl, lv, g), True)
        assert (got == H(x)).all(), (n, q, mode)
        assert (H(eng.trace(D(ct), gk, steps=1)) ==
                H(eng.apply_galois(r.multiply_scalar(D(ct), pow(2, -1, q)), fg.SwitchKey(r, D(keys[0]), bl, lv, n + 1), True))).all()
        if n == 256 and mode == "negacyclic":  # and the formula over exact products
            assert (got == R.trace(q, bl, lv, steps, keys, ct, exact_products(n, q)[mode])).all()


def test_host_device_and_multi_device_give_the_same_words(fg):
    n, q, bl, lv, batch, steps = 1024, P62, 16, 4, 5, 2
    ct = raw_words(77, q, (batch, 2, n))
    keys = canonical(78, q, (steps, lv, 2, n))
    p = raw_words(79, q, (batch, n))
    want = {}
    for devices in (None, [0, 0]):
        r = fg.PolynomialRing(n, q, devices=devices) if devices else fg.PolynomialRing(n, q)
        eng = fg.EncryptionEngine(r)
        for device in (False, True):  # a device tensor on a multi-device context runs where it lives
            w = D if device else (lambda a: a)
            back = H if device else (lambda a: a)
            got = {
                "sigma": back(r.galois(w(p), 3)),
                "galois": back(eng.apply_galois(w(ct), fg.SwitchKey(r, w(keys[0]), bl, lv, 2 * n - 1), True)),
                "trace": back(eng.trace(w(ct), fg.SwitchKey(r, w(keys), bl, lv, R.trace_elements(n, steps)))),
            }
            for k, v in got.items():
                assert (v == want.setdefault(k, v)).all(), (devices, device, k)
    assert (want["sigma"] == R.sigma(p, 3, q)).all()


# ---- meaning ------------------------------------------------------------------
def encrypt(r, eng, rng, sk, msgs, q):
    """c1 uniform, c0 = c1 (*) sk + delta m + e with |e| <= 2 (the ring's own product)."""
    c1 = rng.integers(0, q, size=msgs.shape, dtype=np.uint64)
    e = rng.integers(-2, 3, size=msgs.shape)
    prod = r.multiply(c1, np.ascontiguousarray(np.broadcast_to(sk, msgs.shape)))
    c0 = (prod.astype(object) + eng.delta * msgs.astype(object) + e.astype(object)) % q
    return np.ascontiguousarray(np.stack([c0.astype(np.uint64), c1], axis=-2))


def check_noise(res, bound):
    print("max_noise", res.max_noise.tolist(), "bound", bound)
    assert (res.max_noise.astype(object) <= bound).all() and res.max_noise.all()


def test_meaning_on_the_64_bit_path(fg):
    """n = 256, the 62-bit prime, t = 257, base_log 16 x 4, Gaussian keys."""
    n, q, t, bl, lv, batch = 256, P62, 257, 16, 4, 3
    steps = 8
    assert bl * lv >= (q - 1).bit_length()
    step_bound = lv * n * ((1 << bl) - 1) * GAUSS_CAP          # one key switch: level * n * (2^base_log - 1) * max|e|
    offset = 2 + (q - (q // t) * t)                              # the input error, and q - delta t of a negated message
    trace_bound = step_bound * ((1 << steps) - 1) + offset      # step i scaled by 2^(steps - 1 - i)
    assert trace_bound < (1 << 8) * lv * (1 << 8) * (1 << 16) * GAUSS_CAP + offset < q // (2 * t)
    rng = np.random.default_rng(20261021)
    msgs = rng.integers(1, t, size=(batch, n), dtype=np.uint64)
    # Negacyclic mode only: with real keys the compat product does not keep the key-switch noise
    # small, for g = 1 either (include/fhe_gpu.h; tests/test_galois_abi.py shows it in exact integers).
    for mode in ("negacyclic",):
        r = fg.PolynomialRing(n, q, mode=mode)
        eng = fg.EncryptionEngine(r, t)
        kg = fg.KeyGenerator(r, seed=20261021)
        s1, s2 = kg.secret_key(1), kg.secret_key(2)
        sk1, sk2 = fg.SecretKey(r, s1), fg.SecretKey(r, s2)
        ct = encrypt(r, eng, rng, s1, msgs, q)
        assert (eng.decrypt(ct, sk1).values == msgs).all()
        # re-keying: under the second key and no longer under the first
        rk = kg.switch_key(s2, s1, bl, lv, 10)
        out = eng.rekey(ct, rk)
        res = eng.decrypt(out, sk2)
        assert (res.values == msgs).all(), mode
        check_noise(res, step_bound + offset)
        assert (eng.decrypt(out, sk1).values != msgs).any(), mode
        # sigma_g of the values, three g
        for i, g in enumerate((3, n + 1, 2 * n - 1)):
            gk = kg.switch_key(s1, s1, bl, lv, 20 + 2 * lv * i, g=g)
            res = eng.decrypt(eng.apply_galois(D(ct), D_key(fg, r, gk)), sk1_dev(fg, r, s1))
            assert (H(res.values) == R.sigma(msgs, g, t)).all(), g
            check_noise(res, step_bound + offset)
        # the full trace and isolate_slot
        keys = kg.galois_keys(s1, bl, lv, 100)
        assert keys.key.shape == (steps, lv, 2, n) and keys.g == R.trace_elements(n, steps) and keys.g[-1] == 3
        res = eng.decrypt(eng.trace(ct, keys), sk1)
        want = np.zeros_like(msgs)
        want[:, 0] = msgs[:, 0]
        assert (res.values == want).all()
        check_noise(res, trace_bound)
        for slot in (0, 1, n - 1):
            res = eng.decrypt(eng.isolate_slot(ct, slot, keys), sk1)
            want = np.zeros_like(msgs)
            want[:, slot] = msgs[:, slot]
            assert (res.values == want).all(), slot
            check_noise(res, trace_bound)
        # a partial trace keeps every 8th slot
        res = eng.decrypt(eng.trace(ct, keys, steps=3), sk1)
        want = np.where(np.arange(n) % 8 == 0, msgs, 0).astype(np.uint64)
        assert (res.values == want).all()
        check_noise(res, step_bound * 7 + offset)


def D_key(fg, r, key):
    return fg.SwitchKey(r, D(key.key), key.base_log, key.level, key.g)


def sk1_dev(fg, r, s):
    return fg.SecretKey(r, D(s))


def test_meaning_on_the_32_bit_path(fg):
    """n = 64, q = 132120577, t = 4, base_log 7 x 4, one Galois step."""
    n, q, t, bl, lv, batch = 64, P27, 4, 7, 4, 3
    assert bl * lv >= (q - 1).bit_length()
    offset = 2 + (q - (q // t) * t)
    bound = lv * n * ((1 << bl) - 1) * GAUSS_CAP + offset
    assert bound < q // (2 * t)  # 2^19.8 against 2^23.98
    rng = np.random.default_rng(5)
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    kg = fg.KeyGenerator(r, seed=7)
    s = kg.secret_key(1)
    msgs = rng.integers(0, t, size=(batch, n), dtype=np.uint64)
    ct = encrypt(r, eng, rng, s, msgs, q)
    for g in (3, n + 1, 5 ** 7 % (2 * n)):
        res = eng.decrypt(eng.apply_galois(ct, kg.switch_key(s, s, bl, lv, 10, g=g)), fg.SecretKey(r, s))
        assert (res.values == R.sigma(msgs, g, t)).all(), g
        check_noise(res, bound)


def test_one_packed_comparison_bit_is_isolated_and_opened_by_trustees(fg):
    """greater_equal under all-zero bootstrap keys (as
    test_comparison_bits_are_tallied_and_opened_by_trustees), packed, one slot
    isolated, opened with 3 of 5 key shares: only that slot is non-zero."""
    n, q, t = 1024, P27, 16
    bl, lv, ks_bl, ks_lv, dim = 4, 3, 4, 3, 4
    g_bl, g_lv, steps = 1, 27, 10
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    bsk_ntt = np.zeros((dim, 2 * lv, 2, n), np.uint64)
    ksk_a, ksk_b = np.zeros((n * ks_lv, dim), np.uint64), np.zeros(n * ks_lv, np.uint64)
    cmp_ = fg.Comparisons(r, t, D(bsk_ntt), D(ksk_a), D(ksk_b), bl, lv, ks_bl, ks_lv)
    delta = q // t
    slots = [0, 3, n - 1]
    va, vb = np.array([[5, 2, 7]]), np.array([[4, 6, 7]])

    def enc(vals):
        ct = np.random.default_rng(3).integers(0, q, size=(1, 2, n), dtype=np.uint64)
        ct[:, 0] = 0
        ct[:, 0, slots] = (vals * delta % q).astype(np.uint64)
        return D(ct)

    bits = cmp_.greater_equal(enc(va), enc(vb), slots)
    kg = fg.KeyGenerator(r, seed=99)
    tk = kg.threshold_keys(3, 5, 20)
    pk = kg.pack_key(tk.secret_key.poly, np.zeros(dim, np.int64), 7, 4, 30)
    packed = H(fg.Comparisons.pack(bits, slots, fg.PackKey(D(pk.key), pk.base_log, pk.level, pk.lwe_dim), eng))
    assert (eng.decrypt(packed, tk.secret_key).values[0, slots] == [1, 0, 1]).all()
    # No worst-case bound fits a 27-bit modulus here: (2^steps - 1) level n (2^base_log - 1) 28 is far
    # above q / (2 t).  The estimate instead: a key switch adds, per coefficient, level * n terms d * e
    # with bits d (E d^2 = 1/2 at base_log 1) and errors of variance 3.2^2; step i of the trace is
    # doubled steps - 1 - i times, so the variances add up with weights 4^(steps - 1 - i).  The packing
    # noise below passes through unscaled.  Twelve standard deviations must fit.
    assert g_bl * g_lv >= (q - 1).bit_length()
    sigma = (sum(4 ** k for k in range(steps)) * g_lv * n * 0.5 * 3.2 ** 2) ** 0.5
    print("trace noise sigma", sigma, "q / (2 t)", q // (2 * t),
          "worst case", ((1 << steps) - 1) * g_lv * n * ((1 << g_bl) - 1) * GAUSS_CAP)
    assert 12 * sigma < q // (2 * t)
    keys = kg.galois_keys(tk.secret_key.poly, g_bl, g_lv, 200)
    shares = tk.shares[1:4]
    for slot, bit in ((n - 1, 1), (3, 0), (0, 1)):
        one = eng.isolate_slot(packed, slot, keys)
        partials = eng.partial_decrypt(one, shares)
        res = eng.combine_partial_decryptions(one, partials, [s.share_id for s in shares])
        want = np.zeros((1, n), dtype=np.uint64)
        want[0, slot] = bit
        assert (res.values == want).all(), slot


def test_js_engine():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "galois_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 passed" in r.stdout
