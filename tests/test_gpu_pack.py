"""LWE-to-RLWE packing on the GPU (fhe_lwe_pack_batch, fhe_pack_key_generate,
EncryptionEngine.pack_lwe, Comparisons.pack):

- the packed words against the formula of include/fhe_gpu.h (tests/pack_ref.py)
  and against the chain of existing entry points (key_switch with out_dim = 2n,
  a body add, multiply_glwe_by_monomial by +slot, sum_batch), in both modes,
  with raw u64 words in the key, the masks, the bodies and `out`;
- q >= 2^63 against the formula, large degrees against the chain;
- host, device and multi-device contexts, and the argument errors;
- the key against fhe_sample_batch x 2, multiply, add and the gadget add;
- the meaning: packed LWE messages decrypt with EncryptionEngine.decrypt;
- the pipeline: comparison bits packed, tallied and opened by trustees;
- the JS engine (tests/js/pack_test.js)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pack_ref as R
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


def raw_words(seed, q, shape):
    """Full-range u64 words with 0, q - 1, q, 2^64 - 1 planted at both ends of
    the last axis (as raw_cts of tests/test_gpu_compare.py)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    k = min(4, shape[-1])
    a[..., :k] = edge[:k]
    if shape[-1] >= 8:
        a[..., -4:] = edge[::-1]
    return a


def inputs(seed, n, q, in_dim, level, batch, S):
    """key [entries, 2, n] (a quarter of every c1 row 2^64 - 1), lwe_a
    [batch, S, in_dim] (slot 1 of every ciphertext: all digits zero; slot 2:
    every digit 2^base_log - 1), lwe_b [batch, S], prev [batch, 2, n]."""
    key = raw_words([seed, 1], q, (in_dim * level, 2, n))
    key[:, 1, n // 4: n // 2] = M64
    lwe_a = raw_words([seed, 2], q, (batch, S, in_dim))
    if S > 2:
        lwe_a[:, 1] = 0
        lwe_a[:, 2] = M64
    lwe_b = raw_words([seed, 3], q, (batch, S))
    prev = raw_words([seed, 4], q, (batch, 2, n))
    return key, lwe_a, lwe_b, prev


def chain(fg, r, be, q, n, bl, lv, key, lwe_a, lwe_b, slots, prev=None):
    """The chain of existing entry points (host arrays)."""
    batch, S, in_dim = lwe_a.shape
    entries = in_dim * lv
    ka, kb = key.reshape(entries, 2 * n), np.zeros(entries, np.uint64)
    a, b = fg.BootstrapEngine.key_switch(q, bl, lv, ka, kb, lwe_a.reshape(batch * S, in_dim),
                                         np.zeros(batch * S, np.uint64))
    assert not b.any()
    a = a.reshape(batch, S, 2, n)
    Q = np.uint64(q)
    first = a[:, :, 0, 0].astype(object) + (lwe_b % Q).astype(object)
    a[:, :, 0, 0] = (first % q).astype(np.uint64)
    glwe = np.ascontiguousarray(a[:, :, ::-1]).reshape(batch * S, 2, n)  # (mask = second half, body = first half)
    rot = be.multiply_glwe_by_monomial(glwe, list(slots) * batch)
    cts = np.ascontiguousarray(rot.reshape(batch, S, 2, n)[:, :, ::-1])
    out = r.sum_batch(cts, grouped=True)
    if prev is not None:
        out = ((out.astype(object) + (prev % Q).astype(object)) % q).astype(np.uint64)
    return out


def pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev=None, device=True):
    """EncryptionEngine.pack_lwe on device tensors (or host arrays) -> numpy."""
    pk = fg.PackKey(D(key) if device else key, bl, lv, lwe_a.shape[-1])
    out = None
    if prev is not None:
        out = D(prev) if device else prev.copy()
    w = (D(lwe_a), D(lwe_b)) if device else (lwe_a, lwe_b)
    got = eng.pack_lwe(w[0], w[1], slots, pk, out=out, accumulate=prev is not None)
    assert tuple(got.shape) == (lwe_a.shape[0], 2, eng.ring.degree)
    return H(got) if device else got


WORD_SHAPES = [(4, 97, 2, 4, 3), (256, 7681, 4, 4, 8), (1024, P62, 16, 4, 12), (1024, P27, 33, 2, 5)]


@pytest.mark.parametrize("n,q,bl,lv,in_dim", WORD_SHAPES)
def test_pack_words(fg, n, q, bl, lv, in_dim):
    """Formula and chain, batches 1 / 3 / 17 (a partial tile), slots with 0, n - 1
    and a repeat, accumulate, both modes.  (1024, P27, 33, 2, 5) takes the
    per-term kernel (base_log > 32)."""
    rings = {m: fg.PolynomialRing(n, q, mode=m) for m in ("compat", "negacyclic")}
    engines = {m: fg.EncryptionEngine(r) for m, r in rings.items()}
    be = fg.BootstrapEngine(rings["compat"], 4, 1, 1)
    slots = [0, n - 1, n // 2, n // 2, 1]
    for batch in (1, 3, 17):
        key, lwe_a, lwe_b, prev = inputs([n, batch], n, q, in_dim, lv, batch, len(slots))
        want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots)
        want_acc = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
        assert (want < np.uint64(q)).all() and (want_acc < np.uint64(q)).all()
        if n <= 4:  # word by word in Python integers
            for c in range(batch):
                assert R.pack_formula_int(q, n, bl, lv, key, lwe_a[c], lwe_b[c], slots, prev[c]) == want_acc[c].tolist()
        assert (chain(fg, rings["compat"], be, q, n, bl, lv, key, lwe_a, lwe_b, slots) == want).all(), (n, q, batch, "chain")
        if batch == 3:
            assert (chain(fg, rings["compat"], be, q, n, bl, lv, key, lwe_a, lwe_b, slots, prev) == want_acc).all()
        for mode, eng in engines.items():
            assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots) == want).all(), (n, q, batch, mode)
            assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev) == want_acc).all(), (n, q, batch, mode, "acc")
        for single in ([0], [n - 1]):
            got = pack(fg, engines["negacyclic"], bl, lv, key, lwe_a[:, :1], lwe_b[:, :1], single)
            assert (got == R.pack_formula(q, n, bl, lv, key, lwe_a[:, :1], lwe_b[:, :1], single)).all(), (n, q, batch, single)


def test_pack_words_many_slots_and_tiles(fg):
    """More slots than the inline table holds (32), in more than one slot group,
    over two workgroup tiles (batch 17 of 16 per tile)."""
    n, q, bl, lv, in_dim, batch = 256, 7681, 4, 4, 8, 17
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng, be = fg.EncryptionEngine(r), fg.BootstrapEngine(r, 4, 1, 1)
    rng = np.random.default_rng(40)
    slots = [0, n - 1, 7, 7] + [int(v) for v in rng.integers(0, n, size=37)]
    assert len(slots) > 32
    key, lwe_a, lwe_b, prev = inputs(40, n, q, in_dim, lv, batch, len(slots))
    want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
    assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev) == want).all()
    assert (chain(fg, r, be, q, n, bl, lv, key, lwe_a, lwe_b, slots, prev) == want).all()


@pytest.mark.parametrize("n,q", [(512, Q63), (1024, QG)])
def test_pack_words_wide_moduli(fg, n, q):
    """q >= 2^63: the formula only (key switch's running update wraps there)."""
    bl, lv, in_dim = 16, 4, 6
    slots = [0, n - 1, n // 2, n // 2, 1]
    for mode in ("compat", "negacyclic"):
        eng = fg.EncryptionEngine(fg.PolynomialRing(n, q, mode=mode))
        for batch in (1, 5):
            key, lwe_a, lwe_b, prev = inputs([n, batch, 63], n, q, in_dim, lv, batch, len(slots))
            want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots)
            assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots) == want).all(), (n, q, batch, mode)
            want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
            assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev) == want).all(), (n, q, batch, mode, "acc")


@pytest.mark.parametrize("n,q,bl,lv", [(16384, P62, 16, 4), (32768, P27, 9, 3)])
def test_pack_words_large_degrees(fg, n, q, bl, lv):
    in_dim, batch, slots = 4, 2, [0, n - 1, n // 2]
    r = fg.PolynomialRing(n, q)
    eng, be = fg.EncryptionEngine(r), fg.BootstrapEngine(r, 4, 1, 1)
    key, lwe_a, lwe_b, prev = inputs(n, n, q, in_dim, lv, batch, len(slots))
    want = chain(fg, r, be, q, n, bl, lv, key, lwe_a, lwe_b, slots)
    assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots) == want).all()
    want = chain(fg, r, be, q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
    assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev) == want).all()


def test_pack_host_device_and_multi_device(fg):
    n, q, bl, lv, in_dim, batch = 1024, P62, 16, 4, 12, 17
    slots = [0, n - 1, n // 2, n // 2] + list(range(3, 36))  # beyond the inline table
    key, lwe_a, lwe_b, prev = inputs(77, n, q, in_dim, lv, batch, len(slots))
    want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots)
    want_acc = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
    for devices in (None, [0, 0]):
        r = fg.PolynomialRing(n, q, devices=devices) if devices else fg.PolynomialRing(n, q)
        eng = fg.EncryptionEngine(r)
        for device in (False, True):  # a device tensor on a multi-device context runs where it lives
            assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, device=device) == want).all(), (devices, device)
            assert (pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev, device=device) == want_acc).all(), (devices, device)


def test_pack_argument_errors(fg):
    n, q, bl, lv, in_dim, batch = 256, 7681, 4, 4, 8, 3
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r)
    key, lwe_a, lwe_b, prev = inputs(9, n, q, in_dim, lv, batch, 2)
    dk, da, db, do = D(key), D(lwe_a), D(lwe_b), D(prev)
    pk = fg.PackKey(dk, bl, lv, in_dim)
    with pytest.raises(fg.FHEError, match="slot index out of range") as e:
        eng.pack_lwe(da, db, [0, n], pk)
    assert e.value.code == -9
    with pytest.raises(fg.FHEError, match="LWE masks must be"):
        eng.pack_lwe(da, db, [0], pk)
    # the library's own checks, on device pointers
    slots = (C.c_uint32 * 2)(0, 1)

    def call(key_p, a_p, b_p, out_p):
        rc = fg.lib().fhe_lwe_pack_batch(r._h, bl, lv, in_dim, key_p, a_p, b_p, slots, 2, 0, out_p, batch, fg.FHE_DEVICE)
        assert rc == -9, rc
        return fg.lib().fhe_last_error().decode()

    assert "overlap" in call(dk.data_ptr(), da.data_ptr(), db.data_ptr(), dk.data_ptr() + 8 * n)
    assert "overlap" in call(dk.data_ptr(), da.data_ptr(), db.data_ptr(), da.data_ptr())
    assert "overlap" in call(dk.data_ptr(), do.data_ptr() + 8 * (batch * 2 * n - 1), db.data_ptr(), do.data_ptr())
    assert "overlap" in call(dk.data_ptr(), da.data_ptr(), do.data_ptr() + 8, do.data_ptr())
    assert (H(dk) == key).all() and (H(do) == prev).all()  # nothing ran


@pytest.mark.parametrize("n,q,bl,lv", [(256, P27, 7, 4), (1024, P62, 16, 4)])
def test_pack_key_equals_the_chain(fg, n, q, bl, lv):
    lwe_sk = np.array([-1, 0, 1, -3, 2], dtype=np.int64)  # negative, zero and beyond ternary
    dim, rows, seed, stream = len(lwe_sk), len(lwe_sk) * lv, 2026, 11
    for mode in ("compat", "negacyclic"):
        r = fg.PolynomialRing(n, q, mode=mode)
        kg = fg.KeyGenerator(r, seed=seed)
        sk = kg.secret_key(3)
        for std in (0.0, 2.0):
            pk = kg.pack_key(sk, lwe_sk, bl, lv, stream, std_dev=std)
            assert (pk.base_log, pk.level, pk.lwe_dim) == (bl, lv, dim) and pk.key.shape == (rows, 2, n)
            c1 = fg.sample(r, fg.SAMPLE_UNIFORM, seed, stream, rows * n).reshape(rows, n)
            err = fg.sample(r, fg.SAMPLE_GAUSSIAN, seed, stream + 1, rows * n, std if std else 3.2).reshape(rows, n)
            c0 = r.add(r.multiply(c1, np.ascontiguousarray(np.broadcast_to(sk, (rows, n)))), err)
            for e in range(rows):
                c0[e, 0] = (int(c0[e, 0]) + R.pack_gadget(q, int(lwe_sk[e // lv]), e % lv, bl, lv)) % q
            assert (pk.key[:, 1] == c1).all(), (mode, std)
            assert (pk.key[:, 0] == c0).all(), (mode, std)
            assert err.any() and (pk.key < np.uint64(q)).all()
        # one seed, one key -- on the device too
        again = kg.pack_key(D(sk), D(lwe_sk), bl, lv, stream, std_dev=2.0)
        assert (H(again.key) == pk.key).all()
        assert (kg.pack_key(sk, lwe_sk, bl, lv, stream + 2).key != pk.key).any()


def lwe_encrypt(rng, q, delta, lwe_sk, msgs):
    """msgs [batch, S] -> (a [batch, S, dim], b [batch, S]), errors in [-2, 2]."""
    dim = len(lwe_sk)
    a = rng.integers(0, q, size=msgs.shape + (dim,), dtype=np.uint64)
    e = rng.integers(-2, 3, size=msgs.shape)
    ip = (a.astype(object) * lwe_sk.astype(object)).sum(axis=-1)
    b = (ip + delta * msgs.astype(object) + e.astype(object)) % q
    return a, b.astype(np.uint64)


@pytest.mark.parametrize("mode,slots", [("negacyclic", [3, 250, 17, 128, 0, 255, 64, 99]), ("compat", [0])])
def test_packed_messages_decrypt(fg, mode, slots):
    n, q, t, bl, lv, dim, batch = 256, P27, 16, 7, 4, 16, 3
    assert bl * lv >= (q - 1).bit_length()
    r = fg.PolynomialRing(n, q, mode=mode)
    eng = fg.EncryptionEngine(r, t)
    kg = fg.KeyGenerator(r, seed=20261021)
    sk = kg.secret_key(1)
    rng = np.random.default_rng(5)
    lwe_sk = rng.integers(-1, 2, size=dim).astype(np.int64)
    pk = kg.pack_key(sk, lwe_sk, bl, lv, 7, std_dev=3.2)
    msgs = rng.integers(0, t, size=(batch, len(slots)))
    a, b = lwe_encrypt(rng, q, eng.delta, lwe_sk, msgs)
    ct = eng.pack_lwe(a, b, slots, pk)
    res = eng.decrypt(ct, fg.SecretKey(r, sk))
    want = np.zeros((batch, n), dtype=np.uint64)
    want[:, slots] = msgs
    assert (res.values == want).all()
    print("max_noise", res.max_noise.tolist(), "delta / 4", eng.delta // 4)
    assert (res.max_noise.astype(object) < eng.delta // 4).all() and res.max_noise.all()


def test_comparison_bits_are_tallied_and_opened_by_trustees(fg):
    """greater_equal under all-zero bootstrap keys (as test_truth_tables_under_zero_keys),
    packed, summed over the ballots and opened with 3 of 5 key shares: the number
    of passing ballots per slot."""
    n, q, t = 1024, P27, 16
    bl, lv, ks_bl, ks_lv, dim = 4, 3, 4, 3, 4
    r = fg.PolynomialRing(n, q, mode="negacyclic")
    eng = fg.EncryptionEngine(r, t)
    bsk_ntt = np.zeros((dim, 2 * lv, 2, n), np.uint64)
    ksk_a, ksk_b = np.zeros((n * ks_lv, dim), np.uint64), np.zeros(n * ks_lv, np.uint64)
    cmp_ = fg.Comparisons(r, t, D(bsk_ntt), D(ksk_a), D(ksk_b), bl, lv, ks_bl, ks_lv)
    delta, half_t = q // t, t // 2
    rng = np.random.default_rng(12)
    ballots, slots = 11, [0, 3, n - 1]
    va = rng.integers(0, half_t, size=(ballots, len(slots)))
    vb = rng.integers(0, half_t, size=(ballots, len(slots)))

    def encrypt(vals):
        ct = rng.integers(0, q, size=(ballots, 2, n), dtype=np.uint64)
        ct[:, 0] = 0
        ct[:, 0, slots] = (vals * delta % q).astype(np.uint64)
        return D(ct)

    bits = cmp_.greater_equal(encrypt(va), encrypt(vb), slots)
    kg = fg.KeyGenerator(r, seed=99)
    tk = kg.threshold_keys(3, 5, 20)
    # the LWE key behind all-zero bootstrap keys is the zero key
    pk = kg.pack_key(tk.secret_key.poly, np.zeros(dim, np.int64), 7, 4, 30)
    packed = fg.Comparisons.pack(bits, slots, fg.PackKey(D(pk.key), pk.base_log, pk.level, pk.lwe_dim), eng)
    assert tuple(packed.shape) == (ballots, 2, n)
    tally = H(r.sum_batch(packed, grouped=False))
    shares = tk.shares[1:4]
    partials = eng.partial_decrypt(tally, shares)
    res = eng.combine_partial_decryptions(tally, partials, [s.share_id for s in shares])
    want = np.zeros(n, dtype=np.uint64)
    want[slots] = (va >= vb).sum(axis=0)
    assert want.max() < t
    assert (res.values == want).all()
    assert (eng.decrypt(tally, tk.secret_key).values == want).all()


def test_js_engine():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "pack_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 passed" in r.stdout
