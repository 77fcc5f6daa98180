"""LWE-to-RLWE packing (lwe_pack.hip, fhe_lwe_pack_batch) in the corners of its
signed 96-bit sum and at the thresholds where its fast form switches off, word
for word against the header formula restated in tests/pack_ref.py.

PackAcc<true> keeps hi 2^64 + lo in two's complement; value() negates a
negative sum and carries into the high word only when lo is exactly 0.  Random
inputs (test_gpu_pack.py) never produce that, nor the largest magnitude of a
shape, nor a body that wraps the low word.  tests/range_inputs.py plants these
states (pack_planted; test_range_inputs.py proves on the CPU, in Python
integers, that each occurs), here in all three ciphertext tiles (batch 1, 4,
17), with and without accumulation.  FAST ends at q >= 2^63 and at base_log >
32: the primes on either side of 2^63 and the last prime of the word, base_log
1, 31, 32, 33 and 63.  The window test fills every array from the streaming
edge words.

Run on an MI355X with ``pytest -m gpu``."""
import numpy as np
import pytest

import ntt_primes as P
import pack_ref as R
import range_inputs as I

pytestmark = pytest.mark.gpu

SLOTS = I.PACK_SLOTS  # 0, n - 1 and a repeat


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


def pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev=None):
    pk = fg.PackKey(D(key), bl, lv, lwe_a.shape[-1])
    out = None if prev is None else D(prev)
    got = H(eng.pack_lwe(D(lwe_a), D(lwe_b), slots, pk, out=out, accumulate=prev is not None))
    assert got.shape == (lwe_a.shape[0], 2, eng.ring.degree)
    return got


def bad_words(got, want):
    return np.argwhere(got != want)[:4].tolist()


def prev_words(q, batch, n):
    """`out` before an accumulating call: the streaming edge words, cyclically."""
    W = np.array(P.stream_words(q), dtype=np.uint64)
    return np.ascontiguousarray(W[(np.arange(batch * 2 * n) + np.arange(batch * 2 * n) // n) % len(W)].reshape(batch, 2, n))


def check_planted(fg, eng, n, q, bl, lv, in_dim, batches, label):
    for name, (key, lwe_a, lwe_b) in I.pack_planted(n, q, bl, lv, in_dim, SLOTS).items():
        for batch in batches:
            a = np.ascontiguousarray(np.broadcast_to(lwe_a, (batch,) + lwe_a.shape))
            b = np.ascontiguousarray(np.broadcast_to(lwe_b, (batch,) + lwe_b.shape))
            prev = prev_words(q, batch, n)
            want = R.pack_formula(q, n, bl, lv, key, a, b, SLOTS)
            got = pack(fg, eng, bl, lv, key, a, b, SLOTS)
            assert (got == want).all(), (label, name, batch, "plain", bad_words(got, want))
            want_acc = R.pack_formula(q, n, bl, lv, key, a, b, SLOTS, prev)
            got = pack(fg, eng, bl, lv, key, a, b, SLOTS, prev)
            assert (got == want_acc).all(), (label, name, batch, "accumulate", bad_words(got, want_acc))
            if batch == 1:  # word by word in Python integers
                assert R.pack_formula_int(q, n, bl, lv, key, lwe_a, lwe_b, SLOTS, prev[0]) == want_acc[0].tolist(), (label, name)


@pytest.mark.parametrize("name", ["7681", "u64_bottom", "shoup_top"])
def test_pack_accumulator_states(fg, name):
    n, in_dim = I.PACK_N, I.PACK_IN_DIM
    bl, lv = I.PACK_STATES_DECOMP
    q = 7681 if name == "7681" else P.stream_primes(n)[name]
    eng = fg.EncryptionEngine(fg.PolynomialRing(n, q, mode="negacyclic"))
    check_planted(fg, eng, n, q, bl, lv, in_dim, (1, 4, 17), (name, bl, lv))


@pytest.mark.parametrize("mode", ["compat", "negacyclic"])
@pytest.mark.parametrize("name", ["shoup_top", "wmont_bottom", "u64_max"])
def test_pack_fast_threshold(fg, name, mode):
    """base_log 32 is the largest digit the fast form holds in 32 bits, 33 the
    first it must not take; shoup_top is the last fast modulus."""
    n, in_dim = I.PACK_N, I.PACK_IN_DIM
    q = P.stream_primes(n)[name]
    eng = fg.EncryptionEngine(fg.PolynomialRing(n, q, mode=mode))
    for bl, lv in I.PACK_THRESHOLD_DECOMPS:
        assert (lv - 1) * bl < 64
        check_planted(fg, eng, n, q, bl, lv, in_dim, (1, 4), (name, mode, bl, lv))


@pytest.mark.parametrize("name", P.STREAM_NAMES + ("97",))
def test_pack_window_words(fg, name):
    # 97 = 1 mod 32 only: it runs at n = 16, the largest degree it serves
    n = 16 if name == "97" else 64
    in_dim, lv, bl, batch = I.PACK_WINDOW
    slots = I.pack_window_slots(n)
    q = 97 if name == "97" else P.stream_primes(n)[name]
    eng = fg.EncryptionEngine(fg.PolynomialRing(n, q, mode="negacyclic"))
    key, lwe_a, lwe_b, prev = I.pack_window(n, q, in_dim, lv, batch, len(slots))
    want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots)
    got = pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots)
    assert (got == want).all(), (name, "plain", bad_words(got, want))
    want = R.pack_formula(q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
    got = pack(fg, eng, bl, lv, key, lwe_a, lwe_b, slots, prev)
    assert (got == want).all(), (name, "accumulate", bad_words(got, want))
