"""GPU parity of ciphertext squaring and the squared difference
(csrc/ct_square.hip, elementwise.hip k_square_ntt; fhe_ct_square_batch /
fhe_ct_square_relin_batch): out = square(ct - ref).

Expected value in compat mode: oracle.NTT(n, q).ct_multiply(d, d, is_ntt) with
d = oracle.poly_sub(q, ct % q, ref % q) (or ct % q without a ref).  In every
case, and as the only check in negacyclic mode (the oracle is compat), the
result is also compared bit for bit with the device chain of the entry points
that existed before: eng.multiply(eng.subtract(ct, ref), the same).

Run on an MI355X with ``pytest -m gpu``.
"""
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
REFS = ("none", "shared", "each")


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


def inputs(seed, q, b, n, mode):
    """ct [b, 2, n] and ref (None, [2, n] or [b, 2, n]) of full-range random
    u64 words.  0, q - 1, q, 2^64 - 1 are planted in the first and the last
    ciphertext of both; ciphertext 0 equals its ref (an all-zero difference);
    with more than two ciphertexts every word of ciphertext 1 is below its
    ref's modulo q (the subtraction wraps), or equal to it where that residue
    is zero."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    ct = rng.integers(0, 1 << 64, size=(b, 2, n), dtype=np.uint64)
    ct[0, 0, :4] = edge
    ct[-1, -1, -4:] = edge[::-1]
    if mode == "none":
        return ct, None
    ref = rng.integers(0, 1 << 64, size=(b, 2, n), dtype=np.uint64)
    ref[0, 0, -4:] = edge
    ref[0, -1, :4] = edge[::-1]
    ref[-1, -1, -4:] = edge
    ref[-1, 0, :4] = edge[::-1]
    if mode == "shared":
        ref = ref[0].copy()
    against = ref if mode == "shared" else ref[1]
    ct[0] = ref if mode == "shared" else ref[0]
    if b > 2:  # with two ciphertexts, 1 is the last one and keeps its planted words
        # below the ref's residue; where that is zero (a shared ref's planted 0 and q) equal to it
        r = against % np.uint64(q)
        below = rng.integers(0, 1 << 64, size=(2, n), dtype=np.uint64) % np.where(r == 0, np.uint64(1), r)
        ct[1] = np.where(r == 0, against, below)
    return ct, ref


def expected(t, q, ct, ref, is_ntt):
    """The oracle's multiply(d, d) per ciphertext, d = poly_sub(ct % q, ref % q)."""
    qq = np.uint64(q)
    out = np.empty((ct.shape[0], 3, ct.shape[-1]), dtype=np.uint64)
    for i in range(ct.shape[0]):
        d = np.ascontiguousarray(ct[i] % qq)
        if ref is not None:
            ri = ref if ref.ndim == 2 else ref[i]
            d = oracle.poly_sub(q, d.ravel(), np.ascontiguousarray(ri % qq).ravel()).reshape(d.shape)
        out[i] = t.ct_multiply(d, d, is_ntt)
    return out


def chain(eng, dct, dref, is_ntt):
    """The pre-existing entry points: subtract, then multiply(d, d)."""
    d = dct
    if dref is not None:
        d = eng.subtract(dct, dref if dref.dim() == dct.dim() else dref.unsqueeze(0).expand(dct.shape).contiguous())
    return H(eng.multiply(d, d, is_ntt=is_ntt))


def check_shape(fg, n, q, b, mode="compat", oracle_too=True):
    r = fg.PolynomialRing(n, q, mode=mode)
    eng = fg.EncryptionEngine(r)
    t = oracle.NTT(n, q) if oracle_too else None
    # the last case: canonical words, which take the loader's fast path
    for k, (refmode, canon) in enumerate([(m, False) for m in REFS] + [("each", True)]):
        ct, ref = inputs(n * 7 + k, q, b, n, refmode)
        if canon:
            ct, ref = ct % np.uint64(q), ref % np.uint64(q)
        dct, dref = D(ct), (None if ref is None else D(ref))
        for is_ntt in (False, True):
            if dref is None:
                got = H(eng.square(dct, is_ntt=is_ntt))
            else:
                got = H(eng.squared_difference(dct, dref, is_ntt=is_ntt))
            assert got.shape == (b, 3, n)
            assert (got == chain(eng, dct, dref, is_ntt)).all(), (refmode, is_ntt)
            if oracle_too:
                assert (got == expected(t, q, ct, ref, is_ntt)).all(), (refmode, is_ntt)
            if refmode != "none":
                assert not got[0].any(), "a ciphertext equal to its ref squares to zero"


# test_ct_multiply_vs_oracle's list: every dispatch branch of the fused family
# (several ciphertexts per workgroup up to 2048, 16 or 32 coefficients per
# thread, 32-bit lazy / non-lazy and 64-bit words)
@pytest.mark.parametrize("n,q", [(4, 17), (16, 97), (256, 7681), (1024, P27), (2048, P62), (4096, P27),
                                 (4096, P62), (8192, P27), (8192, P62), (8192, 1073643521),
                                 (8192, 1152921504606584833), (16384, P27), (16384, P62), (16384, 1073643521)])
def test_square_vs_oracle_and_chain(fg, n, q):
    check_shape(fg, n, q, 3 if n >= 8192 else 5)


@pytest.mark.parametrize("n,q", [(32768, P27), (1024, QG)])
def test_square_composed_paths(fg, n, q):
    check_shape(fg, n, q, 2)


def test_square_negacyclic_matches_chain(fg):
    check_shape(fg, 4096, P27, 5, mode="negacyclic", oracle_too=False)


@pytest.mark.parametrize("n,q", [(1024, P27), (16384, P27)])
def test_square_relin_is_composition(fg, n, q):
    bl, lv, b = 4, 7, 3
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r)
    rlk = oracle.splitmix_fill(23, q, lv * 2 * n).reshape(lv, 2, n)
    ek = fg.EvaluationKey(r, D(rlk), bl)
    t = oracle.NTT(n, q)
    for k, refmode in enumerate(REFS):
        ct, ref = inputs(n + 50 + k, q, b, n, refmode)
        dct, dref = D(ct), (None if ref is None else D(ref))
        if dref is None:
            got = H(eng.square_relin(dct, ek))
            want = H(eng.relinearize(eng.square(dct), ek))
        else:
            got = H(eng.compute_anomaly_score(dct, dref, ek))
            want = H(eng.relinearize(eng.squared_difference(dct, dref), ek))
        assert got.shape == (b, 2, n)
        assert (got == want).all(), refmode
        if n == 1024:
            ct3 = expected(t, q, ct, ref, False)
            for i in range(b):
                assert (got[i] == t.relinearize(bl, lv, ct3[i], rlk)).all(), (refmode, i)


def test_host_arrays_multi_device_and_errors(fg):
    import torch

    n, q, b = 1024, P27, 5
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r)
    multi = fg.EncryptionEngine(fg.PolynomialRing(n, q, devices=[0, 0]))
    rlk = oracle.splitmix_fill(29, q, 7 * 2 * n).reshape(7, 2, n)
    for k, refmode in enumerate(REFS):
        ct, ref = inputs(900 + k, q, b, n, refmode)
        dct, dref = D(ct), (None if ref is None else D(ref))
        for is_ntt in (False, True):
            dev = H(eng.squared_difference(dct, dref, is_ntt=is_ntt))
            host = eng.squared_difference(ct, ref, is_ntt=is_ntt)
            assert isinstance(host, np.ndarray) and (host == dev).all(), (refmode, is_ntt)
            # FHE_HOST on two sub-contexts: the batch is split 3 + 2, a per-ciphertext ref with it
            assert (multi.squared_difference(ct, ref, is_ntt=is_ntt) == dev).all(), (refmode, is_ntt)
            assert (H(multi.squared_difference(dct, dref, is_ntt=is_ntt)) == dev).all(), (refmode, is_ntt)
        score = H(eng.compute_anomaly_score(dct, dref, fg.EvaluationKey(r, D(rlk), 4)))
        assert (eng.compute_anomaly_score(ct, ref, fg.EvaluationKey(r, rlk, 4)) == score).all(), refmode
        mr = multi.ring
        assert (multi.compute_anomaly_score(ct, ref, fg.EvaluationKey(mr, rlk, 4)) == score).all(), refmode
    # out = given buffer
    ct, ref = inputs(950, q, b, n, "each")
    out = torch.empty((b, 3, n), dtype=torch.int64, device="cuda:0")
    assert eng.squared_difference(D(ct), D(ref), out=out) is out
    assert (H(out) == H(eng.squared_difference(D(ct), D(ref)))).all()
    # errors
    L = fg.lib()
    dct, dref = D(ct), D(ref)
    pc, pr, po = dct.data_ptr(), dref.data_ptr(), out.data_ptr()
    dev = fg.FHE_DEVICE

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return L.fhe_last_error().decode()

    assert "ref_count must be 0, 1 or the batch size" in err(L.fhe_ct_square_batch(r._h, pc, pr, 2, po, 5, 0, dev))
    assert "ref and ref_count" in err(L.fhe_ct_square_batch(r._h, pc, None, 1, po, 5, 0, dev))
    assert "ref and ref_count" in err(L.fhe_ct_square_batch(r._h, pc, pr, 0, po, 5, 0, dev))
    assert err(L.fhe_ct_square_batch(r._h, None, None, 0, po, 5, 0, dev)) == "null buffer"
    assert err(L.fhe_ct_square_batch(r._h, pc, None, 0, None, 5, 0, dev)) == "null buffer"
    err(L.fhe_ct_square_batch(r._h, pc, None, 0, po, 5, 0, 7))
    # out inside ct, out inside ref (is_ntt too), and inside a shared ref
    assert "overlap" in err(L.fhe_ct_square_batch(r._h, pc, None, 0, pc + 8 * 2 * n, 2, 0, dev))
    assert "overlap" in err(L.fhe_ct_square_batch(r._h, pc, pr, 5, pr + 8 * 4 * n, 5, 1, dev))
    assert "overlap" in err(L.fhe_ct_square_batch(r._h, pc + 8 * 2 * n, pc, 1, pc, 1, 0, dev))
    assert "invalid decomposition" in err(L.fhe_ct_square_relin_batch(r._h, 0, 7, pc, None, 0, pr, po, 5, dev))
    assert err(L.fhe_ct_square_relin_batch(r._h, 4, 7, pc, None, 0, None, po, 5, dev)) == "null buffer"
    assert L.fhe_ct_square_batch(r._h, None, None, 0, None, 0, 0, dev) == 0  # an empty batch is no error
    with pytest.raises(fg.FHEError, match="ciphertext shapes differ"):
        eng.squared_difference(dct, dref[:2])
    # the failed calls enqueued nothing: a good call still works
    assert (H(eng.squared_difference(dct, dref)) == H(out)).all()


def test_square_js_engine(fg):
    """square / squareRelin / computeAnomalyScore of the JS engine over the
    addon's ctSquareAsync / ctSquareRelinPreparedAsync (tests/js/square_test.js)."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "square_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "4 passed" in r.stdout, r.stdout
