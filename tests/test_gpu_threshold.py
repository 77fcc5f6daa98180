"""GPU parity of threshold decryption (csrc/threshold.hip; fhe_shamir_shares_batch,
fhe_key_share_prepare, fhe_partial_decrypt_batch, fhe_combine_partials_batch):
Shamir shares, batched partial decryptions and their combination, bit for bit.

Expected values in compat mode come from the CPU oracle and Python integers:
  shares    sum_k ((coeffs[k] mod q) (i^k mod q) mod q) mod q
  partials  oracle.NTT(n, q).polymul(c1 % q, share % q)
  phase     oracle.poly_mul_scalar / poly_add per partial, poly_sub from c0
  decode    oracle.NTT.decrypt(t, zeros, [phase, zeros]) (a zero key returns
            the given phase with its decode and noise)
and in every mode the results are compared with the device chain of the entry
points that existed before (multiply, multiply_scalar, add, subtract, decrypt).

Run on an MI355X with ``pytest -m gpu``.
"""
import itertools
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
# the minimum degree, several polynomials per workgroup, 32- and 64-bit lanes,
# each stash policy (registers: n < 32; LDS: e.g. 1024 and 16384 at 32 bits;
# the last share's output row: 16384 at 64 bits)
FUSED = [(4, 97), (16, 97), (256, 7681), (1024, P27), (1024, P62), (4096, P27), (16384, P27), (16384, P62)]
COMPOSED = [(1024, QG), (32768, P27)]   # wide modulus, two-pass degree


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


def raw(seed, q, shape):
    """Full-range u64 words with 0, q - 1, q, 2^64 - 1 planted at both ends."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    edge = np.array([0, q - 1, q, M64], dtype=np.uint64)
    flat = a.reshape(-1)
    flat[:4] = edge
    flat[-4:] = edge[::-1]
    return a


def lam_ref(q, ids, used):
    """lagrange_coefficient (key_manager.cpp:548-582) in Python integers."""
    out = []
    for i in ids[:used]:
        num = den = 1
        for j in ids:
            if j != i:
                num = num * j % q
                d = j - i
                den = den * ((q - (-d) % q) if d < 0 else d % q) % q
        out.append(num * oracle.mod_inverse(den, q) % q)
    return out


def oracle_phase(q, ct, partials, lams):
    """[b, n]: c0 - sum_i partials[i] lam_i with the oracle's polynomial ops."""
    qq = np.uint64(q)
    b, n = ct.shape[0], ct.shape[-1]
    acc = np.zeros(b * n, dtype=np.uint64)
    for p, lam in zip(partials, lams):
        term = oracle.poly_mul_scalar(q, np.ascontiguousarray((p % qq).reshape(-1)), int(lam) % q)
        acc = oracle.poly_add(q, acc, term)
    c0 = np.ascontiguousarray((ct[:, 0, :] % qq).reshape(-1))
    return oracle.poly_sub(q, c0, acc).reshape(b, n)


def oracle_decode(n, q, t, phase):
    """decode + noise of a phase: the oracle's decrypt with a zero key."""
    o = oracle.NTT(n, q)
    zero = np.zeros(n, dtype=np.uint64)
    vals = np.empty_like(phase)
    mx = np.empty(phase.shape[0], dtype=np.uint64)
    for i in range(phase.shape[0]):
        v, ph, m = o.decrypt(t, zero, np.stack([phase[i], zero]))
        assert (ph == phase[i]).all()
        vals[i], mx[i] = v, m
    return vals, mx


# ---------------------------------------------------------------- 1. Shamir shares
@pytest.mark.parametrize("n,q", FUSED + COMPOSED)
def test_shamir_shares_equal_the_formula(fg, n, q):
    r = fg.PolynomialRing(n, q)
    for k, (threshold, total) in enumerate([(1, 1), (2, 3), (5, 7)]):
        coeffs = raw(n + k, q, (threshold, n))
        got = H(fg.shamir_shares(r, D(coeffs), total))
        assert got.shape == (total, n)
        c = coeffs.astype(object) % q
        for i in range(1, total + 1):
            want = sum(c[j] * pow(i, j, q) % q for j in range(threshold)) % q
            assert (got[i - 1].astype(object) == want).all(), (threshold, total, i)
        host = fg.shamir_shares(r, coeffs, total)
        assert isinstance(host, np.ndarray) and (host == got).all()


# ---------------------------------------------------------------- 2. partial decryption
def check_partial(fg, n, q, mode="compat", oracle_too=True):
    r = fg.PolynomialRing(n, q, mode=mode)
    eng = fg.EncryptionEngine(r)
    o = oracle.NTT(n, q) if oracle_too else None
    qq = np.uint64(q)
    for k, (b, ns) in enumerate([(3, 1), (5, 3), (3, 3), (5, 1)]):
        ct = raw(n * 3 + k, q, (b, 2, n))
        sh = raw(n * 5 + k, q, (ns, n))
        shares = [fg.KeyShare(r, i + 1, D(sh[i])) for i in range(ns)]
        dct = D(ct)
        got = H(eng.partial_decrypt(dct, shares))
        assert got.shape == (ns, b, n)
        c1 = np.ascontiguousarray(ct[:, 1, :])
        for s in range(ns):
            tiled = np.ascontiguousarray(np.broadcast_to(sh[s], (b, n)))
            assert (got[s] == H(r.multiply(D(c1), D(tiled)))).all(), (b, ns, s)
            if oracle_too:
                assert (got[s] == o.polymul(c1 % qq, tiled % qq)).all(), (b, ns, s)
        # a single KeyShare: [batch, n]
        one = H(eng.partial_decrypt(dct, shares[0]))
        assert one.shape == (b, n) and (one == got[0]).all()
        # c0 is never read
        ct2 = ct.copy()
        ct2[:, 0, :] = raw(n * 7 + k, q, (b, n))
        assert (H(eng.partial_decrypt(D(ct2), shares)) == got).all()


@pytest.mark.parametrize("n,q", FUSED)
def test_partial_decrypt_vs_oracle_and_chain(fg, n, q):
    check_partial(fg, n, q)


@pytest.mark.parametrize("n,q", COMPOSED)
def test_partial_decrypt_composed_paths(fg, n, q):
    check_partial(fg, n, q)


def test_partial_decrypt_negacyclic_matches_chain(fg):
    check_partial(fg, 4096, P27, mode="negacyclic", oracle_too=False)


# ---------------------------------------------------------------- 3. combination
def check_combine(fg, n, q, mode="compat"):
    import torch

    r = fg.PolynomialRing(n, q, mode=mode)
    zero_key = fg.SecretKey(r, D(np.zeros(n, dtype=np.uint64)))
    L = fg.lib()
    b = 3
    for k, (count, t) in enumerate(itertools.product((1, 2, 5), (0, 16, 1 << 40))):
        eng = fg.EncryptionEngine(r, t)
        ct = raw(n * 11 + k, q, (b, 2, n))
        par = raw(n * 13 + k, q, (count, b, n))
        lams = [int(x) for x in raw(n * 17 + k, q, (12,))[2:2 + count]]   # q, 2^64 - 1, then random words
        dct, dpar = D(ct), D(par)
        res = eng.combine_partials(dct, dpar, lams, with_phase=True)
        phase, vals, mx = H(res.phase), H(res.values), res.max_noise
        want = oracle_phase(q, ct, par, lams)
        assert (phase == want).all(), (count, t)
        wv, wm = oracle_decode(n, q, t, want)
        assert (vals == wv).all(), (count, t)
        assert (mx == wm).all(), (count, t, mx, wm)
        # the device chain of the older entry points
        acc = None
        for i in range(count):
            term = r.multiply_scalar(dpar[i], lams[i])
            acc = term if acc is None else r.add(acc, term)
        chain = H(r.subtract(dct[:, 0, :].contiguous(), acc))
        assert (phase == chain).all(), (count, t)
        as_ct = np.stack([chain, np.zeros_like(chain)], axis=1)
        dec = eng.decrypt(D(as_ct), zero_key)
        assert (vals == H(dec.values)).all() and (mx == dec.max_noise).all(), (count, t)
        # each output alone
        lam_arr = (fg.C.c_uint64 * count)(*lams)
        for which in range(3):
            outs = [torch.zeros((b, n), dtype=torch.int64, device="cuda:0"),
                    torch.zeros((b, n), dtype=torch.int64, device="cuda:0"),
                    torch.zeros((b,), dtype=torch.int64, device="cuda:0")]
            ptrs = [o.data_ptr() if i == which else None for i, o in enumerate(outs)]
            rc = L.fhe_combine_partials_batch(r._h, t, dct.data_ptr(), dpar.data_ptr(), lam_arr, count, ptrs[0], ptrs[1],
                                              ptrs[2], b, fg.FHE_DEVICE)
            assert rc == 0, L.fhe_last_error()
            assert (H(outs[which]) == (vals, phase, mx)[which]).all(), (count, t, which)
            assert not any(H(o).any() for i, o in enumerate(outs) if i != which)
        # c1 is never read
        ct2 = ct.copy()
        ct2[:, 1, :] = raw(n * 19 + k, q, (b, n))
        res2 = eng.combine_partials(D(ct2), dpar, lams, with_phase=True)
        assert (H(res2.phase) == phase).all() and (H(res2.values) == vals).all() and (res2.max_noise == mx).all()


@pytest.mark.parametrize("n,q", FUSED + COMPOSED)
def test_combine_vs_oracle_and_chain(fg, n, q):
    check_combine(fg, n, q)


@pytest.mark.parametrize("count", [16, 17, 70])
def test_combine_many_partials(fg, count):
    """Up to 16 lambdas travel as kernel arguments, more in a device table
    written 64 entries per launch: both sides of each boundary."""
    n, q, b, t = 256, 7681, 3, 16
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r, t)
    ct = raw(count, q, (b, 2, n))
    par = raw(count + 1, q, (count, b, n))
    lams = [int(x) for x in raw(count + 2, q, (count,))]
    res = eng.combine_partials(D(ct), D(par), lams, with_phase=True)
    want = oracle_phase(q, ct, par, lams)
    assert (H(res.phase) == want).all()
    wv, wm = oracle_decode(n, q, t, want)
    assert (H(res.values) == wv).all() and (res.max_noise == wm).all()
    host = eng.combine_partials(ct, par, lams, with_phase=True)
    assert (host.phase == want).all() and (host.values == wv).all() and (host.max_noise == wm).all()


# ---------------------------------------------------------------- 4. end to end
# Noise of the encryptions.  In negacyclic mode the ring product is the
# multiplication of Z_q[X]/(X^n + 1) and sigma = 3.2 is the reference's default.
# The compat product is the reference transform pair's: commutative, associative
# and bilinear, so combine == decrypt holds word for word at any noise, but it
# is not that convolution and the noise terms e u, e2 s do not stay small --
# the CPU oracle itself recovers about 5 % of the slots at sigma = 3.2 (n = 1024,
# q = 132120577, t = 16: max_noise 4127087 of a budget 4128768).  There the
# slots are checked on noiseless encryptions (sigma = 3.2e-11 rounds every error
# coefficient to 0, as in tests/test_gpu_dot.py), where phase = encode(m)
# follows from associativity alone; the noisy ones are still compared with
# decrypt, without the slot check.
@pytest.mark.parametrize("n,q,mode,sigmas", [(1024, P27, "compat", (3.2e-11, 3.2)), (4096, P62, "compat", (3.2e-11, 3.2)),
                                             (1024, P27, "negacyclic", (3.2,))])
def test_threshold_decryption_end_to_end(fg, n, q, mode, sigmas):
    t = 16
    r = fg.PolynomialRing(n, q, mode=mode)
    eng = fg.EncryptionEngine(r, t)
    for sigma in sigmas:
        slots_hold = mode == "negacyclic" or sigma < 1e-6
        kg = fg.KeyGenerator(r, seed=20261020, noise_std=sigma)
        tk = kg.threshold_keys(3, 5, stream=100, device_out=True)
        assert (tk.threshold, tk.total_shares, len(tk.shares)) == (3, 5, 5)
        assert [s.share_id for s in tk.shares] == [1, 2, 3, 4, 5]
        # the key material is the documented one: master from `stream`, coefficient j from stream + j
        master = H(tk.secret_key.poly)
        assert (master == fg.sample(r, fg.SAMPLE_TERNARY, kg.seed, 100, n)).all()
        coeffs = np.stack([master] + [fg.sample(r, fg.SAMPLE_UNIFORM, kg.seed, 100 + j, n) for j in (1, 2)])
        c = coeffs.astype(object)
        for s in tk.shares:
            want = sum(c[j] * pow(s.share_id, j, q) % q for j in range(3)) % q
            assert (H(s.poly).astype(object) == want).all(), s.share_id
        pk = fg.PublicKey(r, kg.public_key(tk.secret_key.poly, stream=200))
        slots = np.random.default_rng(n).integers(0, t, size=(4, n), dtype=np.uint64)
        ct = eng.encrypt_sampled(D(slots), pk, kg.seed, stream=300, noise_std=sigma)
        ref = eng.decrypt(ct, tk.secret_key, with_phase=True)
        if slots_hold:
            assert (H(ref.values) == slots).all() and ref.success.all()
        # exact: the ring product is bilinear over Z_q and the lambdas interpolate the shares at 0
        for subset in ((0, 2, 4), (3, 1, 2)):
            shares = [tk.shares[i] for i in subset]
            partials = eng.partial_decrypt(ct, shares)
            res = eng.combine_partial_decryptions(ct, partials, [s.share_id for s in shares], with_phase=True)
            assert (H(res.phase) == H(ref.phase)).all(), (sigma, subset)
            assert (H(res.values) == H(ref.values)).all(), (sigma, subset)
            assert (res.max_noise == ref.max_noise).all(), (sigma, subset)
            if slots_hold:
                assert (H(res.values) == slots).all() and res.success.all(), (sigma, subset)
            # a list of per-trustee blocks is accepted as well
            res_l = eng.combine_partial_decryptions(ct, [partials[i] for i in range(3)], [s.share_id for s in shares])
            assert (H(res_l.values) == H(ref.values)).all() and (res_l.max_noise == ref.max_noise).all()
        # four partials, threshold 3: the reference rule (lambdas over four ids, the first three summed)
        shares = [tk.shares[i] for i in (4, 0, 3, 1)]
        ids = [s.share_id for s in shares]
        partials = eng.partial_decrypt(ct, shares)
        res = eng.combine_partial_decryptions(ct, partials, ids, threshold=3, with_phase=True)
        want = oracle_phase(q, H(ct), H(partials)[:3], lam_ref(q, ids, 3))
        assert (H(res.phase) == want).all()
        wv, wm = oracle_decode(n, q, t, want)
        assert (H(res.values) == wv).all() and (res.max_noise == wm).all()


# ---------------------------------------------------------------- 5. residence
def test_host_arrays_and_multi_device(fg):
    n, q, b, t = 1024, P27, 5, 16
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r, t)
    mr = fg.PolynomialRing(n, q, devices=[0, 0])
    multi = fg.EncryptionEngine(mr, t)
    ct = raw(1, q, (b, 2, n))
    sh = raw(2, q, (3, n))
    lams = [int(x) for x in raw(3, q, (6,))[1:4]]   # q - 1, q, 2^64 - 1
    dev_p = H(eng.partial_decrypt(D(ct), [fg.KeyShare(r, i + 1, D(sh[i])) for i in range(3)]))
    host_p = eng.partial_decrypt(ct, [fg.KeyShare(r, i + 1, sh[i]) for i in range(3)])
    assert isinstance(host_p, np.ndarray) and (host_p == dev_p).all()
    mshares = [fg.KeyShare(mr, i + 1, sh[i]) for i in range(3)]
    # FHE_HOST on two sub-contexts: the batch is split 3 + 2, every share's block with it
    assert (multi.partial_decrypt(ct, mshares) == dev_p).all()
    assert (H(multi.partial_decrypt(D(ct), mshares)) == dev_p).all()
    dev_c = eng.combine_partials(D(ct), D(dev_p), lams, with_phase=True)
    for e, c, p in ((eng, ct, dev_p), (multi, ct, dev_p), (multi, D(ct), D(dev_p))):
        res = e.combine_partials(c, p, lams, with_phase=True)
        get = H if not isinstance(res.values, np.ndarray) else (lambda x: x)
        assert (get(res.values) == H(dev_c.values)).all()
        assert (get(res.phase) == H(dev_c.phase)).all()
        assert (res.max_noise == dev_c.max_noise).all()
    # host shares with device ciphertexts: the prepared form follows the ciphertexts
    assert (H(eng.partial_decrypt(D(ct), [fg.KeyShare(r, 1, sh[0])])) == dev_p[:1]).all()


# ---------------------------------------------------------------- 6. errors
def test_errors(fg):
    n, q, b = 256, 7681, 3
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r)
    kg = fg.KeyGenerator(r, seed=5)
    for threshold, total in ((0, 3), (4, 3)):
        with pytest.raises(fg.FHEError, match="Invalid threshold parameters"):
            kg.threshold_keys(threshold, total, stream=0)
    with pytest.raises(fg.FHEError, match="Invalid threshold parameters"):
        fg.shamir_shares(r, D(raw(1, q, (4, n))), 3)
    ct = D(raw(2, q, (b, 2, n)))
    shares = [fg.KeyShare(r, i + 1, D(raw(3 + i, q, (n,)))) for i in range(3)]
    with pytest.raises(fg.FHEError, match="at least one key share"):
        eng.partial_decrypt(ct, [])
    partials = eng.partial_decrypt(ct, shares)
    good = H(eng.combine_partial_decryptions(ct, partials, [1, 2, 3]).values)
    with pytest.raises(fg.FHEError, match="Not enough partial decryptions"):
        eng.combine_partial_decryptions(ct, partials[:2], [1, 2], threshold=3)
    with pytest.raises(fg.FHEError, match="Not enough partial decryptions"):
        eng.combine_partial_decryptions(ct, [], [])
    with pytest.raises(fg.FHEError, match="distinct and non-zero"):
        eng.combine_partial_decryptions(ct, partials, [1, 2, 1])
    with pytest.raises(fg.FHEError, match="distinct and non-zero"):
        eng.combine_partial_decryptions(ct, partials, [0, 1, 2])
    with pytest.raises(fg.FHEError, match="one share id per partial"):
        eng.combine_partial_decryptions(ct, partials, [1, 2])
    L = fg.lib()
    dev = fg.FHE_DEVICE
    lam = (fg.C.c_uint64 * 3)(1, 2, 3)
    pc, pp = ct.data_ptr(), partials.data_ptr()
    prep = shares[0].prep.data_ptr()

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return L.fhe_last_error().decode()

    assert err(L.fhe_combine_partials_batch(r._h, 0, pc, pp, lam, 0, pp, None, None, b, dev)) == "Not enough partial decryptions"
    assert "at least one of" in err(L.fhe_combine_partials_batch(r._h, 0, pc, pp, lam, 3, None, None, None, b, dev))
    assert "overlap" in err(L.fhe_combine_partials_batch(r._h, 0, pc, pp, lam, 3, pc, None, None, b, dev))
    assert "overlap" in err(L.fhe_combine_partials_batch(r._h, 0, pc, pp, lam, 3, None, pp + 8 * n, None, b, dev))
    assert "at least one key share" in err(L.fhe_partial_decrypt_batch(r._h, prep, 0, pc, pp, b, dev))
    assert "at least one ciphertext" in err(L.fhe_partial_decrypt_batch(r._h, prep, 1, pc, pp, 0, dev))
    assert "overlap" in err(L.fhe_partial_decrypt_batch(r._h, prep, 1, pc, pc + 8 * n, b, dev))
    err(L.fhe_partial_decrypt_batch(r._h, prep, 1, pc, pp, b, 7))
    # the failed calls enqueued nothing: a good call still works
    assert (H(eng.combine_partial_decryptions(ct, eng.partial_decrypt(ct, shares), [1, 2, 3]).values) == good).all()


# ---------------------------------------------------------------- 7. the JS engine
def test_threshold_js_engine(fg):
    """partialDecryptBatch / combinePartialDecryptionsBatch and the three
    single-ciphertext methods of the JS engine over the addon's
    shamirSharesAsync / prepareKeySharesAsync / partialDecryptPreparedAsync /
    combinePartialsAsync (tests/js/threshold_test.js)."""
    node = shutil.which("node")
    addon = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "fhe_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node / N-API addon not available")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "threshold_test.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "5 passed" in r.stdout, r.stdout
