"""CPU-side contract of threshold decryption: the five C entry points are
declared, exported and bound and check their arguments without a GPU;
fhe_lagrange_coefficients (a host function) equals the reference's formula in
Python integers; the Python methods exist; every k_partial_dec kernel and
k_combine_partials use no scratch and spill no VGPR, in 32- and 64-bit words;
the typed JS surface declares FHEThresholdEngine and the addon, the ring wrapper
and the engine have the methods."""
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import fhe_gpu
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_shamir_shares_batch": 6, "fhe_key_share_prepare": 5, "fhe_partial_decrypt_batch": 7,
                "fhe_lagrange_coefficients": 5, "fhe_combine_partials_batch": 11}
CTX_METHODS = ("shamirShares", "prepareKeyShares", "partialDecryptPrepared", "combinePartials")
P27 = 132120577
P62 = 4611686018326724609
QG = 18446744069414584321


def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fhe_gpu.h")).read()
    lib = fhe_gpu.lib()
    bound = {s[0]: s for s in fhe_gpu.SIGNATURES}
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name
        assert name in bound, name
        assert len(bound[name][2]) == nargs, name
    assert "#define FHE_GPU_ABI_VERSION 1" in hdr


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = C.c_uint64(0)
    p = C.addressof(word)
    lam = (C.c_uint64 * 2)(1, 2)

    def err(rc):
        assert rc == -9, rc  # FHE_ERR_INVALID_ARG
        return lib.fhe_last_error().decode()

    # fhe_shamir_shares_batch: threshold == 0, threshold > total, null buffers
    assert err(lib.fhe_shamir_shares_batch(None, p, 0, 3, p, dev)) == "Invalid threshold parameters"
    assert err(lib.fhe_shamir_shares_batch(None, p, 4, 3, p, dev)) == "Invalid threshold parameters"
    assert err(lib.fhe_shamir_shares_batch(None, None, 2, 3, p, dev)) == "null buffer"
    assert err(lib.fhe_shamir_shares_batch(None, p, 2, 3, None, dev)) == "null buffer"
    assert err(lib.fhe_shamir_shares_batch(None, p, 2, 3, p, dev)) == "null context"
    # fhe_key_share_prepare
    assert err(lib.fhe_key_share_prepare(None, None, p, 1, dev)) == "null buffer"
    assert err(lib.fhe_key_share_prepare(None, p, None, 1, dev)) == "null buffer"
    assert err(lib.fhe_key_share_prepare(None, p, p, 1, dev)) == "null context"
    # fhe_partial_decrypt_batch: nshares == 0, batch == 0, null buffers
    assert "at least one key share" in err(lib.fhe_partial_decrypt_batch(None, p, 0, p, p, 1, dev))
    assert "at least one ciphertext" in err(lib.fhe_partial_decrypt_batch(None, p, 1, p, p, 0, dev))
    for args in ((None, 1, p, p), (p, 1, None, p), (p, 1, p, None)):
        assert err(lib.fhe_partial_decrypt_batch(None, *args, 1, dev)) == "null buffer"
    assert err(lib.fhe_partial_decrypt_batch(None, p, 1, p, p, 1, dev)) == "null context"
    # fhe_combine_partials_batch: count == 0, all three outputs null, null inputs
    assert err(lib.fhe_combine_partials_batch(None, 0, p, p, lam, 0, p, p, p, 1, dev)) == "Not enough partial decryptions"
    assert "at least one of values, phase and max_noise" in err(
        lib.fhe_combine_partials_batch(None, 0, p, p, lam, 2, None, None, None, 1, dev))
    assert err(lib.fhe_combine_partials_batch(None, 0, None, p, lam, 2, p, None, None, 1, dev)) == "null buffer"
    assert err(lib.fhe_combine_partials_batch(None, 0, p, None, lam, 2, p, None, None, 1, dev)) == "null buffer"
    assert err(lib.fhe_combine_partials_batch(None, 0, p, p, None, 2, p, None, None, 1, dev)) == "null buffer"
    assert err(lib.fhe_combine_partials_batch(None, 0, p, p, lam, 2, None, None, p, 1, dev)) == "null context"
    # fhe_lagrange_coefficients
    ids = (C.c_uint32 * 3)(1, 2, 3)
    out = (C.c_uint64 * 3)()
    assert "1 <= used <= count" in err(lib.fhe_lagrange_coefficients(97, ids, 0, 0, out))
    assert "1 <= used <= count" in err(lib.fhe_lagrange_coefficients(97, ids, 3, 0, out))
    assert "1 <= used <= count" in err(lib.fhe_lagrange_coefficients(97, ids, 3, 4, out))
    assert err(lib.fhe_lagrange_coefficients(97, None, 3, 3, out)) == "null buffer"
    assert err(lib.fhe_lagrange_coefficients(97, ids, 3, 3, None)) == "null buffer"


def reference_lambda(q, ids, i):
    """lagrange_coefficient (key_manager.cpp:548-582) in Python integers: (num, den)."""
    num = den = 1
    for j in ids:
        if j != i:
            num = num * j % q
            d = j - i
            den = den * ((q - (-d) % q) if d < 0 else d % q) % q
    return num, den


@pytest.mark.parametrize("q", [97, P27, P62, QG])
def test_lagrange_coefficients_equal_the_reference_formula(q):
    for ids, used in (([1], None), ([1, 3], None), ([5, 2, 9], None), (list(range(1, 8)), None), ([4, 1, 2, 3], 2)):
        got = fhe_gpu.lagrange_coefficients(q, ids, used)
        assert len(got) == (len(ids) if used is None else used)
        for k, lam in enumerate(got):
            num, den = reference_lambda(q, ids, ids[k])
            assert lam == num * oracle.mod_inverse(den, q) % q, (q, ids, k)
            if q < 1 << 63:  # NTTProcessor::mod_inverse is an inverse there
                assert lam == num * pow(den, -1, q) % q, (q, ids, k)
    # the coefficients interpolate at 0: sum_i lambda_i f(i) = f(0) for deg f < count
    if q < 1 << 63:
        ids = [5, 2, 9]
        f = lambda x: (11 + 7 * x + 3 * x * x) % q
        assert sum(l * f(i) for l, i in zip(fhe_gpu.lagrange_coefficients(q, ids), ids)) % q == 11


def test_lagrange_coefficients_reject_bad_ids():
    for ids in ([1, 2, 1], [0, 1], [3, 3], [0]):
        with pytest.raises(fhe_gpu.FHEError, match="share ids must be distinct and non-zero") as e:
            fhe_gpu.lagrange_coefficients(97, ids)
        assert e.value.code == -9
    with pytest.raises(fhe_gpu.FHEError):
        fhe_gpu.lagrange_coefficients(97, [1, 2], used=3)
    with pytest.raises(fhe_gpu.FHEError):
        fhe_gpu.lagrange_coefficients(97, [])


def test_python_surface_exists():
    assert callable(fhe_gpu.lagrange_coefficients)
    assert callable(fhe_gpu.KeyGenerator.threshold_keys)
    for meth in ("partial_decrypt", "combine_partial_decryptions"):
        assert callable(getattr(fhe_gpu.EncryptionEngine, meth)), meth
    assert isinstance(fhe_gpu.KeyShare.prep, property)
    tk = fhe_gpu.ThresholdKeys([], None, 2, 3)
    assert (tk.shares, tk.secret_key, tk.threshold, tk.total_shares) == ([], None, 2, 3)


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    pd = [(n, k) for n, k in zip(names, ks) if "k_partial_dec" in n]
    assert any("unsigned int" in n.split("(")[0] for n, _ in pd), [n for n, _ in pd]
    assert any("unsigned long" in n.split("(")[0] for n, _ in pd), [n for n, _ in pd]
    # every fused degree in both words
    for logn in range(2, 15):
        for w in ("unsigned int", "unsigned long"):
            assert any(n.split("(")[0].split("<")[1].startswith("%d, %s" % (logn, w)) for n, _ in pd), (logn, w)
    comb = [(n, k) for n, k in zip(names, ks) if "k_combine_partials" in n]
    assert comb
    for n, k in pd + comb:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])


def test_typescript_declares_threshold_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEThresholdEngine extends FHEAnomalyEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  partialDecryptBatch\(cts: Ciphertext\[\], share: [^)]*\): Promise<PartialDecryption\[\]>;", text, re.M)
        assert re.search(r"^  combinePartialDecryptionsBatch\(cts: Ciphertext\[\], partials: PartialDecryption\[\]\[\], "
                         r"t: number\): Promise<DecryptionResult\[\]>;", text, re.M)
    base = dts[dts.index("export interface FHEEngine {"):]
    base = base[:base.index("\n}")]
    assert "partialDecryptBatch" not in base
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in CTX_METHODS:
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth
        assert re.search(r"^  %sAsync\(" % meth, ctx, re.M), meth
    ring = dts[dts.index("export declare class PolynomialEngine {"):]
    ring = ring[:ring.index("\n}")]
    for meth in ("partialDecrypt", "combinePartials"):
        assert re.search(r"^  %s\(" % meth, ring, re.M), meth


def test_js_prototypes_have_threshold_methods():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype),"
            "r:Object.getOwnPropertyNames(m.PolynomialEngine.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    for meth in ("generateThresholdKeys", "partialDecrypt", "combinePartialDecryptions", "partialDecryptBatch",
                 "combinePartialDecryptionsBatch"):
        assert meth in out["e"], meth
    for meth in CTX_METHODS:
        assert meth in out["c"] and meth + "Async" in out["c"], meth
    for meth in ("partialDecrypt", "combinePartials"):
        assert meth in out["r"], meth
