"""CPU-side contract of ciphertext squaring and the anomaly score: the two C
entry points are declared, exported and bound and check their arguments
without a GPU; the Python methods exist; every k_ct_sq kernel and the
NTT-domain k_square_ntt use no scratch and spill no VGPR, in 32- and 64-bit
words; the typed JS surface declares FHEAnomalyEngine and the addon and engine
have the methods."""
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import fhe_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_ct_square_batch": 8, "fhe_ct_square_relin_batch": 10}
CTX_METHODS = ("ctSquare", "ctSquareAsync", "ctSquareRelinPrepared", "ctSquareRelinPreparedAsync")


def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fhe_gpu.h")).read()
    lib = fhe_gpu.lib()
    bound = {s[0]: s for s in fhe_gpu.SIGNATURES}
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"^int %s\((fhe_ctx \*ctx, [^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name
        assert name in bound, name
        assert len(bound[name][2]) == nargs, name
    assert "#define FHE_GPU_ABI_VERSION 1" in hdr
    # argument checks come before any device work: they answer without a GPU
    dev = fhe_gpu.FHE_DEVICE
    assert lib.fhe_ct_square_batch(None, None, None, 0, None, 1, 0, dev) == -9
    assert lib.fhe_ct_square_relin_batch(None, 4, 7, None, None, 0, None, None, 1, dev) == -9
    # a ref without a count, and a count that is neither 1 nor the batch
    import ctypes as C

    word = C.c_uint64(0)
    p = C.addressof(word)
    assert lib.fhe_ct_square_batch(None, p, p, 0, p, 5, 0, dev) == -9
    assert b"ref and ref_count" in lib.fhe_last_error()
    assert lib.fhe_ct_square_batch(None, p, p, 2, p, 5, 0, dev) == -9
    assert b"ref_count must be 0, 1 or the batch size" in lib.fhe_last_error()
    assert lib.fhe_ct_square_relin_batch(None, 4, 7, p, p, 2, p, p, 5, dev) == -9
    assert b"ref_count must be 0, 1 or the batch size" in lib.fhe_last_error()


def test_python_methods_exist():
    for meth in ("square", "square_relin", "squared_difference", "compute_anomaly_score"):
        assert callable(getattr(fhe_gpu.EncryptionEngine, meth)), meth


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    sq = [(n, k) for n, k in zip(names, ks) if "k_ct_sq" in n]
    assert any("unsigned int" in n.split("(")[0] for n, _ in sq), [n for n, _ in sq]
    assert any("unsigned long" in n.split("(")[0] for n, _ in sq), [n for n, _ in sq]
    # plain and subtract-on-load instantiations of both
    for w in ("unsigned int", "unsigned long"):
        for diff in ("true>", "false>"):
            assert any(w in n.split("(")[0] and n.split("(")[0].endswith(diff) for n, _ in sq), (w, diff)
    ntt = [(n, k) for n, k in zip(names, ks) if "k_square_ntt" in n]
    assert any("k_square_ntt<true>" in n for n, _ in ntt) and any("k_square_ntt<false>" in n for n, _ in ntt), ntt
    for n, k in sq + ntt:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])


def test_typescript_declares_anomaly_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEAnomalyEngine extends FHEPublicWeightEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  computeAnomalyScore\(ballot: Ciphertext, expected: Ciphertext, ek: EvaluationKey\)", text, re.M)
    base = dts[dts.index("export interface FHEEngine {"):]
    base = base[:base.index("\n}")]
    assert "computeAnomalyScore" not in base
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in CTX_METHODS:
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth
    ring = dts[dts.index("export declare class PolynomialEngine {"):]
    assert re.search(r"^  ctSquare\(", ring[:ring.index("\n}")], re.M)


def test_js_prototypes_have_squaring_methods():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype),"
            "r:Object.getOwnPropertyNames(m.PolynomialEngine.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    for meth in ("square", "squareRelin", "computeAnomalyScore"):
        assert meth in out["e"], meth
    for meth in CTX_METHODS:
        assert meth in out["c"], meth
    assert "ctSquare" in out["r"]
