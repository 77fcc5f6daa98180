"""CPU-side contract of the public-weight tallies: the four C entry points are
declared, exported and bound and check their arguments without a GPU; the
Python methods exist; k_ct_sum_scaled exists in both addressing forms and, like
every k_ct_dot_plain kernel, uses no scratch and spills no VGPR; the typed JS
surface declares FHEPublicWeightEngine and the addon and engine have the
methods."""
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
ENTRY_POINTS = {"fhe_ct_sum_scaled_batch": 9, "fhe_ct_sum_scaled_ptrs": 7,
                "fhe_ct_dot_plain_batch": 9, "fhe_ct_dot_plain_ptrs": 7}


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
    assert lib.fhe_ct_sum_scaled_batch(None, None, None, 2, 1, 1, 0, None, dev) == -9
    assert lib.fhe_ct_sum_scaled_ptrs(None, None, None, 2, 1, 0, None) == -9
    assert lib.fhe_ct_dot_plain_batch(None, None, None, 1, 1, 0, 0, None, dev) == -9
    assert lib.fhe_ct_dot_plain_ptrs(None, None, None, 1, 0, 0, None) == -9


def test_python_methods_exist():
    for meth in ("sum_scaled", "sum_scaled_buffers"):
        assert callable(getattr(fhe_gpu.NTTProcessor, meth)), meth
        assert callable(getattr(fhe_gpu.PolynomialRing, meth)), meth
    for meth in ("tally_scalar_weighted", "dot_plain", "dot_plain_buffers"):
        assert callable(getattr(fhe_gpu.EncryptionEngine, meth)), meth


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    scaled = [(n, k) for n, k in zip(names, ks) if "k_ct_sum_scaled" in n]
    assert any("k_ct_sum_scaled<true>" in n for n, _ in scaled), [n for n, _ in scaled]
    assert any("k_ct_sum_scaled<false>" in n for n, _ in scaled), [n for n, _ in scaled]
    plain = [(n, k) for n, k in zip(names, ks) if "k_ct_dot_plain" in n]
    assert any("unsigned int" in n.split("(")[0] for n, _ in plain), [n for n, _ in plain]
    assert any("unsigned long" in n.split("(")[0] for n, _ in plain), [n for n, _ in plain]
    for n, k in scaled + plain:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])


def test_typescript_declares_public_weight_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEPublicWeightEngine extends FHEDotEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  tallyScalarWeightedVotes\(ballots: Ciphertext\[\], weights: bigint\[\]", text, re.M)
        assert re.search(r"^  dotPlain\(cts: Ciphertext\[\], pts: Plaintext\[\]", text, re.M)
    base = dts[dts.index("export interface FHEEngine {"):]
    base = base[:base.index("\n}")]
    assert "tallyScalarWeightedVotes" not in base and "dotPlain" not in base
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in ("sumScaled", "sumScaledAsync", "dotPlain", "dotPlainAsync"):
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth


def test_js_prototypes_have_public_weight_methods():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    assert "tallyScalarWeightedVotes" in out["e"] and "dotPlain" in out["e"]
    for meth in ("sumScaled", "sumScaledAsync", "dotPlain", "dotPlainAsync"):
        assert meth in out["c"], meth
