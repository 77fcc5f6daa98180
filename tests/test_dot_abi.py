"""CPU-side contract of the ciphertext inner product: the two C entry points
are declared, exported and bound and check their arguments without a GPU; the
Python methods exist; every k_ct_dot kernel uses no scratch and spills no
VGPR; the typed JS surface declares FHEDotEngine and the addon and engine
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
ENTRY_POINTS = ["fhe_ct_dot_batch", "fhe_ct_dot_ptrs"]


def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fhe_gpu.h")).read()
    lib = fhe_gpu.lib()
    bound = {s[0]: s for s in fhe_gpu.SIGNATURES}
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(fhe_ctx \*ctx, " % name, hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert len(bound["fhe_ct_dot_batch"][2]) == 9 and len(bound["fhe_ct_dot_ptrs"][2]) == 7
    # argument checks come before any device work: they answer without a GPU
    assert lib.fhe_ct_dot_batch(None, None, None, 1, 1, 0, 0, None, fhe_gpu.FHE_DEVICE) == -9
    assert lib.fhe_ct_dot_ptrs(None, None, None, 1, 0, 0, None) == -9


def test_python_methods_exist():
    for meth in ("dot", "dot_buffers", "tally_weighted_votes"):
        assert callable(getattr(fhe_gpu.EncryptionEngine, meth)), meth


def test_ct_dot_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    hits = [(n, k) for n, k in zip(names, ks) if "k_ct_dot" in n]
    assert any("unsigned int" in n.split("(")[0] for n, _ in hits), [n for n, _ in hits]
    assert any("unsigned long" in n.split("(")[0] for n, _ in hits), [n for n, _ in hits]
    for n, k in hits:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])
    assert not [n for n, _ in hits if "k_ct_sum<" in n]


def test_typescript_declares_dot_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEDotEngine extends FHETallyEngine {"):]
    body = body[:body.index("\n}")]
    assert re.search(r"^  dotProduct\(", body, re.M)
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    assert re.search(r"^  dotProduct\(", impl, re.M)
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    assert re.search(r"^  dot\(", ctx, re.M) and re.search(r"^  dotAsync\(", ctx, re.M)


def test_js_prototypes_have_dot():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    assert "dotProduct" in out["e"]
    assert "dot" in out["c"] and "dotAsync" in out["c"]
