"""CPU-side contract of the ciphertext tally: the two C entry points are
declared, exported and bound; the k_ct_sum kernels use no scratch; the typed
JS surface declares the tally methods and FHEEngineImpl has them."""
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
ENTRY_POINTS = ["fhe_ct_sum_batch", "fhe_ct_sum_ptrs"]
TALLY_METHODS = ["tallyVotes", "tallyMultiCandidate", "updateTally", "tallyWeightedVotes"]


def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fhe_gpu.h")).read()
    lib = fhe_gpu.lib()
    bound = {s[0]: s for s in fhe_gpu.SIGNATURES}
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(fhe_ctx \*ctx, " % name, hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert len(bound["fhe_ct_sum_batch"][2]) == 8 and len(bound["fhe_ct_sum_ptrs"][2]) == 6
    # argument checks come before any device work: they answer without a GPU
    assert lib.fhe_ct_sum_batch(None, None, 2, 1, 1, 0, None, fhe_gpu.FHE_DEVICE) == -9
    assert lib.fhe_ct_sum_ptrs(None, None, 2, 1, 0, None) == -9
    for meth in ("sum_batch", "sum_buffers"):
        assert callable(getattr(fhe_gpu.PolynomialRing, meth))
    for meth in ("batch_add", "tally_votes", "tally_multi_candidate"):
        assert callable(getattr(fhe_gpu.EncryptionEngine, meth))


def test_ct_sum_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    hits = [(n, k) for n, k in zip(names, ks) if "k_ct_sum<" in n]
    assert len(hits) == 2, [n for n, _ in hits]  # contiguous and pointer-table forms
    for n, k in hits:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])


def test_typescript_declares_tally_engine():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHETallyEngine extends FHEEngine {"):]
    body = body[:body.index("\n}")]
    assert re.findall(r"^  (\w+)\(", body, re.M) == TALLY_METHODS
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for m in TALLY_METHODS:
        assert re.search(r"^  %s\(" % m, impl, re.M), m
    ctx = dts[dts.index("export declare class NttContext {"):]
    assert "sumAsync(buffers: DeviceBuffer[], out: DeviceBuffer)" in ctx[:ctx.index("\n}")]
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    assert not [m for m in TALLY_METHODS if m not in out["e"]]
    assert "sum" in out["c"] and "sumAsync" in out["c"]
