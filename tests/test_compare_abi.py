"""CPU-side contract of the encrypted comparisons: fhe_slot_extract_batch and
fhe_lwe_sum_batch are declared, exported and bound and check their arguments
without a GPU; the Python methods exist; the typed JS surface declares
FHECompareEngine and FHEEngineImpl has the seven operations; the new kernels
use no scratch and spill no VGPR; and the extraction formula of the header
equals pyref.rotate + pyref.sample_extract on reduced words for every slot."""
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
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_slot_extract_batch": 12, "fhe_lwe_sum_batch": 12}
ENGINE_METHODS = ("compareGreaterThan", "compareLessThan", "compareEqual", "checkThreshold", "checkThresholds",
                  "checkRange", "detectDuplicate")
M64 = (1 << 64) - 1
QG = 18446744069414584321  # 2^64 - 2^32 + 1


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


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = C.c_uint64(0)
    p = C.addressof(word)
    slots = (C.c_uint32 * 2)(0, 1)
    offs = (C.c_uint64 * 2)(5, 6)

    def err(rc, code=-9):
        assert rc == code, rc
        return lib.fhe_last_error().decode()

    # fhe_slot_extract_batch: null ct / slots / lwe_a / lwe_b, nslots == 0, batch == 0, bad ref_count
    ext = lib.fhe_slot_extract_batch
    assert err(ext(None, None, None, 0, 0, slots, offs, 2, p, p, 1, dev)) == "null buffer"
    assert err(ext(None, p, None, 0, 0, None, offs, 2, p, p, 1, dev)) == "null buffer"
    assert err(ext(None, p, None, 0, 0, slots, offs, 2, None, p, 1, dev)) == "null buffer"
    assert err(ext(None, p, None, 0, 0, slots, offs, 2, p, None, 1, dev)) == "null buffer"
    assert "at least one slot" in err(ext(None, p, None, 0, 0, slots, offs, 0, p, p, 1, dev))
    assert "at least one ciphertext" in err(ext(None, p, None, 0, 0, slots, offs, 2, p, p, 0, dev))
    assert "ref_count must be 0, 1 or the batch size" in err(ext(None, p, p, 2, 0, slots, offs, 2, p, p, 3, dev))
    assert "given together" in err(ext(None, p, p, 0, 0, slots, offs, 2, p, p, 3, dev))
    assert "given together" in err(ext(None, p, None, 1, 0, slots, offs, 2, p, p, 3, dev))
    # the context is looked at after the arguments; offsets may be NULL.  (A slot >= n and an output
    # that overlaps an input are measured against the context's degree: tests/test_gpu_compare.py.)
    assert err(ext(None, p, None, 0, 0, slots, None, 2, p, p, 1, dev)) == "null context"
    assert err(ext(None, p, p, 3, 1, slots, offs, 2, p, p, 3, dev)) == "null context"
    # fhe_lwe_sum_batch: q < 2, terms == 0, batch == 0, null buffers, residence
    lsum = lib.fhe_lwe_sum_batch
    assert "modulus must be >= 2" in err(lsum(1, 4, p, p, 1, 0, p, p, 1, dev, 0, None), -8)
    assert "at least one term" in err(lsum(97, 4, p, p, 0, 0, p, p, 1, dev, 0, None))
    assert "at least one ciphertext" in err(lsum(97, 4, p, p, 1, 0, p, p, 0, dev, 0, None))
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert err(lsum(97, 4, args[0], args[1], 1, 0, args[2], args[3], 1, dev, 0, None)) == "null buffer"
    assert "where must be" in err(lsum(97, 4, p, p, 1, 0, p, p, 1, 7, 0, None))


def test_python_surface_exists():
    for meth in ("slot_extract", "lwe_sum"):
        assert callable(getattr(fhe_gpu.BootstrapEngine, meth)), meth
    for meth in ("greater_equal", "greater_than", "less_than", "check_threshold", "equal", "check_range",
                 "detect_duplicate", "encode"):
        assert callable(getattr(fhe_gpu.Comparisons, meth)), meth


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    for pat, count in (("k_slot_extract<", 2), ("k_slot_table", 1), ("k_lwe_sum", 1)):
        hits = [(n, k) for n, k in zip(names, ks) if pat in n]
        assert len(hits) == count, (pat, [n for n, _ in hits])
        for n, k in hits:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])


def test_typescript_declares_compare_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHECompareEngine extends FHEThresholdEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        for meth in ENGINE_METHODS:
            ret = r"Promise<Ciphertext\[\]>" if meth == "checkThresholds" else "Promise<Ciphertext>"
            assert re.search(r"^  %s\([^;]*bk: BootstrapKey[^;]*\): %s;" % (meth, ret), text, re.M), meth
    base = dts[dts.index("export interface FHEEngine {"):]
    base = base[:base.index("\n}")]
    for meth in ENGINE_METHODS:
        assert meth not in base, meth
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in ("slotExtract", "lweSum"):
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth
        assert re.search(r"^  %sAsync\(" % meth, ctx, re.M), meth


def test_js_prototypes_have_compare_methods():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    for meth in ENGINE_METHODS:
        assert meth in out["e"], meth
    for meth in ("slotExtract", "lweSum"):
        assert meth in out["c"] and meth + "Async" in out["c"], meth


def slot_formula(q, d0, d1, h, offset):
    """The contract of include/fhe_gpu.h on reduced words: (a [n], b)."""
    n = len(d1)
    a = [d1[h - j] if j <= h else (q - d1[n + h - j]) % q for j in range(n)]
    return a, (d0[h] + offset % q) % q


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("q", [97, 7681, QG])
def test_formula_equals_rotate_and_sample_extract(n, q):
    # raw words 0, q and 2^64 - 1 planted; the chain runs on the reduced words
    raw = [(0x9E3779B97F4A7C15 * (i + 1) * (q | 1)) & M64 for i in range(2 * n)]
    raw[0], raw[1], raw[n - 1], raw[n], raw[n + 1], raw[2 * n - 1] = 0, q, M64, M64, 0, q
    d0, d1 = [x % q for x in raw[:n]], [x % q for x in raw[n:]]
    assert 0 in d1
    for h in range(n):
        mask = pyref.rotate(d1, -h, q)
        body = pyref.rotate(d0, -h, q)
        want_a, want_b = pyref.sample_extract([mask, body], q)
        for off in (0, q - 1, M64):
            a, b = slot_formula(q, d0, d1, h, off)
            assert a == want_a, (n, q, h)
            assert b == (want_b + off % q) % q, (n, q, h, off)
            assert all(x < q for x in a) and b < q
