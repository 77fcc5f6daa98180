"""C-ABI checks that need no GPU: the library loads, exports every entry
point include/fhe_gpu.h declares, validates parameters with the reference's
messages, computes the host-side constants bit-exactly, and refuses to
compute without a device (no CPU fallback)."""
import json
import os
import re

import numpy as np
import pytest

import oracle
import fhe_gpu
from fhe_gpu import FHEError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fhe_gpu.h")
P27 = 132120577
P62 = 4611686018326724609


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(fhe_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_exports_every_declared_symbol():
    lib = fhe_gpu.lib()
    declared = header_functions()
    assert len(declared) >= 40
    missing = [n for n in declared if not hasattr(lib, n)]
    assert not missing, missing
    # and the Python binding covers all of them
    bound = {s[0] for s in fhe_gpu.SIGNATURES}
    assert set(declared) <= bound, set(declared) - bound


def test_library_is_gfx950_code_object():
    so = fhe_gpu.LIB_PATH
    blob = open(so, "rb").read()
    assert b"gfx950" in blob
    assert b"amdgcn-amd-amdhsa" in blob


def test_version_and_detect():
    assert "gfx950" in fhe_gpu.version()
    caps = fhe_gpu.detect_hardware()
    assert caps["deviceCount"] >= 0


@pytest.mark.parametrize(
    "n,q,code,msg",
    [
        (12, 97, -1, "Polynomial degree must be a power of 2"),
        (0, 97, -1, "Polynomial degree must be a power of 2"),
        (2, 97, -2, "Polynomial degree must be between 4 and 65536"),
        (131072, 97, -2, "Polynomial degree must be between 4 and 65536"),
        (8, 96, -3, "Modulus must be odd"),
        (16, 17, -4, "Modulus is not NTT-friendly"),
    ],
)
def test_ctx_validation_messages(n, q, code, msg):
    with pytest.raises(FHEError) as ei:
        fhe_gpu.NTTProcessor(n, q)
    assert ei.value.code == code
    assert msg in str(ei.value)


def test_no_cpu_fallback_without_device(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is present")
    with pytest.raises(FHEError) as ei:
        fhe_gpu.NTTProcessor(1024, P27)
    assert ei.value.code == -11
    with pytest.raises(FHEError) as ei:
        fhe_gpu.modmul_batch(P27, np.ones(8, np.uint64), np.ones(8, np.uint64))
    assert ei.value.code == -11


def test_compat_modular_arithmetic_matches_oracle():
    rng = np.random.default_rng(0)
    for q in (P27, P62, 97, 12289, 7681, 2 ** 61 - 1):
        m = fhe_gpu.ModularArithmetic(q)
        k = oracle.mont_constants(q)
        assert m.constants == k
        for _ in range(200):
            a, b = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 63))
            assert m.montgomery_mul(a, b) == oracle.mont_mul(k, a, b)
            assert m.to_montgomery(a) == oracle.to_mont(k, a)
            assert m.from_montgomery(a) == oracle.from_mont(k, a)
            assert m.mod_add(a, b) == oracle.mod_add(q, a, b)
            assert m.mod_sub(a, b) == oracle.mod_sub(q, a, b)
        assert m.get_modulus() == q


def test_compat_aarch64_division_semantics():
    # gcd(q, 2^64-1) > 1 traps on x86 in the reference; AArch64 result here
    for q in (17, 257, 65537):
        assert fhe_gpu.ModularArithmetic(q).constants == oracle.mont_constants(q)


def test_modular_arithmetic_errors():
    with pytest.raises(FHEError, match="Modulus must be positive"):
        fhe_gpu.ModularArithmetic(0)
    with pytest.raises(FHEError, match="odd and non-zero"):
        fhe_gpu.ModularArithmetic(96)
    m = fhe_gpu.ModularArithmetic(97)
    with pytest.raises(FHEError, match="non-negative"):
        m.montgomery_mul(-1, 3)


def test_multi_limb_constants(golden_dir):
    with open(os.path.join(golden_dir, "multi_limb.json")) as f:
        cases = json.load(f)
    for c in cases:
        assert fhe_gpu.MultiLimbModularArithmetic(c["q"]).constants == c["constants"]
    # sparse modulus exercising the reference's truncated long division
    for qm in ([1, 1 << 63], [3, 1 << 62], [0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF]):
        assert fhe_gpu.MultiLimbModularArithmetic(qm).constants == oracle.ml_constants(qm)


def test_static_helpers_match_reference(golden_dir):
    with open(os.path.join(golden_dir, "reference_kat.json")) as f:
        kat = json.load(f)
    P = fhe_gpu.NTTProcessor
    for i, r in kat["bit_reverse_3"]:
        assert P.bit_reverse(i, 3) == r
    for b, e, m, r in kat["mod_pow"]:
        assert P.mod_pow(b, e, m) == r
    for n, q, psi in kat["psi_table"]:
        assert P.find_primitive_root(n, q) == psi


def test_rns_ring_validation():
    """PolynomialRing(degree, moduli) with no modulus (polynomial_ring.cpp:
    228-230) fails before any device work."""
    import fhe_gpu

    with pytest.raises(fhe_gpu.FHEError, match="At least one modulus required"):
        fhe_gpu.RNSPolynomialRing(1024, [])


def test_parameter_presets():
    """parameter_set.cpp presets as data, and which moduli the GPU can run
    (Q_40_1, Q_40_2, Q_50_2 are composite; Q_50_1 stops at N = 8192)."""
    from fhe_gpu import params as P

    assert P.create_parameter_set("tfhe-128-fast").lwe_dimension == 742
    with pytest.raises(ValueError, match="Unknown parameter preset: nope"):
        P.create_parameter_set("nope")
    assert P.Q_40_1 == 257 * 4278255361
    assert not P._is_prime(P.Q_40_1) and not P._is_prime(P.Q_40_2) and not P._is_prime(P.Q_50_2)
    assert P._is_prime(P.Q_60_1) and P._is_prime(P.Q_50_1) and P._is_prime(132120577)
    fast = P.gpu_moduli(P.create_parameter_set("tfhe-128-fast"))
    assert not fast[0]["usable"]
    ckks = P.gpu_moduli(P.create_parameter_set("ckks-128-ml"))
    assert [m["usable"] for m in ckks] == [True, False, False, False, False]  # only Q_60_1 admits N = 16384
    assert all(m["usable"] for m in P.gpu_moduli(P.create_parameter_set("bfv-128-simd")))


# ------------------------------------------------------------ register budget
# Kernels of the measured paths must run without scratch:
# the BASELINE workloads (C3 fwd+modmul, C4 polymul, both primes), the
# transforms, the external product and the single-launch blind rotation.
SCRATCH_FREE = [
    "k_ntt_fwd_mul<14, unsigned int, true>", "k_ntt_fwd_mul<1294, unsigned long, false>",
    "k_polymul2<1294, unsigned int, true>", "k_polymul2<14, unsigned long, ",
    "k_ntt_fwd<14, unsigned int, true, 0>", "k_ntt_fwd<1294, unsigned long, ",
    "k_ntt_inv<14, unsigned int>", "k_ntt_inv<14, unsigned long>",
    "k_extprod_acc<", "k_extprod2<14, unsigned long>", "k_br_persist<", "k_decrypt<",
    # round 4: the two-CU blind rotation, k = 2..4 single launch, the RNS limb kernels
    "k_br_pair<", "k_br_multi<", "k_br_persist_k<", "k_ntt_fwd_limbs<", "k_ntt_inv_limbs<", "k_polymul_limbs<",
    "k_polymul2_limbs<",
]
# Measured exceptions inside SCRATCH_FREE's patterns, each pinned to its
# spill count (so it cannot grow unnoticed): the spill-free variant of each
# measured slower on MI355X.
SCRATCH_EXEMPT = {
    # tfhe-256-secure's three digit levels in lockstep: 4 VGPRs spilled,
    # 29.6 ms vs 31.0 ms one level at a time
    "k_br_pair<12, unsigned long, 3>": 4,
    "k_br_pair<16396, unsigned long, 3>": 4,  # the same kernel with unit twiddles (gk_compat(12))
}
# Ratchet over EVERY kernel with scratch, the exempt ones included:
# 95 in round 2, 70 before the negacyclic mode moved into the stage tables,
# 35 at the start of round 6; 22 after the flag-free 64-bit arithmetic moved
# into ntt_inv / ntt_ext / ntt_cipher / ntt_engine_enc and k_sample lost its
# indexed local array (round 6).  The count may only go down.
SCRATCH_CEILING = 22


def test_kernel_scratch_budget():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    import glob

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    for pat in SCRATCH_FREE:
        hits = [(n, k) for n, k in zip(names, ks) if pat in n]
        assert hits, f"no kernel matches {pat}"
        for n, k in hits:
            pinned = [v for x, v in SCRATCH_EXEMPT.items() if x in n]
            if pinned:
                assert k["vgpr_spill"] <= pinned[0], (n, k["vgpr_spill"], pinned[0])
                continue
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])
    with_scratch = [n for n, k in zip(names, ks) if k["scratch"]]
    assert len(with_scratch) <= SCRATCH_CEILING, with_scratch


# ---------------------------------------------------- compile-time switches
# Every FHE_* name the kernel sources test in a preprocessor conditional.  The
# first seven are the axes on which the shipped .hip units differ (each unit
# sets them before its includes), the last two the diagnostics builds of
# DESIGN.md.  A variant that lost its A/B is deleted, not parked behind a new
# switch: adding a name here is a reviewed change, like SCRATCH_CEILING.
COMPILE_SWITCHES = {
    "FHE_NS", "FHE_U64_NOVCC", "FHE_MULHI64", "FHE_SPLIT_X64", "FHE_STREAM_TW2", "FHE_STREAM_DEPTH",
    "FHE_OPAQUE_TW", "FHE_DEBUG_SLOTS", "FHE_BR_STAMPS",
}


def test_compile_switches_are_the_listed_ones():
    import glob
    import re

    csrc = os.path.join(ROOT, "node-fhe-accelerate_amd", "csrc")
    files = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))
    assert files
    found = {}
    for path in files:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    for name in re.findall(r"\bFHE_\w+", line):
                        found.setdefault(name, f"{os.path.basename(path)}:{no}")
    assert set(found) == COMPILE_SWITCHES, {n: w for n, w in found.items() if n not in COMPILE_SWITCHES}


# ------------------------------------------------------------ config flags
def test_env_defaults_python(monkeypatch):
    """FHE_NTT_MODE / FHE_GPU_DEVICES fill the context
    arguments a caller leaves unset; explicit arguments win."""
    import fhe_gpu as fg

    monkeypatch.delenv("FHE_NTT_MODE", raising=False)
    monkeypatch.delenv("FHE_GPU_DEVICES", raising=False)
    assert fg.env_defaults() == ("compat", 0, None)
    monkeypatch.setenv("FHE_NTT_MODE", "negacyclic")
    monkeypatch.setenv("FHE_GPU_DEVICES", "2")
    assert fg.env_defaults() == ("negacyclic", 2, None)
    monkeypatch.setenv("FHE_GPU_DEVICES", "1, 3")
    assert fg.env_defaults() == ("negacyclic", 1, [1, 3])
    assert fg.env_defaults("compat", 5, None) == ("compat", 5, None)
    assert fg.env_defaults(None, None, [4]) == ("negacyclic", 4, [4])
    monkeypatch.setenv("FHE_GPU_DEVICES", "a,b")
    with pytest.raises(fg.FHEError):
        fg.env_defaults()


def test_env_defaults_js():
    import shutil
    import subprocess

    if not shutil.which("node"):
        pytest.skip("node not installed")
    js = os.path.join(ROOT, "node-fhe-accelerate_amd", "lib", "engine.js")
    code = (f"const e=require({js!r});const r=[];"
            "process.env.FHE_GPU_DEVICES='0,1';r.push(e.envDefaults({}));"
            "process.env.FHE_NTT_MODE='negacyclic';process.env.FHE_GPU_DEVICES='3';r.push(e.envDefaults({}));"
            "r.push(e.envDefaults({mode:'compat',device:2}));"
            "let bad=false;process.env.FHE_GPU_DEVICES='x';try{e.envDefaults({})}catch(_){bad=true}r.push(bad);"
            "console.log(JSON.stringify(r));")
    env = {k: v for k, v in os.environ.items() if k not in ("FHE_NTT_MODE", "FHE_GPU_DEVICES")}
    out = subprocess.run(["node", "-e", code], capture_output=True, text=True, env=env, check=True).stdout
    import json

    r = json.loads(out)
    assert r[0] == {"mode": "compat", "device": 0, "devices": [0, 1]}
    assert r[1] == {"mode": "negacyclic", "device": 3}
    assert r[2] == {"mode": "compat", "device": 2}
    assert r[3] is True


# ------------------------------------------------------------ measurement plumbing
def test_build_id_and_bench_kernels_exist():
    """fhe_build_id() is the Makefile's source hash, and every exact kernel
    symbol bench.py attaches a profile to (BENCH_KERNELS) is in the build: a
    renamed or re-templated kernel must update the table, never silently
    match a stale profile."""
    import glob
    import sys

    bid = fhe_gpu.build_id()
    assert re.fullmatch(r"[0-9a-f]{16}", bid), bid
    hdr = os.path.join(ROOT, "node-fhe-accelerate_amd", "build", "obj", "build_id.h")
    if os.path.exists(hdr):
        assert bid in open(hdr).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    names = set(kr.demangle([k["name"] for k in kr.kernels()]))
    sys.path.insert(0, ROOT)
    import bench

    missing = {k: s for k, s in bench.BENCH_KERNELS.items() if s not in names}
    assert not missing, missing


def test_typescript_declarations_match_exports():
    """index.d.ts (the typed surface a TS caller binds against): every
    declared value is exported by lib/index.js, and every method of the
    reference FHEEngine interface (fhe-engine.ts:33-78, restated there)
    exists on FHEEngineImpl.  No tsc in this image, so the check is by name."""
    import shutil
    import subprocess

    if not shutil.which("node"):
        pytest.skip("node not installed")
    pkg = os.path.join(ROOT, "node-fhe-accelerate_amd")
    addon = os.path.join(pkg, "build", "fhe_napi.node")
    if not os.path.exists(addon):
        pytest.skip("N-API addon not built")
    dts = open(os.path.join(pkg, "index.d.ts")).read()
    values = set(re.findall(r"^export (?:declare )?(?:function|class|const|enum) (\w+)", dts, re.M))
    body = dts[dts.index("export interface FHEEngine {"):]
    body = body[:body.index("\n}")]
    methods = re.findall(r"^\s+(\w+)\(", body, re.M)
    assert len(methods) == 44, len(methods)
    code = ("const m=require(%r);const E=m.FHEEngineImpl.prototype;"
            "console.log(JSON.stringify({keys:Object.keys(m),"
            "methods:Object.getOwnPropertyNames(E)}))" % os.path.join(pkg, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    missing = sorted(v for v in values if v not in out["keys"])
    assert not missing, missing
    absent = sorted(m for m in methods if m not in out["methods"])
    assert not absent, absent


def test_profile_traffic_requires_exact_kernel_and_build(tmp_path, monkeypatch):
    """bench.py attaches a PMC traffic figure only from a summary of the exact
    kernel it launches on the exact build loaded: a stale
    build id, a different instantiation or another workload is ignored."""
    import json
    import sys

    sys.path.insert(0, ROOT)
    import bench

    bid = fhe_gpu.build_id()
    sym = bench.BENCH_KERNELS["polymul/q27"]
    wl = {"kernel": "polymul", "n": 16384, "batch": 65536, "q": bench.P27}

    def put(name, **kw):
        d = tmp_path / "profiles" / name
        d.mkdir(parents=True)
        s = {"build_id": bid, "kernel_name": sym, "hbm_traffic_bytes_per_launch": 1.0, "workload": dict(wl),
             "generated": "2026-01-01T00:00:00Z", "kernel_trace_full_batch": {"avg_ns": 5e6}}
        s.update(kw)
        (d / "summary.json").write_text(json.dumps(s))

    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    put("stale", build_id="0" * 16, hbm_traffic_bytes_per_launch=2.0, generated="2026-02-01T00:00:00Z")
    put("other_kernel", kernel_name=sym.replace("true", "false"), hbm_traffic_bytes_per_launch=3.0,
        generated="2026-02-01T00:00:00Z")
    put("other_workload", workload=dict(wl, batch=8192), hbm_traffic_bytes_per_launch=4.0,
        generated="2026-02-01T00:00:00Z")
    assert bench.pmc_traffic("polymul", 16384, 65536, bench.P27) is None
    put("match")
    tr = bench.pmc_traffic("polymul", 16384, 65536, bench.P27)
    assert tr is not None and tr[0] == 1.0 and tr[1].endswith("match/summary.json") and tr[2] == 5.0


def test_valu_roofline_arithmetic():
    """The VALU-issue roofline bench.py attaches (tools/valu_roofline.py,
    VERDICT r5 next #1), recomputed by hand on a fixture summary: issue floor
    = dynamic VALU instructions x mix-weighted cycles (256 / measured rate;
    unmeasured mnemonics at the full-rate 2 cycles) / (1024 SIMDs x 2.4 GHz),
    and the HBM fraction priced on the profile's own kernel time."""
    import json
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import valu_roofline as vr

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "valu_roofline_fixture.json")))
    s, rates = fx["summary"], fx["rates"]
    mix = s["valu_static_mix"]
    total = sum(mix.values())
    cyc = sum(c * (256.0 / rates[m] if m in rates else 2.0) for m, c in mix.items()) / total
    insts = s["pmc_per_launch_avg"]["SQ_INSTS_VALU"]
    floor_ms = insts * cyc / (256 * 4) / 2.4e9 * 1e3
    prof_ms = s["kernel_trace_full_batch"]["avg_ns"] / 1e6
    r = vr.valu_roofline(s, rates, kernel_ms=fx["event_kernel_ms"])
    assert abs(r["issue_floor_ms"] - floor_ms) < 1e-9 * floor_ms
    assert abs(r["frac_profile"] - floor_ms / prof_ms) < 1e-12
    assert abs(r["frac"] - floor_ms / fx["event_kernel_ms"]) < 1e-12
    assert abs(r["unmeasured_share"] - 66 / total) < 1e-12
    assert abs(r["achieved_inst_per_cu_cycle_profile"] - insts / (256 * 2.4e9 * prof_ms * 1e-3)) < 1e-12
    # the numbers themselves: 2.48 G wave-instructions at ~3.66 cycles each
    # take ~3.78 ms of the 6.14 ms kernel
    assert 3.7 < r["issue_floor_ms"] < 3.85 and 0.6 < r["frac_profile"] < 0.63
    fp = vr.hbm_frac_profile(s, fx["algorithmic_bytes"])
    assert abs(fp - fx["algorithmic_bytes"] / (prof_ms * 1e-3) / 8e12) < 1e-12
    # at the clock the kernel held (GRBM_GUI_ACTIVE / 8 per ms) the floor
    # scales by 2.4 GHz / that clock
    assert "issue_floor_ms_at_held_clock" not in r
    r2 = vr.valu_roofline(dict(s, effective_clock_ghz=2.0), rates, kernel_ms=fx["event_kernel_ms"])
    assert abs(r2["issue_floor_ms_at_held_clock"] - floor_ms * 1.2) < 1e-9 * floor_ms
    assert abs(r2["frac_at_held_clock"] - floor_ms * 1.2 / fx["event_kernel_ms"]) < 1e-12
    # a summary without the counters or the mix gives no roofline
    assert vr.valu_roofline({"kernel_trace_full_batch": s["kernel_trace_full_batch"]}, rates) is None
    # the committed rate table parses and prices the multiplies at half rate
    table = vr.load_rates()
    assert table and 3.5 < 256.0 / table["v_mad_u64_u32"] < 5 and 256.0 / table["v_add_u32"] < 2.5


def test_key_switch_rejects_entry_count_overflow():
    """the key-switch kernels index the (coefficient, level)
    entries in 32 bits, so in_dim * level >= 2^32 is refused up front
    (FHE_ERR_INVALID_ARG) instead of summing the wrong entries -- checked
    before any device work, so it runs without a GPU."""
    lib = fhe_gpu.lib()
    rc = lib.fhe_key_switch_batch(P27, 4, 2, 1 << 31, 16, None, None, None, None, None, None, 0, 1, 0, None)
    assert rc == -9, rc
    assert "below 2^32" in lib.fhe_last_error().decode()
    # the limit itself is fine for the shape check (batch 0: nothing to run)
    assert lib.fhe_key_switch_batch(P27, 4, 2, (1 << 31) - 1, 16, None, None, None, None, None, None, 0, 1, 0,
                                    None) == 0


def test_cpu_calibration_record():
    """bench.py's cpu_baseline.calibration: the committed
    tools/calibrate_cpu.py run, per config port time / compiled-reference
    time, and the later rerun carried beside it."""
    import json
    import sys

    sys.path.insert(0, ROOT)
    import bench

    cal = bench.cpu_calibration(16384, 132120577)
    raw = json.load(open(os.path.join(ROOT, "profiles", "r6_cpu_calibration.json")))
    assert cal["ratio_median_all_configs"] == raw["ratio_median"]
    fw = cal["forward_ntt_N16384"]
    assert fw["reference_us"] == 2843.0 and abs(fw["ratio"] - fw["port_us"] / 2843.0) < 1e-12
    assert cal["multiply_N16384"]["reference_us"] == 8603.0
    assert cal["within_10pct_at_this_config"] == (0.9 <= fw["ratio"] <= 1.1)
    assert len(raw["rows"]) == 12 and all(r["ratio"] == r["port_us"] / r["reference_us"] for r in raw["rows"])
    assert "rerun" in cal and cal["rerun"]["ratio_range"][0] <= cal["rerun"]["ratio_median_all_configs"]
