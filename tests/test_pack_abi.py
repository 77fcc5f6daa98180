"""CPU-side contract of the LWE-to-RLWE packing: fhe_lwe_pack_batch and
fhe_pack_key_generate are declared, exported and bound and check their
arguments without a GPU; the Python methods exist; the typed JS surface declares
FHEPackEngine; the new kernels use no scratch and spill no VGPR; the header
formula equals pyref.key_switch (out_dim = 2n) + a body add + pyref.rotate +
modular sums for every slot; and, in exact integers, the packed ciphertext
decrypts to the planted messages with its noise below q / (4 t).

The header declares the two entry points with 13 and 11 arguments (count the
prototypes of include/fhe_gpu.h: ctx, base_log, level, in_dim, pack_key, lwe_a,
lwe_b, slots, nslots, accumulate, out, batch, where; and ctx, base_log, level,
sk, lwe_sk, lwe_dim, seed, stream, std_dev, pack_key, where)."""
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fhe_gpu
import pack_ref as R
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_lwe_pack_batch": 13, "fhe_pack_key_generate": 11}
ENGINE_METHODS = ("generatePackKey", "packBits")
M64 = (1 << 64) - 1


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
    # the contract is in the header
    for text in ("fhe_lwe_pack_batch       the packing key switch", "W_s[p][j]", "(q - W_s[p][n+j-h]) % q",
                 "fhe_pack_key_generate       the key of fhe_lwe_pack_batch", "FHE_MODE_NEGACYCLIC",
                 "NOT the\n *   q >> ((l+1) base_log) of fhe_ksk_generate"):
        assert text in hdr, text


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = C.c_uint64(0)
    p = C.addressof(word)
    slots = (C.c_uint32 * 2)(0, 1)

    def err(rc, code=-9):
        assert rc == code, rc
        return lib.fhe_last_error().decode()

    pack = lib.fhe_lwe_pack_batch
    # a null pack_key, lwe_a, lwe_b, slots or out
    for i in range(5):
        a = [p, p, p, slots, p]
        a[i] = None
        assert err(pack(None, 4, 2, 3, a[0], a[1], a[2], a[3], 2, 0, a[4], 1, dev)) == "null buffer", i
    assert "at least one slot" in err(pack(None, 4, 2, 3, p, p, p, slots, 0, 0, p, 1, dev))
    assert "at least one ciphertext" in err(pack(None, 4, 2, 3, p, p, p, slots, 2, 0, p, 0, dev))
    assert "in_dim and level" in err(pack(None, 4, 2, 0, p, p, p, slots, 2, 0, p, 1, dev))
    assert "in_dim and level" in err(pack(None, 4, 0, 3, p, p, p, slots, 2, 0, p, 1, dev))
    # the shift limits of relinearisation: 1 <= base_log <= 63, (level - 1) base_log < 64
    for bl, lv in ((0, 2), (64, 1), (32, 3), (22, 4)):
        assert "invalid decomposition" in err(pack(None, bl, lv, 3, p, p, p, slots, 2, 0, p, 1, dev)), (bl, lv)
    assert "below 2^31" in err(pack(None, 4, 2, 1 << 31, p, p, p, slots, 2, 0, p, 1, dev))
    # the context is looked at after the arguments.  (A slot >= n and an output that overlaps an
    # input are measured against the context's degree: tests/test_gpu_pack.py.)
    assert err(pack(None, 4, 2, 3, p, p, p, slots, 2, 0, p, 1, dev)) == "null context"
    assert err(pack(None, 63, 1, 3, p, p, p, slots, 2, 1, p, 1, dev)) == "null context"
    assert err(pack(None, 32, 2, 3, p, p, p, slots, 2, 1, p, 1, dev)) == "null context"


def test_python_surface_exists():
    assert callable(fhe_gpu.KeyGenerator.pack_key)
    assert callable(fhe_gpu.EncryptionEngine.pack_lwe)
    assert callable(fhe_gpu.Comparisons.pack)
    k = fhe_gpu.PackKey(np.zeros((6, 2, 4), np.uint64), 7, 2, 3)
    assert (k.base_log, k.level, k.lwe_dim) == (7, 2, 3) and k.key.shape == (6, 2, 4)


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    for pat, count in (("k_lwe_pack<", 8), ("k_pack_table", 1), ("k_pack_key_finish", 1)):
        hits = [(n, k) for n, k in zip(names, ks) if pat in n]
        assert len(hits) == count, (pat, [n for n, _ in hits])
        for n, k in hits:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])


def test_typescript_declares_pack_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEPackEngine extends FHECompareEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  generatePackKey\(sk: SecretKey, bk: BootstrapKey[^;]*\): Promise<PackKey>;", text, re.M)
        assert re.search(r"^  packBits\(bits: Ciphertext\[\], slots: number\[\], packKey: PackKey\): Promise<Ciphertext>;",
                         text, re.M)
    for name in ("FHEEngine", "FHECompareEngine"):
        base = dts[dts.index("export interface %s " % name):]
        base = base[:base.index("\n}")]
        for meth in ENGINE_METHODS:
            assert meth not in base, (name, meth)
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in ("lwePack", "lwePackAsync", "packKeyGenerate"):
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth


def test_js_prototypes_have_pack_methods():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    for meth in ENGINE_METHODS:
        assert meth in out["e"], meth
    for meth in ("lwePack", "lwePackAsync", "packKeyGenerate"):
        assert meth in out["c"], meth


def planted(seed, q, count):
    """Full-range u64 words with 0, q and 2^64 - 1 planted."""
    w = [(0x9E3779B97F4A7C15 * (i + seed) * (q | 1) + (seed << 40)) & M64 for i in range(count)]
    for i, v in enumerate((0, q, M64)):
        w[(i * 5 + seed) % count] = v
    return w


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("q", [97, 7681])
def test_formula_equals_key_switch_rotate_and_sums(n, q):
    bl, lv, in_dim = (2, 4, 3) if q == 97 else (5, 3, 2)
    entries = in_dim * lv
    slots = list(range(n)) + [0, n - 1, n - 1]  # every slot, and repeats
    S = len(slots)
    key = planted(1, q, entries * 2 * n)
    key = [[key[(e * 2 + p) * n:(e * 2 + p + 1) * n] for p in range(2)] for e in range(entries)]
    flat_a = planted(2, q, S * in_dim)
    lwe_b = planted(3, q, S)
    prev = [planted(4, q, n), planted(5, q, n)]
    for w in ([x for row in key for half in row for x in half], flat_a, lwe_b, prev[0], prev[1]):
        assert {0, q, M64} <= set(w), "raw words planted"
    lwe_a = [flat_a[s * in_dim:(s + 1) * in_dim] for s in range(S)]
    lwe_a[-2] = [0] * in_dim                 # every digit zero
    lwe_a[-1] = [M64] * in_dim               # every digit 2^base_log - 1
    # the chain per slot: key switch to 2n words against the key viewed as [entries][2n], zero body
    # key and zero body; + b mod q on coefficient 0 of the first half; X^h (mask = second half, body =
    # first half); modular sums over the slots
    ksk = [row[0] + row[1] for row in key]
    want = [[0] * n, [0] * n]
    for s, h in enumerate(slots):
        a, b, wraps, _ = pyref.key_switch(ksk, [0] * entries, lwe_a[s], 0, q, bl, lv, out_dim=2 * n)
        assert b == 0 and wraps == 0
        first, second = a[:n], a[n:]
        first[0] = (first[0] + lwe_b[s] % q) % q
        rot = [pyref.rotate(first, h, q), pyref.rotate(second, h, q)]
        want = [[(x + y) % q for x, y in zip(want[p], rot[p])] for p in range(2)]
    got = R.pack_formula_int(q, n, bl, lv, key, lwe_a, lwe_b, slots)
    assert got == want, (n, q)
    assert all(x < q for row in got for x in row)
    acc = R.pack_formula_int(q, n, bl, lv, key, lwe_a, lwe_b, slots, prev)
    assert acc == [[(x + y % q) % q for x, y in zip(want[p], prev[p])] for p in range(2)]
    # the numpy restatement used on the GPU side gives the same words
    u = lambda x: np.array(x, dtype=np.uint64)
    vec = R.pack_formula(q, n, bl, lv, u(key), u(lwe_a)[None], u(lwe_b)[None], slots, u(prev)[None])
    assert vec.tolist() == [acc]


def test_packed_ciphertext_decrypts_in_exact_integers():
    n, q, t, bl, lv, dim = 16, 7681, 4, 7, 2, 6
    assert bl * lv >= (q - 1).bit_length()  # the digits recompose every mask word
    delta = q // t
    rng = np.random.default_rng(20261021)
    sk = [int(v) for v in rng.integers(-1, 2, size=n)]
    lwe_sk = [int(v) for v in rng.integers(-1, 2, size=dim)]
    assert -1 in lwe_sk and 0 in lwe_sk and 1 in lwe_sk
    msgs, slots = [3, 1, 2, 3], [0, 5, 11, 15]
    # The pack key of fhe_pack_key_generate with errors in {-1, 0, 1}: row e carries eps_e X^e.
    # The packed noise at coefficient j is sum_s d(s, e) eps_e over the ONE row e = (j - h_s) mod n
    # of each slot (rows e >= dim lv do not exist), so it is at most the sum of the digit caps of
    # those rows: (q - 1) >> bl for a high digit (l = 0), 2^bl - 1 for a low one.  With these slots
    # that worst case stays below q / (4 t), whatever the masks and the signs are.  (Dense errors
    # would not: 12 rows of 16 coefficients each give a noise of standard deviation ~ 320.)
    caps = [(q - 1) >> bl if e % lv == 0 else (1 << bl) - 1 for e in range(dim * lv)]
    worst = max(sum(caps[(j - h) % n] for h in slots if (j - h) % n < dim * lv) for j in range(n))
    assert worst < q / (4 * t), worst
    key = []
    for i in range(dim):
        for l in range(lv):
            c1 = [int(v) for v in rng.integers(0, q, size=n)]
            err = [0] * n
            err[i * lv + l] = int(rng.integers(-1, 2))
            c0 = [(x + e) % q for x, e in zip(pyref.negacyclic_schoolbook(c1, sk, q), err)]
            c0[0] = (c0[0] + R.pack_gadget(q, lwe_sk[i], l, bl, lv)) % q
            key.append([c0, c1])
    # four messages as LWE ciphertexts without error: b = <a, s> + delta m
    lwe_a = [[int(v) for v in rng.integers(0, q, size=dim)] for _ in msgs]
    lwe_b = [(sum(a * s for a, s in zip(row, lwe_sk)) + delta * m) % q for row, m in zip(lwe_a, msgs)]
    c0, c1 = R.pack_formula_int(q, n, bl, lv, key, lwe_a, lwe_b, slots)
    phase = [(x - y) % q for x, y in zip(c0, pyref.negacyclic_schoolbook(c1, sk, q))]
    want = [0] * n
    for h, m in zip(slots, msgs):
        want[h] = m
    noise = []
    for j in range(n):
        assert (phase[j] * t + q // 2) // q % t == want[j], j
        e = (phase[j] - delta * want[j]) % q
        noise.append(min(e, q - e))
    print("largest noise", max(noise), "bound", q / (4 * t))
    assert 0 < max(noise) <= worst < q / (4 * t)
