"""CPU-side contract of SIMD batching: the slot codec, the rotation element
and the Galois chain are declared, exported and bound and check their
arguments without a GPU; fhe_simd_rotation_element (host arithmetic) equals
the model; the model of tests/simd_ref.py obeys the laws the header states
(permutation of the odd residues, round trip, rotation, slot-wise product,
slot sum); in exact integers, with real ternary keys and Gaussian errors,
SIMD-encoded ciphertexts multiply slot by slot, rotate under sigma_3 and sum
over their slots -- each with 4 * noise < q / (2 t) asserted first; the Python
surface exists, the typed JS surface declares FHESimdEngine, and the new
kernels use no scratch and spill no VGPR.

The header declares the entry points with 3, 1, 2, 2, 4, 6, 5 and 12 arguments."""
import ctypes as C
import glob
import json
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bfv_ref as B
import fhe_gpu
import galois_ref as G
import simd_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_simd_ctx_create": 3, "fhe_simd_ctx_destroy": 1, "fhe_simd_ctx_get_info": 2,
                "fhe_simd_slot_index": 2, "fhe_simd_rotation_element": 4, "fhe_simd_encode_batch": 6,
                "fhe_simd_decode_batch": 5, "fhe_ct_galois_chain_batch": 12}
P62 = 4611686018326724609
ENGINE_METHODS = ("generateRotationKeys", "encodeSimd", "decodeSimd", "rotateRows", "rotateColumns", "sumSlots",
                  "innerProductScaled")
CONTEXT_METHODS = ("simdEncode", "simdEncodeAsync", "simdDecode", "simdDecodeAsync", "ctGaloisChain", "ctGaloisChainAsync")


def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fhe_gpu.h")).read()
    lib = fhe_gpu.lib()
    bound = {s[0]: s for s in fhe_gpu.SIGNATURES}
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"^(?:int|void)\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name
        assert name in bound, name
        assert len(bound[name][2]) == nargs, name
    assert C.sizeof(fhe_gpu.SimdInfo) == 32
    assert "typedef struct { uint64_t q, t, psi; uint32_t n; int32_t word_bits; } fhe_simd_info;" in hdr
    for text in ("e(s) =\n *   3^i mod 2n for r = 0 and 2n - (3^i mod 2n) for r = 1", "k(s) = (e(s) - 1) / 2",
                 "X[k(s)] = values[s] mod t", "c when c <= (t - 1) / 2,\n *   else q - (t - c)", "out[s] = Y[k(s)]",
                 "assumes a prime t", "g(steps, swap) = 3^(steps mod n/2) (2n - 1)^swap mod 2n",
                 "w[r][i] = v[r xor swap][(i + steps)\n *   mod n/2]", "g_i = 3^(2^i) mod 2n for i < log2(n/2), then g = 2n - 1",
                 "no longer\n *   decodes at n = 256", "fhe_ct_trace_batch keeps coefficients, not SIMD slots",
                 "a packed\n *   comparison bit sits at a coefficient", "must be\n *   destroyed before ctx",
                 "FHE_SIMD_FUSED=0 (read per call) forces the composed path", "steps must be between 1 and 64",
                 "word-identical to that\n *   chain of calls", "gs / key_idx are HOST arrays in both residences"):
        assert text in hdr, text


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = (C.c_uint64 * 2)(0, 0)
    p = C.addressof(word)
    h = C.c_void_p()
    g3 = (C.c_uint32 * 2)(3, 5)
    g_even = (C.c_uint32 * 2)(3, 4)

    def err(rc, code=-9):
        assert rc == code, rc
        return lib.fhe_last_error().decode()

    assert err(lib.fhe_simd_ctx_create(None, 65537, None)) == "null out"
    assert err(lib.fhe_simd_ctx_create(None, 65537, C.byref(h))) == "null context"
    assert h.value is None
    lib.fhe_simd_ctx_destroy(None)  # a no-op
    assert err(lib.fhe_simd_ctx_get_info(None, None)) == "null simd context"
    assert err(lib.fhe_simd_slot_index(None, None)) == "null simd context"
    enc, dec, chain = lib.fhe_simd_encode_batch, lib.fhe_simd_decode_batch, lib.fhe_ct_galois_chain_batch
    # the buffers and the count come before the context
    assert err(enc(None, None, 0, p, 1, dev)) == "null buffer"
    assert err(enc(None, p, 1, None, 1, dev)) == "null buffer"
    assert err(dec(None, None, p, 1, dev)) == "null buffer"
    assert err(dec(None, p, None, 1, dev)) == "null buffer"
    assert err(enc(None, p, 0, p, 0, dev)) == "at least one polynomial is needed"
    assert err(dec(None, p, p, 0, dev)) == "at least one polynomial is needed"
    assert err(enc(None, p, 0, p, 1, dev)) == "null simd context"
    assert err(dec(None, p, p, 1, dev)) == "null simd context"
    # the chain: the step count, the element list and every element's parity come first
    for ns in (0, 65, 1 << 31):
        assert err(chain(None, 4, 2, ns, g3, None, p, p, 0, p, 1, dev)) == "steps must be between 1 and 64", ns
    assert err(chain(None, 4, 2, 2, None, None, p, p, 0, p, 1, dev)) == "null buffer"
    assert err(chain(None, 4, 2, 2, g_even, None, p, p, 0, p, 1, dev)) == "Galois element must be odd"
    assert err(chain(None, 4, 2, 1, g_even, None, p, p, 0, p, 1, dev)) == "null context"  # only gs[0] = 3 is read
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert err(chain(None, 4, 2, 2, g3, None, a[0], a[1], 1, a[2], 1, dev)) == "null buffer", i
    assert err(chain(None, 4, 0, 2, g3, None, None, p, 0, p, 1, dev)) == "null context"  # no key without levels
    assert "at least one ciphertext" in err(chain(None, 4, 2, 2, g3, None, p, p, 0, p, 0, dev))
    for bl, lv in ((0, 2), (64, 1), (32, 3), (22, 4)):
        assert "invalid decomposition" in err(chain(None, bl, lv, 2, g3, None, p, p, 0, p, 1, dev)), (bl, lv)
    assert err(chain(None, 16, 4, 2, g3, g3, p, p, 1, p, 1, dev)) == "null context"


@pytest.mark.parametrize("n", [4, 8, 1024, 65536])
def test_rotation_element_equals_the_model(n):
    half = n // 2
    for steps in (0, 1, -1, half - 1, half, -half - 3, 1 << 40):
        for swap in (False, True):
            g = fhe_gpu.rotation_element(n, steps, swap)
            assert g == S.rotation_element(n, steps, swap), (n, steps, swap)
            assert g % 2 == 1 and 0 < g < 2 * n
    assert fhe_gpu.rotation_element(n, 0) == 1 and fhe_gpu.rotation_element(n, 0, True) == 2 * n - 1
    assert fhe_gpu.rotation_element(n, 1) == 3 % (2 * n)


def test_rotation_element_rejects_bad_degrees():
    lib = fhe_gpu.lib()
    g = C.c_uint32(7)
    for n in (0, 1, 2, 3, 6, 1000, 131072, 65537):
        assert lib.fhe_simd_rotation_element(n, 1, 0, C.byref(g)) == -9, n
    assert lib.fhe_simd_rotation_element(8, 1, 0, None) == -9
    with pytest.raises(fhe_gpu.FHEError):
        fhe_gpu.rotation_element(12, 1)


# ---- the model's laws ------------------------------------------------------
def prime_for(n):
    """The smallest prime t = 1 (mod 2n)."""
    t = 2 * n + 1
    while any(t % d == 0 for d in range(2, int(t ** 0.5) + 1)):
        t += 2 * n
    return t


SIZES = [4, 8, 16, 32, 64]


def test_exponents_are_a_permutation_of_the_odd_residues():
    n = 4
    while n <= 65536:
        e = S.exponents(n)
        assert sorted(e) == list(range(1, 2 * n, 2)), n
        assert sorted(S.slot_index(n)) == list(range(n)), n
        n *= 2
    assert S.exponents(4) == [1, 3, 7, 5] and S.slot_index(8) == [0, 1, 4, 5, 7, 6, 3, 2]


@pytest.mark.parametrize("n", SIZES)
def test_model_round_trip_rotation_product_and_sum(n):
    t = prime_for(n)
    psi = S.find_psi(n, t)
    assert pow(psi, n, t) == t - 1
    rng = random.Random(n)
    v = [rng.randrange(t) for _ in range(n)]
    w = [rng.randrange(t) for _ in range(n)]
    mv, mw = S.encode(v, t, psi), S.encode(w, t, psi)
    assert all(0 <= c < t for c in mv)
    assert S.decode(mv, t, psi) == v
    # raw words are read mod t on both sides
    assert S.encode([x + t * (i % 3) for i, x in enumerate(v)], t, psi) == mv
    assert S.decode([c + t * (i % 5) for i, c in enumerate(mv)], t, psi) == v
    # the centred lift mod q keeps the residue class of the signed value
    q = 7681 if t < 7681 else P62
    for c, l in zip(mv, S.lift(mv, t, q)):
        assert (l if l <= q // 2 else l - q) == (c if c <= (t - 1) // 2 else c - t)
    # rotation law
    half = n // 2
    for steps in (0, 1, -1, half - 1, half + 1, -half - 3):
        for swap in (False, True):
            g = S.rotation_element(n, steps, swap)
            assert S.decode(G.sigma_int(mv, g, t), t, psi) == S.rotate(v, steps, swap), (steps, swap)
    # ring products are slot-wise products, sums slot-wise sums
    assert S.decode(G.negacyclic_schoolbook(mv, mw, t), t, psi) == [a * b % t for a, b in zip(v, w)]
    assert S.decode([(a + b) % t for a, b in zip(mv, mw)], t, psi) == [(a + b) % t for a, b in zip(v, w)]
    # slot sum
    gs = S.slot_sum_elements(n)
    assert len(gs) == n.bit_length() - 1 and gs[-1] == 2 * n - 1
    x = list(mv)
    for i, g in enumerate(gs):
        if i == len(gs) - 1:
            rows = S.decode(x, t, psi)
            assert rows == [sum(v[:half]) % t] * half + [sum(v[half:]) % t] * half
        x = [(a + b) % t for a, b in zip(x, G.sigma_int(x, g, t))]
    assert S.decode(x, t, psi) == [sum(v) % t] * n
    assert x == [sum(v) % t] + [0] * (n - 1)  # the constant polynomial


# ---- meaning, in exact integers, with real keys ---------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_encrypted_inner_product_and_rotation_decode(seed):
    """n = 64, q = P62, t = 257, key-switch base 2^16 x 4: multiply_scaled ->
    relinearize -> slot sum decodes to <v, w> mod t in every slot, and sigma_3
    after the relinearisation to the product rows rotated left by one.
    Margins (q / (2 t)) / noise measured for seeds 1 and 2: above 10^9 after the
    product, about 5 * 10^7 after the slot sum (at t = 65537 the same chain leaves about 400 and 8 - 17)."""
    n, q, t, bl, lv = 64, P62, 257, 16, 4
    psi = S.find_psi(n, t)
    rng = random.Random(20261021 + seed)
    mul = G.negacyclic_schoolbook
    s, pk = B.keygen(rng, n, q)
    v = [rng.randrange(t) for _ in range(n)]
    w = [rng.randrange(t) for _ in range(n)]
    mv, mw = S.encode(v, t, psi), S.encode(w, t, psi)
    ct1, ct2 = B.encrypt(rng, mv, pk, q, t), B.encrypt(rng, mw, pk, q, t)
    assert S.decode(B.decode(B.phase2(ct1, s, q), q, t), t, psi) == v
    ct = B.relinearize(B.multiply_scaled(ct1, ct2, q, t), B.relin_key(rng, s, q, bl, lv), q, bl)
    limit = q / (2 * t)

    def opened(c, want_slots):
        ph = B.phase2(c, s, q)
        noise = B.noise(ph, S.encode(want_slots, t, psi), q, t)
        print("noise", noise, "margin", limit / max(noise, 1))
        assert 4 * noise < limit, (noise, limit)
        return S.decode(B.decode(ph, q, t), t, psi), limit / max(noise, 1)

    prod = [a * b % t for a, b in zip(v, w)]
    got, margin = opened(ct, prod)
    assert got == prod
    keys = []
    for g in S.slot_sum_elements(n):
        masks = [[rng.randrange(q) for _ in range(n)] for _ in range(lv)]
        errs = [B.sample_gauss(rng, n) for _ in range(lv)]
        keys.append(G.switch_key_int(q, bl, g, s, s, masks, errs, mul))
    # sigma_3: both rows one step to the left
    rot = G.ct_galois_int(q, bl, lv, 3, keys[0], ct, False, mul)
    got, _ = opened(rot, S.rotate(prod, 1))
    assert got == S.rotate(prod, 1)
    x = ct
    for g, key in zip(S.slot_sum_elements(n), keys):
        x = G.ct_galois_int(q, bl, lv, g, key, x, True, mul)
    ip = sum(a * b for a, b in zip(v, w)) % t
    got, margin = opened(x, [ip] * n)
    assert got == [ip] * n


# ---- surfaces --------------------------------------------------------------
def test_python_surface_exists():
    for cls, names in ((fhe_gpu.SimdEncoder, ("encode", "decode", "slot_index", "close")),
                       (fhe_gpu.KeyGenerator, ("rotation_keys",)),
                       (fhe_gpu.EncryptionEngine, ("encode_simd", "decode_simd", "decrypt_simd", "galois_chain",
                                                   "rotate_rows", "rotate_columns", "sum_slots", "inner_product_scaled"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    assert isinstance(fhe_gpu.EncryptionEngine.simd, property)
    assert callable(fhe_gpu.rotation_element)
    for n in (4, 64, 8192):
        assert fhe_gpu.slot_sum_elements(n) == S.slot_sum_elements(n)
    # the chain and the rotations refuse keys that are not the rotation set
    ring = type("Ring", (), {"degree": 8})()
    eng = fhe_gpu.EncryptionEngine.__new__(fhe_gpu.EncryptionEngine)
    eng.ring = ring
    one = fhe_gpu.SwitchKey(ring, np.zeros((3, 2, 8), np.uint64), 7, 3, 5)
    trace_keys = fhe_gpu.SwitchKey(ring, np.zeros((3, 3, 2, 8), np.uint64), 7, 3, [9, 5, 3])
    ct = np.zeros((2, 8), np.uint64)
    with pytest.raises(fhe_gpu.FHEError, match="nkeys"):
        eng.galois_chain(ct, [3], one)
    with pytest.raises(fhe_gpu.FHEError, match="same length"):
        eng.galois_chain(ct, [3, 5], trace_keys, [0])
    with pytest.raises(fhe_gpu.FHEError, match="key index"):
        eng.galois_chain(ct, [3], trace_keys, [3])
    for call in (lambda: eng.rotate_rows(ct, 1, trace_keys), lambda: eng.rotate_columns(ct, trace_keys),
                 lambda: eng.sum_slots(ct, trace_keys)):
        with pytest.raises(fhe_gpu.FHEError, match="rotation_keys"):
            call()


def test_typescript_declares_simd_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHESimdEngine extends FHEScaledEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  generateRotationKeys\(sk: SecretKey[^;]*\): Promise<RotationKeys>;", text, re.M)
        assert re.search(r"^  encodeSimd\(values: bigint\[\][^;]*\): Promise<Plaintext>;", text, re.M)
        assert re.search(r"^  decodeSimd\([^;]*\): Promise<bigint\[\]>;", text, re.M)
        assert re.search(r"^  rotateRows\(ct: Ciphertext, steps: number, keys: RotationKeys\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  rotateColumns\(ct: Ciphertext, keys: RotationKeys\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  sumSlots\(ct: Ciphertext, keys: RotationKeys[^;]*\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  innerProductScaled\(ct1: Ciphertext, ct2: Ciphertext, ek: EvaluationKey, keys: RotationKeys\)"
                         r": Promise<Ciphertext>;", text, re.M)
    assert "export interface RotationKeys {" in dts
    # the base interfaces do not gain them
    for name in ("FHEEngine", "FHECompareEngine", "FHEPackEngine", "FHEGaloisEngine", "FHEScaledEngine"):
        base = dts[dts.index("export interface %s " % name):]
        base = base[:base.index("\n}")]
        for meth in ENGINE_METHODS:
            assert meth not in base, (name, meth)
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in CONTEXT_METHODS:
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth


def test_js_prototypes_have_simd_methods():
    if not shutil.which("node"):
        pytest.skip("node not installed")
    if not os.path.exists(os.path.join(PKG, "build", "fhe_napi.node")):
        pytest.skip("N-API addon not built")
    code = ("const m=require(%r);console.log(JSON.stringify({e:Object.getOwnPropertyNames(m.FHEEngineImpl.prototype),"
            "c:Object.getOwnPropertyNames(m.NttContext.prototype)}))" % os.path.join(PKG, "lib", "index.js"))
    out = json.loads(subprocess.run(["node", "-e", code], capture_output=True, text=True, check=True).stdout)
    for meth in ENGINE_METHODS:
        assert meth in out["e"], meth
    for meth in CONTEXT_METHODS:
        assert meth in out["c"], meth


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    # encode: log2(n) = 2 .. 14 at both word sizes; decode: the same, and the lazy form of the 32-bit lanes
    for pat, count in ((r"k_simd_encode<\d+, unsigned (int|long)>", 26),
                       (r"k_simd_decode<\d+, unsigned (int|long), (true|false)>", 39),
                       (r"k_simd_permute\(", 1), (r"k_simd_lift\(", 1)):
        hits = [(n, k) for n, k in zip(names, ks) if re.search(pat, n)]
        assert len(hits) == count, (pat, [n for n, _ in hits])
        for n, k in hits:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])
