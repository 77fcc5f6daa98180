"""CPU-side contract of the hoisted rotations and the plaintext linear
transform: fhe_ct_hoist_batch, fhe_ct_hoisted_galois_batch and
fhe_ct_hoisted_linear_batch are declared, exported and bound (Python, N-API,
TypeScript) and check their arguments without a GPU; pi_g of tests/hoist_ref.py
is a permutation and is the action of sigma_g on the spectrum X_k =
a(psi^(2k+1)); in exact integers, with real ternary keys and Gaussian errors,
hoisted rotations decrypt to the rotated slot vectors and a 32 x 32 matrix
applied through its 32 diagonals decrypts to M v mod t in every slot, with the
noise under the bound derived here; the new kernels use no scratch.

The header declares the entry points with 7, 10 and 12 arguments."""
import ctypes as C
import glob
import os
import random
import re
import sys

import numpy as np
import pytest

import bfv_ref as B
import fhe_gpu
import galois_ref as G
import hoist_ref as Hr
import simd_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_ct_hoist_batch": 7, "fhe_ct_hoisted_galois_batch": 10, "fhe_ct_hoisted_linear_batch": 12}
P62 = 4611686018326724609
CONTEXT_METHODS = ("ctHoist", "ctHoistAsync", "ctHoistedGalois", "ctHoistedGaloisAsync", "ctHoistedLinear",
                   "ctHoistedLinearAsync")
ENGINE_METHODS = ("hoist", "rotateMany", "linearTransform", "generateRotationKeysFor")


def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fhe_gpu.h")).read()
    lib = fhe_gpu.lib()
    bound = {s[0]: s for s in fhe_gpu.SIGNATURES}
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"^int\s+%s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name
        assert name in bound, name
        assert len(bound[name][2]) == nargs, name
    for text in ("pi_g(k) = (((2k+1) g mod 2n) - 1) / 2 = g k + (g - 1) / 2", "row 0     = the words of fhe_ntt_fwd_batch(c0)",
                 "d_l = ((c1 mod q) >> l*base_log) & (2^base_log - 1)", "not of sigma_g(c1)",
                 "out0 = sigma_g(c0) + sum_l sigma_g(d_l) (*) b_l", "out1 =               sum_l sigma_g(d_l) (*) a_l",
                 "add_input = 0) exactly", "they DIFFER from fhe_ct_galois_batch",
                 "level n (2^base_log - 1) max|e|", "accumulate != 0 reads out as one more degree-1 term",
                 "fhe_polymul_batch\n *   of both components with fhe_ntt_inv_batch(p_r), fhe_ct_sum_batch",
                 "answers FHE_ERR_UNSUPPORTED", "FHE_HOIST_FUSED=0 (read per call)", "rotations must be\n *   between 1 and 4096",
                 "terms must be between 1 and\n *   4096", "key index out of range"):
        assert text in hdr, text


def test_python_napi_and_typescript_surfaces():
    for cls, names in ((fhe_gpu.EncryptionEngine, ("hoist", "rotate_many", "linear_transform", "matvec", "prepare_plain")),
                       (fhe_gpu.KeyGenerator, ("rotation_keys_for",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    ring = type("Ring", (), {"degree": 8})()
    h = fhe_gpu.HoistedCiphertext(ring, np.zeros((3, 4, 8), np.uint64), 7, 3)
    assert (h.base_log, h.level, h.buf.shape) == (7, 3, (3, 4, 8))
    with pytest.raises(fhe_gpu.FHEError, match="1 \\+ level"):
        fhe_gpu.HoistedCiphertext(ring, np.zeros((3, 3, 8), np.uint64), 7, 3)
    # a step without its key is refused before any call into the library
    eng = fhe_gpu.EncryptionEngine.__new__(fhe_gpu.EncryptionEngine)
    eng.ring = ring
    keys = fhe_gpu.SwitchKey(ring, np.zeros((2, 3, 2, 8), np.uint64), 7, 3, [3, 9])
    with pytest.raises(fhe_gpu.FHEError, match="no key for rotation step"):
        eng.rotate_many(h, [1, 3], keys)
    with pytest.raises(fhe_gpu.FHEError, match="base_log, level"):
        eng.rotate_many(fhe_gpu.HoistedCiphertext(ring, np.zeros((1, 3, 8), np.uint64), 7, 2), [1], keys)
    with pytest.raises(fhe_gpu.FHEError, match="power of two dividing"):
        eng.matvec(h, np.zeros((3, 3), np.int64), keys)
    napi = open(os.path.join(PKG, "napi", "fhe_napi.c")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, napi), name
    for meth in CONTEXT_METHODS:
        if not meth.endswith("Async"):  # the M() table registers NAME and NAME "Async"
            assert 'M("%s",' % meth in napi, meth
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in CONTEXT_METHODS:
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    js = open(os.path.join(PKG, "lib", "engine.js")).read()
    for meth in ENGINE_METHODS:
        assert re.search(r"^  %s\(" % meth, impl, re.M), meth
        assert re.search(r"^    async %s\(" % meth, js, re.M), meth


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = (C.c_uint64 * 2)(0, 0)
    p = C.addressof(word)
    g3 = (C.c_uint32 * 2)(3, 5)
    g_even = (C.c_uint32 * 2)(3, 4)

    def err(rc, code=-9):
        assert rc == code, rc
        return lib.fhe_last_error().decode()

    hoist, gal, lin = lib.fhe_ct_hoist_batch, lib.fhe_ct_hoisted_galois_batch, lib.fhe_ct_hoisted_linear_batch
    # hoist: buffers, count and decomposition before the context
    assert err(hoist(None, 16, 4, None, p, 1, dev)) == "null buffer"
    assert err(hoist(None, 16, 4, p, None, 1, dev)) == "null buffer"
    assert "at least one ciphertext" in err(hoist(None, 16, 4, p, p, 0, dev))
    for bl, lv in ((0, 2), (64, 1), (32, 3), (22, 4)):
        assert "invalid decomposition" in err(hoist(None, bl, lv, p, p, 1, dev)), (bl, lv)
    assert "at least one decomposition level" in err(hoist(None, 16, 0, p, p, 1, dev))
    assert err(hoist(None, 16, 4, p, p, 1, dev)) == "null context"
    # the applications: the count, the element list and every element's parity come first
    for n in (0, 4097, 1 << 31):
        assert err(gal(None, 4, n, g3, None, p, p, p, 1, dev)) == "rotations must be between 1 and 4096", n
        assert err(lin(None, 4, n, g3, None, p, p, p, 0, p, 1, dev)) == "terms must be between 1 and 4096", n
    assert err(gal(None, 4, 2, None, None, p, p, p, 1, dev)) == "null buffer"
    assert err(gal(None, 4, 2, g_even, None, p, p, p, 1, dev)) == "Galois element must be odd"
    assert err(lin(None, 4, 2, g_even, None, p, p, p, 0, p, 1, dev)) == "Galois element must be odd"
    assert err(gal(None, 4, 1, g_even, None, p, p, p, 1, dev)) == "null context"  # only gs[0] = 3 is read
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert err(gal(None, 4, 2, g3, None, a[0], a[1], a[2], 1, dev)) == "null buffer", i
    for i in range(4):
        a = [p, p, p, p]
        a[i] = None
        assert err(lin(None, 4, 2, g3, None, a[0], a[1], a[2], 1, a[3], 1, dev)) == "null buffer", i
    assert "at least one ciphertext" in err(gal(None, 4, 2, g3, None, p, p, p, 0, dev))
    assert "at least one ciphertext" in err(lin(None, 4, 2, g3, None, p, p, p, 0, p, 0, dev))
    assert "invalid decomposition" in err(gal(None, 0, 2, g3, None, p, p, p, 1, dev))
    assert err(gal(None, 4, 2, g3, g3, p, p, p, 1, dev)) == "null context"
    assert err(lin(None, 4, 2, g3, g3, p, p, p, 1, p, 1, dev)) == "null context"


# ---- pi_g ------------------------------------------------------------------
def prime_for(n):
    """The smallest prime t = 1 (mod 2n)."""
    t = 2 * n + 1
    while any(t % d == 0 for d in range(2, int(t ** 0.5) + 1)):
        t += 2 * n
    return t


@pytest.mark.parametrize("n", [8, 64, 256])
def test_pi_is_a_permutation_and_the_spectrum_action_of_sigma(n):
    t = prime_for(n)
    psi = S.find_psi(n, t)
    rng = random.Random(n)
    a = [rng.randrange(t) for _ in range(n)]
    roots = [pow(psi, 2 * k + 1, t) for k in range(n)]
    X = [S.horner(a, r, t) for r in roots]  # X_k = a(psi^(2k+1)), natural order
    for g in (3, n + 1, 2 * n - 1, pow(3, 5, 2 * n)):
        perm = [Hr.pi(n, g, k) for k in range(n)]
        assert sorted(perm) == list(range(n)), g
        assert perm == [(g * k + (g - 1) // 2) % n for k in range(n)], g  # the affine form the kernels compute
        sa = G.sigma_int(a, g, t)
        assert [S.horner(sa, r, t) for r in roots] == [X[j] for j in perm], g
    assert [Hr.pi(n, 1, k) for k in range(n)] == list(range(n))


# ---- meaning, in exact integers, with real keys ---------------------------
def test_hoisted_rotations_and_matvec_decrypt():
    """n = 64, q = P62, t = 257, key-switch base 2^16 x 4.  Bound, derived: a
    fresh ciphertext carries |e1 + e u + e2 s| <= E (2 n + 1) with E = max|e|;
    one hoisted key switch adds sum_l sigma_g(d_l) (*) e_l, at most level n
    (2^16 - 1) E; a plaintext product multiplies the noise by at most n (t / 2)
    (lifted coefficients are at most t / 2) and a sum over `terms` diagonals
    adds up: terms n (t / 2) (fresh + level n (2^16 - 1) E), about 1.2 10^14
    against q / (2 t) of about 9 10^15."""
    n, q, t, bl, lv, D = 64, P62, 257, 16, 4, 32
    half = n // 2
    psi = S.find_psi(n, t)
    rng = random.Random(20261021)
    mul = G.negacyclic_schoolbook
    s, pk = B.keygen(rng, n, q)
    vec = [rng.randrange(t) for _ in range(D)]
    v = [vec[(sl % half) % D] for sl in range(n)]  # period D along both rows
    ct = B.encrypt(rng, S.encode(v, t, psi), pk, q, t)
    limit = q // (2 * t)
    emax = 0
    keys = {}
    for st in range(1, D):
        g = S.rotation_element(n, st)
        masks = [[rng.randrange(q) for _ in range(n)] for _ in range(lv)]
        errs = [B.sample_gauss(rng, n) for _ in range(lv)]
        emax = max(emax, max(abs(int(e)) for row in errs for e in row))
        keys[st] = (g, G.switch_key_int(q, bl, g, s, s, masks, errs, mul))

    def opened(c, want_slots, bound):
        ph = B.phase2(c, s, q)
        noise = B.noise(ph, S.encode(want_slots, t, psi), q, t)
        print("noise", noise, "bound", bound, "limit", limit)
        assert noise <= bound < limit, (noise, bound, limit)
        return S.decode(B.decode(ph, q, t), t, psi)

    fresh = B.noise(B.phase2(ct, s, q), S.encode(v, t, psi), q, t)
    switch = lv * n * ((1 << bl) - 1) * emax
    # rotations: the hoisted digits are sigma_g of the digits of c1, not the digits of sigma_g(c1)
    for st in (1, 5, D - 1):
        g, key = keys[st]
        rot = Hr.hoisted_galois_int(q, bl, lv, g, key, ct, mul)
        assert opened(rot, S.rotate(v, st), fresh + switch + t) == S.rotate(v, st), st
        assert rot != G.ct_galois_int(q, bl, lv, g, key, ct, False, mul)
    # g = 1: the words of the unhoisted key switch
    masks = [[rng.randrange(q) for _ in range(n)] for _ in range(lv)]
    errs = [B.sample_gauss(rng, n) for _ in range(lv)]
    k1 = G.switch_key_int(q, bl, 1, s, s, masks, errs, mul)
    assert Hr.hoisted_galois_int(q, bl, lv, 1, k1, ct, mul) == G.ct_galois_int(q, bl, lv, 1, k1, ct, False, mul)
    # matvec: all 32 diagonals; diagonal 0 enters as a plaintext product, without a key switch
    M = [[rng.randrange(t) for _ in range(D)] for _ in range(D)]
    want = [sum(M[i][j] * vec[j] for j in range(D)) % t for i in range(D)]
    pts = []
    for j in range(D):
        diag = [M[i][(i + j) % D] for i in range(D)]
        pts.append(S.lift(S.encode([diag[(sl % half) % D] for sl in range(n)], t, psi), t, q))
    acc = [mul(row, pts[0], q) for row in ct]
    steps = list(range(1, D))
    out = Hr.hoisted_linear_int(q, bl, lv, [keys[st][0] for st in steps], [keys[st][1] for st in steps],
                                [pts[st] for st in steps], ct, mul, acc)
    bound = D * n * (t // 2) * (fresh + switch + t)
    got = opened(out, [want[(sl % half) % D] for sl in range(n)], bound)
    assert got == [want[(sl % half) % D] for sl in range(n)]


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    # log2(n) = 2 .. 14 at both word sizes; the hoist also in the lazy form of the 32-bit lanes
    for pat, count in ((r"k_hoist_fwd<\d+, unsigned (int|long), (true|false)>", 39),
                       (r"k_hoist_apply<\d+, unsigned (int|long), (true|false)>", 52),
                       (r"k_hoist_mac<(true|false)>", 2), (r"k_hoist_digits\(", 1), (r"k_hoist_table\(", 1)):
        hits = [(n, k) for n, k in zip(names, ks) if re.search(pat, n)]
        assert len(hits) == count, (pat, [n for n, _ in hits])
        for n, k in hits:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])
