"""CPU-side contract of the Galois automorphisms, the ciphertext key switch
and the trace: fhe_poly_galois_batch, fhe_switch_key_generate,
fhe_ct_galois_batch and fhe_ct_trace_batch are declared, exported and bound
and check their arguments without a GPU; the Python methods exist; the typed
JS surface declares FHEGaloisEngine; the new kernels use no scratch and spill
no VGPR; sigma_g composes and inverts as the group (Z / 2n)^*; the formula
equals sigma_g followed by relinearisation; and, in exact integers, a
Galois-switched ciphertext decrypts to sigma_g(m), a re-keyed one decrypts under
the new key in both ring products, a full trace leaves only slot 0 and
isolate_slot only the chosen slot -- each with its worst-case noise asserted
below q / (4 t) first.

The header declares the four entry points with 6, 11, 10 and 9 arguments."""
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
import galois_ref as R
import oracle
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {"fhe_poly_galois_batch": 6, "fhe_switch_key_generate": 11, "fhe_ct_galois_batch": 10,
                "fhe_ct_trace_batch": 9}
ENGINE_METHODS = ("generateSwitchKey", "generateGaloisKeys", "applyGalois", "reKey", "isolateSlot")
CONTEXT_METHODS = ("polyGalois", "switchKeyGenerate", "ctGalois", "ctGaloisAsync", "ctTrace", "ctTraceAsync")
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
    for text in ("out[k] = in[j] mod q when k < n, else out[k - n] = (q - in[j] mod q) % q",
                 "fhe_poly_galois_batch    sigma_g of npoly polynomials", "Galois element must be odd",
                 "Galois element\n *   out of range", "out0 = sigma_g(c0) [+ c0 mod q] + sum_l d_l (*) b_l",
                 "out1 =             [  c1 mod q] + sum_l d_l (*) a_l", "level 0 therefore copies rows 0 and 1",
                 "g_i = n / 2^i + 1", "(2^steps)^-1 mod q", "1 <= steps <= log2(n)",
                 "m[j] = (q - sigma_g(sk_from)[j]) % q", "the NEGATED source key", "fhe_relin_key_prepare (same shape",
                 "only under FHE_MODE_NEGACYCLIC", "For g = 1 (re-keying) the message moves to\n *   sk_to in both modes",
                 "with real keys only under FHE_MODE_NEGACYCLIC"):
        assert text in hdr, text


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = C.c_uint64(0)
    p = C.addressof(word)
    seed = (C.c_uint64 * 4)(1, 2, 3, 4)

    def err(rc, code=-9):
        assert rc == code, rc
        return lib.fhe_last_error().decode()

    pg, sw, cg, tr = (lib.fhe_poly_galois_batch, lib.fhe_switch_key_generate, lib.fhe_ct_galois_batch,
                      lib.fhe_ct_trace_batch)
    # an even Galois element, before anything else is looked at
    for g in (0, 2, 1 << 31):
        assert err(pg(None, g, p, p, 1, dev)) == "Galois element must be odd", g
        assert err(sw(None, p, p, g, 4, 2, seed, 0, 3.2, p, dev)) == "Galois element must be odd", g
        assert err(cg(None, 4, 2, g, p, p, 0, p, 1, dev)) == "Galois element must be odd", g
    # null buffers
    assert err(pg(None, 3, None, p, 1, dev)) == "null buffer"
    assert err(pg(None, 3, p, None, 1, dev)) == "null buffer"
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert err(cg(None, 4, 2, 3, a[0], a[1], 1, a[2], 1, dev)) == "null buffer", i
        assert err(tr(None, 4, 2, 1, a[0], a[1], a[2], 1, dev)) == "null buffer", i
    # no key is needed without levels: the context is reached
    assert err(cg(None, 4, 0, 3, None, p, 0, p, 1, dev)) == "null context"
    assert err(tr(None, 4, 0, 1, None, p, p, 1, dev)) == "null context"
    # nothing to do
    assert "at least one polynomial" in err(pg(None, 3, p, p, 0, dev))
    assert "at least one ciphertext" in err(cg(None, 4, 2, 3, p, p, 0, p, 0, dev))
    assert "at least one ciphertext" in err(tr(None, 4, 2, 1, p, p, p, 0, dev))
    assert "steps must be between 1 and log2(n)" in err(tr(None, 4, 2, 0, p, p, p, 1, dev))
    # the shift limits of relinearisation: 1 <= base_log <= 63, (level - 1) base_log < 64
    for bl, lv in ((0, 2), (64, 1), (32, 3), (22, 4)):
        assert "invalid decomposition" in err(cg(None, bl, lv, 3, p, p, 0, p, 1, dev)), (bl, lv)
        assert "invalid decomposition" in err(tr(None, bl, lv, 1, p, p, p, 1, dev)), (bl, lv)
    # the context is looked at after the arguments.  (g >= 2n, steps > log2(n) and the overlaps are
    # measured against the context's degree: tests/test_gpu_galois.py.)
    assert err(pg(None, 3, p, p, 1, dev)) == "null context"
    assert err(cg(None, 63, 1, 3, p, p, 1, p, 1, dev)) == "null context"
    assert err(cg(None, 32, 2, 0xFFFFFFFF, p, p, 0, p, 1, dev)) == "null context"
    assert err(tr(None, 21, 4, 16, p, p, p, 1, dev)) == "null context"
    assert err(sw(None, p, p, 3, 4, 2, seed, 0, 3.2, p, dev)) == "null context"


def test_python_surface_exists():
    for cls, names in ((fhe_gpu.PolynomialRing, ("galois",)), (fhe_gpu.KeyGenerator, ("switch_key", "galois_keys")),
                       (fhe_gpu.EncryptionEngine, ("apply_galois", "rekey", "trace", "isolate_slot"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    ring = type("Ring", (), {"degree": 4})()  # the constructor only asks for the degree
    k = fhe_gpu.SwitchKey(ring, np.zeros((3, 2, 4), np.uint64), 7, 3, 5)
    assert (k.base_log, k.level, k.g, k.steps) == (7, 3, 5, None) and k.key.shape == (3, 2, 4)
    k = fhe_gpu.SwitchKey(ring, np.zeros((2, 3, 2, 4), np.uint64), 7, 3, [5, 3])
    assert k.steps == 2 and k.g == [5, 3]
    with pytest.raises(fhe_gpu.FHEError):
        fhe_gpu.SwitchKey(ring, np.zeros((3, 2, 4), np.uint64), 7, 2)
    eng = fhe_gpu.EncryptionEngine.__new__(fhe_gpu.EncryptionEngine)
    with pytest.raises(fhe_gpu.FHEError, match="g = 1"):
        eng.rekey(np.zeros((2, 4), np.uint64), fhe_gpu.SwitchKey(ring, np.zeros((3, 2, 4), np.uint64), 7, 3, 5))


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    # k_dmac MODE 4 for log2(n) = 2 .. 14 and both word sizes, as every other mode
    for pat, count in (("k_poly_galois(", 1), (r"k_dmac<\d+, unsigned (int|long), 2, false, 4>", 26)):
        hits = [(n, k) for n, k in zip(names, ks) if re.search(pat if "<" in pat else re.escape(pat), n)]
        assert len(hits) == count, (pat, [n for n, _ in hits])
        for n, k in hits:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k["scratch"], k["vgpr_spill"])
    # the existing modes keep their instantiations
    for mode in range(4):
        assert sum(1 for n in names if re.search(r"k_dmac<\d+, unsigned (int|long), 2, false, %d>" % mode, n)) == 26


def test_typescript_declares_galois_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEGaloisEngine extends FHEPackEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  generateSwitchKey\(skTo: SecretKey, skFrom: SecretKey[^;]*\): Promise<SwitchKey>;", text, re.M)
        assert re.search(r"^  generateGaloisKeys\(sk: SecretKey, steps\?: number[^;]*\): Promise<GaloisKeys>;", text, re.M)
        assert re.search(r"^  applyGalois\(ct: Ciphertext, g: number, key: SwitchKey\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  reKey\(ct: Ciphertext, key: SwitchKey\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  isolateSlot\(ct: Ciphertext, slot: number, keys: GaloisKeys\): Promise<Ciphertext>;", text, re.M)
    for name in ("FHEEngine", "FHECompareEngine", "FHEPackEngine"):
        base = dts[dts.index("export interface %s " % name):]
        base = base[:base.index("\n}")]
        for meth in ENGINE_METHODS:
            assert meth not in base, (name, meth)
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in CONTEXT_METHODS:
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth


def test_js_prototypes_have_galois_methods():
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


def planted(seed, q, count):
    """Full-range u64 words with 0, q and 2^64 - 1 planted."""
    w = [(0x9E3779B97F4A7C15 * (i + seed) * (q | 1) + (seed << 40)) & M64 for i in range(count)]
    for i, v in enumerate((0, q, M64)):
        w[(i * 5 + seed) % count] = v
    return w


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("q", [97, 7681, (1 << 64) - (1 << 32) + 1])
def test_sigma_is_the_group_of_odd_residues(n, q):
    p = planted(n, q, n)
    assert {0, q, M64} <= set(p), "raw words planted"
    red = [x % q for x in p]
    odd = range(1, 2 * n, 2)
    assert R.sigma_int(p, 1, q) == red
    # sigma_{2n-1}: X -> X^-1 keeps coefficient 0 and reverses the rest with a sign
    assert R.sigma_int(p, 2 * n - 1, q) == [red[0]] + [(q - red[n - k]) % q for k in range(1, n)]
    # sigma_{n+1} negates the odd coefficients
    assert R.sigma_int(p, n + 1, q) == [(q - x) % q if j & 1 else x for j, x in enumerate(red)]
    for g in odd:
        s = R.sigma_int(p, g, q)
        assert all(x < q for x in s)
        assert sorted(min(x, q - x) % q for x in s) == sorted(min(x, q - x) % q for x in red), g  # a signed permutation
        assert R.sigma_int(s, pow(g, -1, 2 * n), q) == red, g
        assert R.sigma(np.array(p, dtype=np.uint64), g, q).tolist() == s, g  # the gather of the GPU side
        for h in odd:
            assert R.sigma_int(R.sigma_int(p, h, q), g, q) == R.sigma_int(p, g * h % (2 * n), q), (g, h)
    # a ring automorphism of Z_q[X] / (X^n + 1)
    a, b = planted(n + 1, q, n), planted(n + 2, q, n)
    for g in odd:
        lhs = R.sigma_int(R.negacyclic_schoolbook(a, b, q), g, q)
        assert lhs == R.negacyclic_schoolbook(R.sigma_int(a, g, q), R.sigma_int(b, g, q), q), g


def test_own_schoolbook_agrees_with_the_oracle_products():
    n, q = 16, 7681
    a, b = planted(1, q, n), planted(2, q, n)
    assert R.negacyclic_schoolbook(a, b, q) == pyref.negacyclic_schoolbook([x % q for x in a], [x % q for x in b], q)
    assert R.negacyclic_schoolbook(a, b, q) == pyref.negacyclic_multiply(a, b, q)


@pytest.mark.parametrize("n,q,bl,lv", [(4, 97, 2, 4), (16, 7681, 5, 3), (16, 7681, 4, 0)])
@pytest.mark.parametrize("add_input", [0, 1])
def test_formula_equals_sigma_then_relinearisation(n, q, bl, lv, add_input):
    """ct3 = (sigma(c0) [+ c0], [c1 | 0], sigma(c1)) through the oracle's own
    relinearize (the compat product) and, for the true ring product, through
    digit-by-digit products written out here."""
    key = planted(3, q, max(1, lv) * 2 * n)
    key = [[[x % q for x in key[(l * 2 + p) * n:(l * 2 + p + 1) * n]] for p in range(2)] for l in range(lv)]
    ct = [planted(4, q, n), planted(5, q, n)]
    ref = oracle.NTT(n, q)
    for g in range(1, 2 * n, 2):
        s0, s1 = R.sigma_int(ct[0], g, q), R.sigma_int(ct[1], g, q)
        row0 = [(x + y % q) % q for x, y in zip(s0, ct[0])] if add_input else s0
        row1 = [y % q for y in ct[1]] if add_input else [0] * n
        ct3 = np.array([row0, row1, s1], dtype=np.uint64)
        want = ref.relinearize(bl, lv, ct3, np.array(key, dtype=np.uint64)).tolist()
        assert R.ct_galois_int(q, bl, lv, g, key, ct, add_input, pyref.compat_polymul) == want, g
        mask = (1 << bl) - 1
        for l in range(lv):
            d = [(w >> (l * bl)) & mask for w in s1]
            row0 = [(x + y) % q for x, y in zip(row0, pyref.negacyclic_multiply(d, key[l][1], q))]
            row1 = [(x + y) % q for x, y in zip(row1, pyref.negacyclic_multiply(d, key[l][0], q))]
        got = R.ct_galois_int(q, bl, lv, g, key, ct, add_input, R.negacyclic_schoolbook)
        assert got == [row0, row1], g
        u = lambda x: np.array(x, dtype=np.uint64)
        mul = lambda a, b: u([R.negacyclic_schoolbook(x.tolist(), y.tolist(), q) for x, y in zip(a, b)])
        vec = R.ct_galois(q, bl, lv, g, u(key).reshape(lv, 2, n), u(ct)[None], add_input, mul)
        assert vec.tolist() == [got], g


# ---- meaning, in exact integers -------------------------------------------
N, Q, T = 16, 7681, 4
DELTA = Q // T
PRODUCTS = {"negacyclic": R.negacyclic_schoolbook, "compat": pyref.compat_polymul}


def digit_caps(bl, lv):
    """The largest digit of a canonical word at each level."""
    return [min((1 << bl) - 1, (Q - 1) >> (l * bl)) for l in range(lv)]


def switch_noise_bound(bl, lv, errs):
    """|d_l (*) e_l| <= max(d_l) * ||e_l||_1 coefficient-wise, for the ring
    product and, with errors on coefficient 0 only (constants multiply as scalars
    there too), for the compat product.  It is at most the
    level * n * (2^base_log - 1) * max|e| of dense errors."""
    assert bl * lv >= (Q - 1).bit_length()  # the digits recompose every canonical word
    b = sum(c * sum(abs(int(v)) for v in e) for c, e in zip(digit_caps(bl, lv), errs))
    assert b <= lv * N * ((1 << bl) - 1) * max(abs(int(v)) for e in errs for v in e)
    return b


def make_key(rng, bl, lv, g, sk_to, sk_from, mul, constant_errors=False):
    """fhe_switch_key_generate's formula over uniform masks and one error of
    +-1 per level (at coefficient 0 with constant_errors, else anywhere)."""
    masks = [[int(v) for v in rng.integers(0, Q, size=N)] for _ in range(lv)]
    errs = []
    for _ in range(lv):
        e = [0] * N
        e[0 if constant_errors else int(rng.integers(0, N))] = int(rng.choice([-1, 1]))
        errs.append(e)
    return R.switch_key_int(Q, bl, g, sk_to, sk_from, masks, errs, mul), errs


def encrypt(rng, msgs, sk, mul):
    c1 = [int(v) for v in rng.integers(0, Q, size=N)]
    e = [int(v) for v in rng.integers(-1, 2, size=N)]
    c0 = [(x + DELTA * m + err) % Q for x, m, err in zip(mul(c1, [s % Q for s in sk], Q), msgs, e)]
    return [c0, c1]


def open_ct(ct, sk, mul, want, bound):
    """Decodes and returns the largest distance of the phase from DELTA * want."""
    phase = [(x - y) % Q for x, y in zip(ct[0], mul(ct[1], [s % Q for s in sk], Q))]
    assert [(p * T + Q // 2) // Q % T for p in phase] == want
    noise = max(min((p - DELTA * w) % Q, (DELTA * w - p) % Q) for p, w in zip(phase, want))
    print("largest noise", noise, "bound", bound, "q / (4 t)", Q / (4 * T))
    assert noise <= bound
    return noise


def secret(rng):
    s = [int(v) for v in rng.integers(-1, 2, size=N)]
    assert -1 in s and 1 in s
    return s


@pytest.mark.parametrize("g", [3, N + 1, 2 * N - 1, 5 ** 7 % (2 * N)])
def test_galois_switched_ciphertext_decrypts_to_sigma_of_the_message(g):
    bl, lv = 4, 4
    rng = np.random.default_rng([20261021, g])
    mul = PRODUCTS["negacyclic"]
    sk = secret(rng)
    key, errs = make_key(rng, bl, lv, g, sk, sk, mul)
    # key-switch noise + the input error (1) + the offset q - DELTA t of a negated message (1)
    bound = switch_noise_bound(bl, lv, errs) + 1 + (Q - DELTA * T)
    assert bound < Q / (4 * T), bound
    msgs = [int(v) for v in rng.integers(0, T, size=N)]
    out = R.ct_galois_int(Q, bl, lv, g, key, encrypt(rng, msgs, sk, mul), 0, mul)
    assert open_ct(out, sk, mul, R.sigma_int(msgs, g, T), bound) > 0


def rekey_case(product, constant_errors, seed):
    bl, lv = 4, 4
    rng = np.random.default_rng([20261021, seed])
    mul = PRODUCTS[product]
    sk_from, sk_to = secret(rng), secret(rng)
    assert sk_from != sk_to
    key, errs = make_key(rng, bl, lv, 1, sk_to, sk_from, mul, constant_errors=constant_errors)
    bound = switch_noise_bound(bl, lv, errs) + 1
    assert bound < Q / (4 * T), bound
    msgs = [int(v) for v in rng.integers(0, T, size=N)]
    ct = encrypt(rng, msgs, sk_from, mul)
    open_ct(ct, sk_from, mul, msgs, 1)
    out = R.ct_galois_int(Q, bl, lv, 1, key, ct, 0, mul)
    return out, sk_from, sk_to, msgs, bound, mul


@pytest.mark.parametrize("product,constant_errors", [("negacyclic", False), ("negacyclic", True), ("compat", True)])
def test_rekeyed_ciphertext_decrypts_under_the_new_key(product, constant_errors):
    """The true ring product with errors anywhere; the compat product with the
    errors on coefficient 0 (the algebra alone: constants multiply as scalars)."""
    out, sk_from, sk_to, msgs, bound, mul = rekey_case(product, constant_errors, 1)
    open_ct(out, sk_to, mul, msgs, bound)
    phase = [(x - y) % Q for x, y in zip(out[0], mul(out[1], [s % Q for s in sk_from], Q))]
    assert [(p * T + Q // 2) // Q % T for p in phase] != msgs  # and no longer under the old one


def test_compat_product_does_not_keep_rekeying_noise_small():
    """What the header says about g = 1 in compat mode: with key errors off
    coefficient 0 the noise d_l (*) e_l is not bounded by max(d) ||e||_1 under
    the compat product, and the re-keyed ciphertext does not decrypt."""
    failures = 0
    for seed in range(2, 10):
        out, _, sk_to, msgs, bound, mul = rekey_case("compat", False, seed)
        phase = [(x - y) % Q for x, y in zip(out[0], mul(out[1], [s % Q for s in sk_to], Q))]
        noise = max(min((p - DELTA * m) % Q, (DELTA * m - p) % Q) for p, m in zip(phase, msgs))
        failures += noise > bound
    assert failures == 8


def trace_setup(rng, bl, lv, steps):
    mul = PRODUCTS["negacyclic"]
    sk = secret(rng)
    keys, step_bounds = [], []
    for g in R.trace_elements(N, steps):
        key, errs = make_key(rng, bl, lv, g, sk, sk, mul)
        keys.append(key)
        step_bounds.append(switch_noise_bound(bl, lv, errs))
    # x + sigma(x) at most doubles what is there: step i's noise is scaled by 2^(steps - 1 - i);
    # the surviving coefficients keep the input error (1) exactly
    bound = sum(b << (steps - 1 - i) for i, b in enumerate(step_bounds)) + 1
    assert bound < Q / (4 * T), bound
    return mul, sk, keys, bound


def test_full_trace_leaves_only_slot_zero():
    bl, lv, steps = 3, 5, 4  # base_log 4 (levels 15, 15, 15, 1) would give 15 * 46 + 1 > q / (4 t)
    rng = np.random.default_rng(20261022)
    mul, sk, keys, bound = trace_setup(rng, bl, lv, steps)
    msgs = [3] + [int(v) for v in rng.integers(1, T, size=N - 1)]
    ct = encrypt(rng, msgs, sk, mul)
    out = R.trace_int(Q, bl, lv, steps, keys, ct, mul)
    assert open_ct(out, sk, mul, [3] + [0] * (N - 1), bound) > 0
    # slot 0 comes back exactly: message and input noise
    before = (ct[0][0] - mul(ct[1], [s % Q for s in sk], Q)[0]) % Q
    after = (out[0][0] - mul(out[1], [s % Q for s in sk], Q)[0]) % Q
    d = (after - before) % Q
    assert min(d, Q - d) <= bound - 1


def test_partial_trace_keeps_every_fourth_slot():
    bl, lv, steps = 3, 5, 2
    rng = np.random.default_rng(20261023)
    mul, sk, keys, bound = trace_setup(rng, bl, lv, steps)
    msgs = [int(v) for v in rng.integers(1, T, size=N)]
    out = R.trace_int(Q, bl, lv, steps, keys, encrypt(rng, msgs, sk, mul), mul)
    open_ct(out, sk, mul, [m if j % 4 == 0 else 0 for j, m in enumerate(msgs)], bound)


@pytest.mark.parametrize("slot", [0, 1, 7, N - 1])
def test_isolate_slot_leaves_only_the_chosen_slot(slot):
    bl, lv, steps = 3, 5, 4
    rng = np.random.default_rng([20261024, slot])
    mul, sk, keys, bound = trace_setup(rng, bl, lv, steps)
    msgs = [int(v) for v in rng.integers(1, T, size=N)]
    ct = encrypt(rng, msgs, sk, mul)
    x = [pyref.rotate(row, -slot, Q) for row in ct]
    y = R.trace_int(Q, bl, lv, steps, keys, x, mul)
    out = [pyref.rotate(row, slot, Q) for row in y]
    open_ct(out, sk, mul, [m if j == slot else 0 for j, m in enumerate(msgs)], bound)
