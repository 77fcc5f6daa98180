"""CPU-side contract of the scale-invariant BFV product: the entry points are
declared, exported and bound and check their arguments without a GPU; the
Python, TypeScript and JS surfaces exist; the two new kernels use no scratch;
the exact-integer model (tests/bfv_ref.py) agrees with itself -- schoolbook
against Kronecker, the three-channel formula of bfv_scale.hip against the direct
rounding on random and edge values -- and, with real ternary keys and Gaussian
errors, the scaled product decodes to m1 m2 mod (X^n + 1, t) where the
reference's unscaled tensor does not.

Argument counts of the prototypes in include/fhe_gpu.h: create (ctx, t, out),
get_info (sc, info), the lift (sc, in, out_p1, out_p2, npoly, where), the lift
of ct - ref (sc, ct, ref, ref_count, out_p1, out_p2, batch, where), scale-round
(sc, xq, xp1, xp2, out, npoly, where), multiply (sc, ct1, ct2, out, batch,
where), dot (sc, a, b, count, groups, out, where), square (sc, ct, ref,
ref_count, out, batch, where)."""
import ctypes as C
import glob
import json
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

import bfv_ref as R
import fhe_gpu
from ntt_primes import prime_below

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "node-fhe-accelerate_amd")
ENTRY_POINTS = {
    "fhe_scale_ctx_create": 3, "fhe_scale_ctx_get_info": 2, "fhe_poly_center_lift_batch": 6,
    "fhe_ct_center_lift_batch": 8, "fhe_poly_scale_round_batch": 7, "fhe_ct_multiply_scaled_batch": 6,
    "fhe_ct_dot_scaled_batch": 7, "fhe_ct_square_scaled_batch": 7,
}
ENGINE_METHODS = ("multiplyScaled", "dotProductScaled", "squareScaled")
CONTEXT_METHODS = ("ctMultiplyScaled", "ctMultiplyScaledAsync", "ctDotScaled", "ctDotScaledAsync", "ctSquareScaled",
                   "ctSquareScaledAsync")
P27 = 132120577
P62 = 4611686018326724609
QG = (1 << 64) - (1 << 32) + 1


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
    assert re.search(r"^void fhe_scale_ctx_destroy\(fhe_scale_ctx \*sc\);", hdr, re.M)
    assert hasattr(lib, "fhe_scale_ctx_destroy") and "fhe_scale_ctx_destroy" in bound
    assert "typedef struct { uint64_t q, t, aux[2]; uint32_t n, naux; uint64_t max_count; } fhe_scale_info;" in hdr
    assert C.sizeof(fhe_gpu.ScaleInfo) == 48
    # the contract is in the header
    for text in ("out word = rnd(t X) mod q, canonical in [0, q)", "rescales ONCE, after summing", "NOT word-identical",
                 "c0 - c1 s + c2 s^2", "SUBTRACTS c2 s^2", "relinearise first", "FHE_MODE_NEGACYCLIC only",
                 "t count n q < aux[0] aux[1]", "FHE_SCALE_CHUNK=", "must be destroyed before ctx"):
        assert text in hdr, text
    # the auxiliary primes of the model are the library's: NTT-friendly for every degree, below 2^62
    src = open(os.path.join(PKG, "csrc", "fhe_gpu.cpp")).read()
    for p in R.AUX_PRIMES:
        assert "%dull" % p in src and p < 1 << 62 and p % (1 << 17) == 1, p
    assert len(set(R.AUX_PRIMES)) == 3 and R.aux_for(P62) == (R.AUX_PRIMES[1], R.AUX_PRIMES[2])


def test_argument_checks_answer_without_a_gpu():
    lib = fhe_gpu.lib()
    dev = fhe_gpu.FHE_DEVICE
    word = (C.c_uint64 * 2)()
    p = C.addressof(word)

    def err(rc, code=-9):
        assert rc == code, rc
        return lib.fhe_last_error().decode()

    h = C.c_void_p()
    assert err(lib.fhe_scale_ctx_create(None, 4, None)) == "null out"
    assert err(lib.fhe_scale_ctx_create(None, 4, C.byref(h))) == "null context"
    info = fhe_gpu.ScaleInfo()
    assert err(lib.fhe_scale_ctx_get_info(None, C.byref(info))) == "null scale context"
    lib.fhe_scale_ctx_destroy(None)
    mul, dot, sq = lib.fhe_ct_multiply_scaled_batch, lib.fhe_ct_dot_scaled_batch, lib.fhe_ct_square_scaled_batch
    lift, lift_ct, rnd = lib.fhe_poly_center_lift_batch, lib.fhe_ct_center_lift_batch, lib.fhe_poly_scale_round_batch
    # null pointers and zero counts come before the context
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert err(mul(None, a[0], a[1], a[2], 1, dev)) == "null buffer", i
        assert err(dot(None, a[0], a[1], 1, 1, a[2], dev)) == "null buffer", i
        assert err(lift(None, a[0], a[1], a[2], 1, dev)) == "null buffer", i
    for i in range(4):
        a = [p, p, p, p]
        a[i] = None
        assert err(rnd(None, a[0], a[1], a[2], a[3], 1, dev)) == "null buffer", i
    assert err(sq(None, None, None, 0, p, 1, dev)) == "null buffer"
    assert err(sq(None, p, None, 0, None, 1, dev)) == "null buffer"
    assert "at least one ciphertext pair" in err(mul(None, p, p, p, 0, dev))
    assert err(dot(None, p, p, 0, 1, p, dev)) == "Cannot tally empty ballot list"
    assert "at least one group" in err(dot(None, p, p, 1, 0, p, dev))
    assert "at least one ciphertext" in err(sq(None, p, None, 0, p, 0, dev))
    assert "at least one polynomial" in err(lift(None, p, p, p, 0, dev))
    assert "at least one polynomial" in err(rnd(None, p, p, p, p, 0, dev))
    # ref and ref_count as fhe_ct_square_batch
    assert "given together" in err(sq(None, p, p, 0, p, 2, dev))
    assert "given together" in err(sq(None, p, None, 1, p, 2, dev))
    assert "0, 1 or the batch size" in err(sq(None, p, p, 3, p, 2, dev))
    assert "0, 1 or the batch size" in err(lift_ct(None, p, p, 3, p, p, 2, dev))
    # then the context
    for rc in (mul(None, p, p, p, 1, dev), dot(None, p, p, 1, 1, p, dev), sq(None, p, p, 1, p, 2, dev),
               lift(None, p, p, p, 1, dev), rnd(None, p, p, p, p, 1, dev)):
        assert err(rc) == "null scale context"


def test_python_surface_exists():
    for name in ("multiply", "dot", "square", "squared_difference", "center_lift", "scale_round"):
        assert callable(getattr(fhe_gpu.ScaledMultiplier, name)), name
    for name in ("multiply_scaled", "dot_scaled", "square_scaled", "squared_difference_scaled",
                 "tally_weighted_votes_scaled", "multiply_relin_scaled"):
        assert callable(getattr(fhe_gpu.EncryptionEngine, name)), name


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    if not glob.glob(os.path.join(kr.OBJ_DIR, "*.o")):
        pytest.skip("objects not built (run __graft_entry__.build())")
    ks = kr.kernels()
    names = kr.demangle([k["name"] for k in ks])
    for pat, count in (("k_center_lift(", 1), ("k_scale_round<", 2)):  # two primes and the single-prime form
        hits = [(n, k) for n, k in zip(names, ks) if pat in n]
        assert len(hits) == count, (pat, [n for n, _ in hits])
        for n, k in hits:
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (n, k)


def test_typescript_declares_scaled_engine():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    body = dts[dts.index("export interface FHEScaledEngine extends FHEGaloisEngine {"):]
    body = body[:body.index("\n}")]
    impl = dts[dts.index("export declare class FHEEngineImpl implements FHETallyEngine {"):]
    impl = impl[:impl.index("\n}")]
    for text in (body, impl):
        assert re.search(r"^  multiplyScaled\(ct1: Ciphertext, ct2: Ciphertext\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  dotProductScaled\(cts1: Ciphertext\[\], cts2: Ciphertext\[\][^;]*\): Promise<Ciphertext>;", text, re.M)
        assert re.search(r"^  squareScaled\(ct: Ciphertext\): Promise<Ciphertext>;", text, re.M)
    assert "options?: TallyWeightedOptions" in body
    opts = dts[dts.index("export interface TallyWeightedOptions {"):]
    assert re.search(r"^  scaled\?: boolean;", opts[:opts.index("\n}")], re.M)
    for name in ("FHEEngine", "FHEGaloisEngine"):
        base = dts[dts.index("export interface %s " % name):]
        base = base[:base.index("\n}")]
        for meth in ENGINE_METHODS:
            assert meth not in base, (name, meth)
    ctx = dts[dts.index("export declare class NttContext {"):]
    ctx = ctx[:ctx.index("\n}")]
    for meth in CONTEXT_METHODS:
        assert re.search(r"^  %s\(" % meth, ctx, re.M), meth


def test_js_prototypes_have_scaled_methods():
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


# ---------------------------------------------------------------- the model agrees with itself
def test_schoolbook_equals_kronecker():
    rng = random.Random(256)
    for n, bits in ((256, 62), (256, 3), (512, 27)):
        a = [rng.randrange(-(1 << bits), 1 << bits) for _ in range(n)]
        b = [rng.randrange(-(1 << bits), 1 << bits) for _ in range(n)]
        a[0], a[-1], b[0], b[-1] = (1 << bits) - 1, -(1 << bits) + 1, -(1 << bits) + 1, -(1 << bits) + 1
        assert R.negacyclic_kron(a, b) == R.negacyclic(a, b), (n, bits)
    z = [0] * 256
    assert R.negacyclic_kron(z, z) == z
    x = [0] * 256
    x[255] = -1
    assert R.negacyclic_kron(x, x) == [0] * 254 + [-1, 0]  # X^510 = -X^254


@pytest.mark.parametrize("n,q", [(4, 97), (1024, P27), (1024, P62), (256, QG), (32768, P27)])
def test_three_channel_formula_equals_direct_rounding(n, q):
    p1, p2 = R.aux_for(q)
    assert q not in (p1, p2)
    for t in [t for t in (2, 4, 65537) if t < q] + [R.max_t(n, q, p1, p2)]:
        assert 1 <= R.max_count(n, q, t, p1, p2)
        assert R.max_count(n, q, t + 1, p1, p2) == 0 or t < R.max_t(n, q, p1, p2) or t == q - 1
        xs = R.edge_values(q, t, p1, p2, count=200, seed=n)
        bound = (p1 * p2 - 1) // 2
        ys = [R.rnd(t * x, q) for x in xs]
        # the edge list holds what it promises
        assert {0, 1, -1} <= set(xs) and bound in ys and -bound in ys and min(ys) < 0
        assert {(q - 1) // 2, (q + 1) // 2} <= {t * x % q for x in xs}
        for x, y in zip(xs, ys):
            assert abs(t * x - q * y) <= (q - 1) // 2  # nearest integer
            assert R.three_channel(x % q, x % p1, x % p2, q, t, p1, p2) == y % q, (t, x)


def test_lift_and_rnd():
    for q in (97, P27, QG):
        h = (q - 1) // 2
        assert [R.lift(x, q) for x in (0, 1, h, h + 1, q - 1, q, q + h + 1, (1 << 64) - 1)] == \
            [0, 1, h, -h, -1, 0, -h, ((1 << 64) - 1) % q - (q if ((1 << 64) - 1) % q > h else 0)]
        assert [R.rnd(y, q) for y in (0, h, h + 1, -h, -h - 1, q, 3 * q + h, 3 * q + h + 1)] == [0, 0, 1, 0, -1, 1, 3, 4]


# ---------------------------------------------------------------- meaning in exact integers
def _messages(rng, n, t, count):
    return [[rng.randrange(t) for _ in range(n)] for _ in range(count)]


MEANING = [
    # n, q, t, pairs, relinearisation (base_log, level) or None
    (1024, prime_below((1 << 62) - 1, 1024), 65537, 1, None),
    (256, P27, 4, 7, None),
    (1024, P27, 2, 1, None),
    # the parameter sets of tests/test_gpu_scaled.py, relinearisation noise included
    (1024, P62, 65537, 1, (16, 4)),
    (256, P27, 4, 1, (7, 4)),
    (256, P27, 4, 7, (7, 4)),
]


@pytest.mark.parametrize("n,q,t,pairs,relin", MEANING)
def test_scaled_product_decodes_where_the_unscaled_tensor_does_not(n, q, t, pairs, relin):
    rng = random.Random(n * 1000003 + t + pairs)
    s, pk = R.keygen(rng, n, q)
    m1, m2 = _messages(rng, n, t, pairs), _messages(rng, n, t, pairs)
    if pairs > 1:  # a weighted tally: constant weights
        m2 = [[w[0] or 1] + [0] * (n - 1) for w in m2]
    c1 = [R.encrypt(rng, m, pk, q, t) for m in m1]
    c2 = [R.encrypt(rng, m, pk, q, t) for m in m2]
    assert R.decode(R.phase2(c1[0], s, q), q, t) == m1[0]
    want = [0] * n
    for a, b in zip(m1, m2):
        want = [(x + y) % t for x, y in zip(want, R.plain_product(a, b, t))]
    ct3 = R.dot_scaled(c1, c2, q, t)
    phase = R.phase3(ct3, s, q)
    assert R.decode(phase, q, t) == want
    noise, bound = R.noise(phase, want, q, t), q / (2 * t)
    print("n", n, "q", q, "t", t, "pairs", pairs, "noise %.3g bound %.3g margin %.1fx" % (noise, bound, bound / noise))
    assert 4 * noise < bound
    if relin:
        bl, lv = relin
        ct2 = R.relinearize(ct3, R.relin_key(rng, s, q, bl, lv), q, bl)
        phase = R.phase2(ct2, s, q)
        assert R.decode(phase, q, t) == want
        noise = R.noise(phase, want, q, t)
        print("  after relinearisation %d x 2^%d: noise %.3g margin %.1fx" % (lv, bl, noise, bound / noise))
        assert 4 * noise < bound
    # the reference's multiply: the tensor mod q, no rescale, carries Delta^2 m
    X = [[0] * n for _ in range(3)]
    for a, b in zip(c1, c2):
        X = [[(u + v) % q for u, v in zip(r, x)] for r, x in zip(X, R.tensor(a, b, q))]
    assert R.decode(R.phase3(X, s, q), q, t) != want
