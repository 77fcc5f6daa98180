"""GPU parity of the one-launch RNS kernels (k_ntt_fwd_limbs, k_ntt_inv_limbs,
k_polymul_limbs, k_polymul2_limbs, k_ew_limbs: grid.y = limb, constants from
a device table) at every degree 4..16384, in each of their three
instantiation families (lazy 32-bit, non-lazy 32-bit, 64-bit;
ntt_primes.limb_families), on the rows that fill the unreduced input windows.

Device-resident calls on a ring whose limbs share word and laziness take
these kernels; host arrays go limb by limb and never reach them, so every
operand here is a device tensor.  The limbs of a ring differ by orders of
magnitude (two neighbours at the lazy bound beside the smallest NTT prime), so
a kernel that read limb 0's constants for another limb fails on every row.
Below N = 4096 a workgroup carries several polynomials and limb y starts at
y * batch * N: the unused slots of limb y's last workgroup address limb
y + 1's first rows, which only the `valid` flag keeps out -- every batch here
leaves such a workgroup, and every word of every limb is compared.

Compat mode bit-exact against the CPU oracle (oracle/ref_cpu.c); negacyclic
mode against the same call on a single PolynomialRing, which
test_gpu_negacyclic.py ties to oracle/pyref.py at these degrees and moduli,
and up to N = 1024 against pyref directly.

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import ntt_primes as P
import oracle
import test_gpu_negacyclic as neg

pytestmark = pytest.mark.gpu

OPS = ("fwd", "inv", "mul", "pw", "add", "sub")


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    neg._CACHE.clear()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)  # (the copy waits for the stream the call ran on)


def limb_rows(n, moduli, batch=None, inverse=False, ppb=1, start=None):
    """[limbs, b, n]: limb i holds base_rows(n, q_i), so a row is of the same
    kind in every limb while its words differ.  batch None: every base row,
    at least ppb + 3 rows, no whole number of workgroups; a number: that many
    rows, cyclically from the row named `start`.  Returns (names per limb,
    rows)."""
    names, limbs = [], []
    for q in moduli:
        nm, base = P.base_rows(n, q, inverse=inverse)
        if batch is None:
            rows = P.tile_rows(base, ppb + 3, ppb)
        else:
            at = nm.index(start if start in nm else "const q-1")
            nm, base = nm[at:] + nm[:at], np.roll(base, -at, axis=0)
            rows = P.tile_rows(base, batch)[:batch]
        names.append(nm)
        limbs.append(rows)
    count = max(r.shape[0] for r in limbs)  # (a wide limb has fewer base rows: repeat them)
    limbs = [r if r.shape[0] == count else P.tile_rows(r, count)[:count] for r in limbs]
    return names, np.ascontiguousarray(np.stack(limbs))


def word_rows(n, moduli, b):
    """Two operands [limbs, b, n] of ntt_primes.stream_words(q_i), cycled
    along the row (and shifted from row to row); the second one word ahead."""
    j = np.arange(n)[None, :] + np.arange(b)[:, None]
    a, c = [], []
    for q in moduli:
        w = np.array(P.stream_words(q), dtype=np.uint64)
        a.append(w[j % w.size])
        c.append(w[(j + 1) % w.size])
    return np.ascontiguousarray(np.stack(a)), np.ascontiguousarray(np.stack(c))


def bad(got, exp, names):
    rows = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0]
    return [(int(i), names[i % len(names)]) for i in rows[:6]]


class Launch:
    """Runs ring calls on device copies of the operands and checks after each
    call that the inputs still hold what was sent."""

    def __init__(self, ring, **operands):
        self.ring, self.h = ring, operands
        self.d = {k: dev(v) for k, v in operands.items()}

    def __call__(self, op, a, b=None):
        r = self.ring
        fn = {"fwd": r.forward_ntt, "inv": r.inverse_ntt, "mul": r.multiply, "pw": r.pointwise_multiply,
              "add": r.add, "sub": r.subtract}[op]
        args = [a] if b is None else [a, b]
        out = host(fn(*[self.d[k] for k in args]))
        for k in args:
            assert (host(self.d[k]) == self.h[k]).all(), (op, k, "input changed")
        return out


def elementwise_expected(q, op, a, b):
    fn = {"pw": oracle.pointwise, "add": oracle.poly_add, "sub": oracle.poly_sub}[op]
    return fn(q, np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()).reshape(a.shape)


def roll_rows(x, k=5):
    return np.ascontiguousarray(np.roll(x, k if x.shape[1] > k else 1, axis=1))


def single_ring(fg, n, q, mode, x, xi, y):
    """The same transform calls on one PolynomialRing (device tensors)."""
    r = fg.PolynomialRing(n, q, mode=mode)
    return {"fwd": host(r.forward_ntt(dev(x))), "inv": host(r.inverse_ntt(dev(xi))),
            "mul": host(r.multiply(dev(x), dev(y)))}


# ------------------------------------------------------------ every op in one launch
@pytest.mark.parametrize("mode", ["compat", "negacyclic"])
@pytest.mark.parametrize("family", P.LIMB_FAMILIES)
@pytest.mark.parametrize("logn", range(2, 15))
def test_every_op_one_launch(fg, monkeypatch, logn, family, mode):
    monkeypatch.delenv("FHE_RNS_ONE_LAUNCH", raising=False)
    n = 1 << logn
    moduli = P.limb_families(n)[family]
    info = fg.PolynomialRing(n, moduli[0]).info
    ppb = info.polys_per_block
    assert info.word_bits == (64 if family == "u64" else 32) and ppb == max(1, 4096 // max(n, 16))
    ring = fg.RNSPolynomialRing(n, moduli, mode=mode)
    names, x = limb_rows(n, moduli, ppb=ppb)
    inames, xi = limb_rows(n, moduli, inverse=True, ppb=ppb)
    b = x.shape[1]
    assert b >= ppb + 3 and (ppb == 1 or b % ppb) and (ppb == 1 or xi.shape[1] % ppb)
    y = roll_rows(x)
    wa, wb = word_rows(n, moduli, b)
    run = Launch(ring, x=x, xi=xi, y=y, wa=wa, wb=wb)
    got = {"fwd": run("fwd", "x"), "inv": run("inv", "xi"), "mul": run("mul", "x", "y")}
    for op in ("pw", "add", "sub"):
        got[op] = run(op, "x", "y")
        got[op + " words"] = run(op, "wa", "wb")

    for i, q in enumerate(moduli):
        if mode == "compat":
            t = oracle.NTT(n, q)
            exp = {"fwd": t.forward(x[i]), "inv": t.inverse(xi[i]), "mul": t.polymul(x[i], y[i])}
        else:
            exp = single_ring(fg, n, q, mode, x[i], xi[i], y[i])
        for op in ("pw", "add", "sub"):
            exp[op] = elementwise_expected(q, op, x[i], y[i])
            exp[op + " words"] = elementwise_expected(q, op, wa[i], wb[i])
        for op, e in exp.items():
            assert (got[op][i] == e).all(), (op, i, q, bad(got[op][i], e, inames[i] if op == "inv" else names[i]))
        if mode == "negacyclic" and n <= 1024:
            top = "const lim-1" if "const lim-1" in names[i] else "const q-1"
            for nm in (top, "mixed one slow word per 16"):
                k = names[i].index(nm)
                assert (got["fwd"][i, k] == neg.ref_forward(q, x[i, k])).all(), ("forward vs pyref", i, q, nm)
                assert (got["mul"][i, k] == neg.ref_mul(q, x[i, k], y[i, k])).all(), ("multiply vs pyref", i, q, nm)


# ------------------------------------------------------------ ragged batches
@pytest.mark.parametrize("n", [4, 64, 1024, 2048, 4096])
def test_ragged_batches(fg, monkeypatch, n):
    """Batches of one, one short of a workgroup, one past it and one past two
    (lazy family): the free slots of limb 0's last workgroup address limb 1's
    rows 0.., so every word of every limb is compared with the oracle."""
    monkeypatch.delenv("FHE_RNS_ONE_LAUNCH", raising=False)
    moduli = P.limb_families(n)["lazy"]
    ppb = fg.PolynomialRing(n, moduli[0]).info.polys_per_block
    assert (ppb == 1) == (n == 4096) and ppb == 4096 // max(n, 16)
    ring = fg.RNSPolynomialRing(n, moduli)
    refs = [oracle.NTT(n, q) for q in moduli]
    batches = sorted({1, ppb + 1, 2 * ppb + 1} | ({ppb - 1} if ppb > 1 else set()))
    for b in batches:
        names, x = limb_rows(n, moduli, batch=b, start="const lim-1")
        inames, xi = limb_rows(n, moduli, batch=b, inverse=True, start="const lim-1")
        assert x.shape == xi.shape == (3, b, n)
        y = roll_rows(x, 1)  # (batch 1: the square of the top-of-window row)
        run = Launch(ring, x=x, xi=xi, y=y)
        fwd, inv, mul = run("fwd", "x"), run("inv", "xi"), run("mul", "x", "y")
        for i, t in enumerate(refs):
            for op, got, exp, nm in (("fwd", fwd[i], t.forward(x[i]), names[i]), ("inv", inv[i], t.inverse(xi[i]), inames[i]),
                                     ("mul", mul[i], t.polymul(x[i], y[i]), names[i])):
                assert (got == exp).all(), (op, b, i, moduli[i], bad(got, exp, nm))


# ------------------------------------------------------------ one launch vs one launch per limb
@pytest.mark.parametrize("family", P.LIMB_FAMILIES)
@pytest.mark.parametrize("n", [256, 8192])
def test_one_launch_equals_per_limb_launches(fg, monkeypatch, n, family):
    moduli = P.limb_families(n)[family]
    ppb = fg.PolynomialRing(n, moduli[0]).info.polys_per_block
    ring = fg.RNSPolynomialRing(n, moduli)
    _, x = limb_rows(n, moduli, ppb=ppb)
    _, xi = limb_rows(n, moduli, inverse=True, ppb=ppb)
    run = Launch(ring, x=x, xi=xi, y=roll_rows(x))
    got = {}
    for one in ("1", "0"):
        monkeypatch.setenv("FHE_RNS_ONE_LAUNCH", one)
        got[one] = {"fwd": run("fwd", "x"), "inv": run("inv", "xi"),
                    **{op: run(op, "x", "y") for op in ("mul", "pw", "add", "sub")}}
    assert tuple(got["1"]) == OPS
    for op in OPS:
        assert (got["1"][op] == got["0"][op]).all(), op
        assert got["1"][op].any(), op


# ------------------------------------------------------------ rings that are not uniform
def mixed_rings(n):
    s, w = P.sweep_primes(n), P.stream_primes(n)
    return {"laziness differs": [s["lazy_top"], s["nonlazy_bottom"]], "word differs": [s["u32_top"], s["u64_bottom"]],
            "one wide limb": [s["u64_top"], w["wide_bottom"]]}


@pytest.mark.parametrize("kind", ["laziness differs", "word differs", "one wide limb"])
def test_mixed_rings_compute_every_limb(fg, monkeypatch, kind):
    """Limbs of different kernel shapes must not share one launch (the `one`
    predicate of fhe_rns_ctx_create) and still compute every limb: device
    tensors, all six ops against the oracle."""
    monkeypatch.delenv("FHE_RNS_ONE_LAUNCH", raising=False)
    n = 1024
    moduli = mixed_rings(n)[kind]
    ppb = fg.PolynomialRing(n, moduli[0]).info.polys_per_block
    ring = fg.RNSPolynomialRing(n, moduli)
    names, x = limb_rows(n, moduli, ppb=ppb)
    inames, xi = limb_rows(n, moduli, inverse=True, ppb=ppb)
    assert x.shape[1] % ppb and xi.shape[1] % ppb
    y = roll_rows(x)
    run = Launch(ring, x=x, xi=xi, y=y)
    got = {"fwd": run("fwd", "x"), "inv": run("inv", "xi"), **{op: run(op, "x", "y") for op in ("mul", "pw", "add", "sub")}}
    for i, q in enumerate(moduli):
        t = oracle.NTT(n, q)
        exp = {"fwd": t.forward(x[i]), "inv": t.inverse(xi[i]), "mul": t.polymul(x[i], y[i])}
        for op in ("pw", "add", "sub"):
            exp[op] = elementwise_expected(q, op, x[i], y[i])
        for op, e in exp.items():
            assert (got[op][i] == e).all(), (op, i, q, bad(got[op][i], e, inames[i] if op == "inv" else names[i]))
