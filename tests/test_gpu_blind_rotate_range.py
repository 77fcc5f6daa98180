"""GPU blind rotation and bootstrap over the whole rotation range, with an LWE
modulus of its own, and negacyclic CMux / blind rotation / bootstrap against
a reference that shares nothing with the library.

The other blind-rotation tests pass lwe_q = q and draw the mask below q: near
2^62 the product a * 2N wraps and the rotation amount is 0..4 (0..16 at the
60-bit preset), so the wrap branch of the rotation (a coefficient crossing
X^N), a rotation by exactly 2N, the int32 truncation and a step that only
canonicalises are reached on a handful of coefficients or not at all.  Here
lwe_q is 2^32, 4N, 257 or a 27-bit prime and every mask set is checked, with
``oracle.pyref.rot_amount`` and before the library runs, to contain each kind
of step that applies to its lwe_q (tests/lwe_inputs.py) and to execute at
least half of its steps.

Compat mode is compared with the C oracle given the same lwe_q, on every row
and on every kernel path the environment switches select; negacyclic mode with
``pyref.blind_rotate`` over ``pyref.negacyclic_multiply`` (Python integers
only).  Bit-exact throughout.  Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import lwe_inputs as L
import ntt_primes as P
import oracle
from oracle import pyref

pytestmark = pytest.mark.gpu

P27 = 132120577
P62 = 4611686018326724609
Q60 = 1152921504606584833    # Q_60_1, tfhe-256-secure
Q62 = 4611686018429485057    # 2^62 + 2^21 + 1: the wide family starts here
QG = P.QG
M64 = L.M64
LWE_NAMES = ["2^32", "4N", "257", "P27"]
BR_ENV = ("FHE_BR_PERSIST_MAX", "FHE_BR_PAIR", "FHE_BR_MULTI", "FHE_BR_PAIR_TIMEOUT_US", "FHE_BR_PAIR_COOP")

# k = 1, N = 1024..4096: 2 level workgroups per ciphertext at level 2 / 3
# (k_br_multi; at level 1 the two-CU pair), the pair, one CU (k_br_persist),
# one fused CMux launch per step
PATHS_K1 = {"multi": {}, "pair": {"FHE_BR_MULTI": "0"}, "one": {"FHE_BR_PAIR": "0"},
            "step": {"FHE_BR_PERSIST_MAX": "0"}}
# k = 2..4: the k + 1 accumulators in LDS for the whole loop, or composed steps
PATHS_KN = {"lds": {}, "composed": {"FHE_BR_PERSIST_MAX": "0"}}
# N = 32768 and q >= 2^62: composed steps only
PATHS_COMPOSED = {"composed": {}}


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def rnd(seed, q, *shape):
    return oracle.splitmix_fill(seed, q, int(np.prod(shape))).reshape(shape)


def accumulators(seed, q, b, k, n):
    """Both components non-zero; raw words in the planted ciphertext (row 0),
    in the one whose steps are all skipped (row 1: they come back copied or
    negated) and in the one whose steps only rotate by multiples of 2N (row
    2: they come back reduced)."""
    acc = rnd(seed, q, b, k + 1, n)
    for i in range(min(b, 3)):
        plant_raw(acc[i, (0, k, k)[i]], q)
    return acc


def plant_raw(poly, q):
    """Raw words at both ends: the body's rotation X^s negates (and so
    reduces) coefficient 0 for s in [N, 2N) and coefficient N - 1 for s in
    [1, N], so one end at least stays raw whatever the body (but for s = N)."""
    poly[:3] = poly[-3:] = [M64, q, q + 1]


def run_paths(monkeypatch, be, paths, acc0, lwe_a, lwe_b, bsk_ntt, lwe_q):
    """One blind rotation per path -> ({path: acc}, {path: repairs taken})."""
    got, reps = {}, {}
    for name, env in paths.items():
        for v in BR_ENV:
            monkeypatch.delenv(v, raising=False)
        for var, val in env.items():
            monkeypatch.setenv(var, val)
        before = be.repair_count()
        acc = acc0.copy()
        be.blind_rotate(acc, lwe_a, lwe_b, bsk_ntt, lwe_q=lwe_q)
        got[name] = acc
        reps[name] = be.repair_count() - before
    for v in BR_ENV:
        monkeypatch.delenv(v, raising=False)
    return got, reps


def assert_paths_equal(got, reps, exp):
    """Every path equals the expected rows; the message names the paths and
    rows that do not."""
    bad = {p: [i for i in range(len(exp)) if not (v[i] == exp[i]).all()] for p, v in got.items()}
    assert not any(bad.values()), f"rows differing from the reference per path {bad}, repairs {reps}"


def assert_raw_words_survive(exp, q):
    """The inputs must still test what they are for: in the wholly skipped
    ciphertext (row 1) the reference hands raw words back, and in the one
    whose steps only rotate by multiples of 2N (row 2) it hands none back."""
    assert (np.asarray(exp[1]) >= q).any()
    assert (np.asarray(exp[2]) < q).all()


def oracle_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0):
    t = oracle.NTT(n, q)
    return [t.blind_rotate(k, bl, lv, lwe_a[i], int(lwe_b[i]), lwe_q, bsk, acc0[i]) for i in range(len(acc0))]


# ------------------------------------------------------------ compat mode vs the C oracle
COMPAT = [
    # k = 1 fused: the pair (level 1); six CUs per ciphertext, the pair and the LDS-aliasing one-CU kernel at
    # N = 4096; four CUs per ciphertext; a 32-bit ring
    (1024, P62, 23, 1, 1, PATHS_K1), (4096, Q60, 10, 3, 1, PATHS_K1), (2048, P62, 15, 2, 1, PATHS_K1),
    (1024, P27, 9, 3, 1, PATHS_K1),
    # k = 2..4: LDS kernels and composed steps
    (1024, P62, 15, 2, 2, PATHS_KN), (1024, P62, 15, 2, 3, PATHS_KN), (512, P62, 23, 1, 4, PATHS_KN),
    # the wide family (q >= 2^62)
    (1024, QG, 15, 2, 1, PATHS_COMPOSED), (1024, Q62, 23, 1, 1, PATHS_COMPOSED),
]


@pytest.mark.parametrize("lwe_name", LWE_NAMES)
@pytest.mark.parametrize("n,q,bl,lv,k,paths", COMPAT, ids=lambda v: None if isinstance(v, dict) else str(v))
def test_blind_rotate_full_range_vs_oracle(fg, monkeypatch, n, q, bl, lv, k, paths, lwe_name):
    lwe_q = L.lwe_modulus(lwe_name, n)
    b, dim = 5, 8
    lwe_a, lwe_b = L.masks(700 + n, n, lwe_q, b, dim), L.bodies(701 + n, n, lwe_q, b)
    L.check_coverage(n, lwe_q, lwe_a)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), bl, lv, k)
    bsk = rnd(702 + n + k, q, dim, (k + 1) * lv, k + 1, n)
    acc0 = accumulators(703 + n, q, b, k, n)
    exp = oracle_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0)
    assert_raw_words_survive(exp, q)
    got, reps = run_paths(monkeypatch, be, paths, acc0, lwe_a, lwe_b, be.prepare_ggsw(bsk), lwe_q)
    assert_paths_equal(got, reps, exp)


@pytest.mark.parametrize("lwe_name", LWE_NAMES)
def test_blind_rotate_full_range_two_pass_degree(fg, lwe_name):
    """N = 32768 (composed steps over the two-pass transform), three calls of
    two ciphertexts with two steps each; together they hold every class of
    step and of ciphertext."""
    n, q, bl, lv, k = 32768, P62, 23, 1, 1
    lwe_q = L.lwe_modulus(lwe_name, n)
    p = L.planted(n, lwe_q, 6)
    calls = [np.array([[p[0], p[1]], [0, 0]], np.uint64), np.array([[p[2], p[3]], [p[4], p[5]]], np.uint64),
             np.array([[lwe_q, 0], [0, 2 * lwe_q]], np.uint64)]
    L.check_coverage(n, lwe_q, np.concatenate(calls))
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), bl, lv, k)
    bsk = rnd(711, q, 2, (k + 1) * lv, k + 1, n)
    bsk_ntt = be.prepare_ggsw(bsk)
    for c, lwe_a in enumerate(calls):
        lwe_b = L.bodies(712 + c, n, lwe_q, 2)
        acc0 = accumulators(715 + c, q, 2, k, n)
        acc = acc0.copy()
        be.blind_rotate(acc, lwe_a, lwe_b, bsk_ntt, lwe_q=lwe_q)
        assert_paths_equal({"composed": acc}, {}, oracle_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0))


@pytest.mark.parametrize("lwe_name", LWE_NAMES)
def test_blind_rotate_full_range_repair_pass(fg, monkeypatch, lwe_name):
    """A zero poll budget: every ciphertext that reaches a hand-off is given
    up and recomputed by the repair pass (k_br_persist from the saved input),
    with the call's lwe_q -- all but row 1, whose steps are all skipped."""
    n, q, bl, lv, k, b, dim = 1024, P62, 23, 1, 1, 6, 8
    lwe_q = L.lwe_modulus(lwe_name, n)
    lwe_a, lwe_b = L.masks(720, n, lwe_q, b, dim), L.bodies(721, n, lwe_q, b)
    L.check_coverage(n, lwe_q, lwe_a)
    live = sum(any(r != 0 for r in row) for row in L.amounts(n, lwe_q, lwe_a))
    assert live == b - 1
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), bl, lv, k)
    bsk = rnd(722, q, dim, (k + 1) * lv, k + 1, n)
    acc0 = accumulators(723, q, b, k, n)
    paths = {"repair": {"FHE_BR_PAIR_TIMEOUT_US": "0"}, "pair": {}}
    exp = oracle_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0)
    assert_raw_words_survive(exp, q)
    got, reps = run_paths(monkeypatch, be, paths, acc0, lwe_a, lwe_b, be.prepare_ggsw(bsk), lwe_q)
    assert_paths_equal(got, reps, exp)
    assert reps == {"repair": live, "pair": 0}


@pytest.mark.parametrize("lwe_name", LWE_NAMES)
@pytest.mark.parametrize("n,q,bl,lv", [(1024, P62, 23, 1), (4096, Q60, 10, 3)])
def test_bootstrap_explicit_lwe_modulus_vs_oracle(fg, n, q, bl, lv, lwe_name):
    """fhe_bootstrap_batch hands its lwe_q on to the blind rotation; the test
    polynomial holds raw words, which the wholly skipped ciphertext carries
    into the sample extract."""
    k, b, dim, out_dim = 1, 3, 8, 12
    lwe_q = L.lwe_modulus(lwe_name, n)
    lwe_a, lwe_b = L.masks(730 + n, n, lwe_q, b, dim), L.bodies(731 + n, n, lwe_q, b)
    L.check_coverage(n, lwe_q, lwe_a)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), bl, lv, k)
    o = oracle.NTT(n, q)
    bsk = rnd(732 + n, q, dim, (k + 1) * lv, k + 1, n)
    tp = rnd(733 + n, q, n)
    plant_raw(tp, q)
    ksk_a, ksk_b = rnd(734, q, k * n * lv, out_dim), rnd(735, q, k * n * lv)
    oa, ob = be.bootstrap(lwe_a, lwe_b, be.prepare_ggsw(bsk), tp, ksk_a, ksk_b, bl, lv, lwe_q=lwe_q)
    for i in range(b):
        ea, eb = o.bootstrap(k, bl, lv, lwe_a[i], int(lwe_b[i]), lwe_q, bsk, tp, bl, lv, ksk_a, ksk_b)
        assert (oa[i] == ea).all() and int(ob[i]) == eb, i


@pytest.mark.parametrize("n,q,bl,lv,k", [(1024, P62, 23, 1, 1), (1024, P62, 15, 2, 2)])
def test_graph_replay_follows_lwe_modulus(fg, monkeypatch, n, q, bl, lv, k):
    """Device-resident per-step (k = 1) and composed (k = 2) blind rotations
    on a side stream are captured into the context's graph.  Three calls on
    the same buffers with lwe_q = 2^32, 4N, 2^32: lwe_q is a kernel argument
    frozen at capture, so a cache that ignored it would replay the first
    graph for the second call."""
    import torch

    monkeypatch.setenv("FHE_BR_PERSIST_MAX", "0")
    b, dim = 5, 8
    lwe_qs = [1 << 32, 4 * n, 1 << 32]
    lwe_a, lwe_b = L.masks(740, n, 1 << 32, b, dim), L.bodies(741, n, 1 << 32, b)
    lwe_a[3, :7] = L.planted(n, 4 * n, 7)   # rows 3 and 4 for 4N; under 2^32 all their steps are skipped
    lwe_a[4, :] = L.identity_steps(4 * n, dim)
    lwe_b[0] = 5 * n // 2  # a body that rotates under 4N as well
    for lwe_q in set(lwe_qs):
        L.check_coverage(n, lwe_q, lwe_a)
        assert all(pyref.rot_amount(int(v), n, lwe_q) != L.INT32_MIN for v in lwe_b)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), bl, lv, k)
    bsk = rnd(742, q, dim, (k + 1) * lv, k + 1, n)
    acc0 = accumulators(743, q, b, k, n)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")

    side = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(side):
        bsk_ntt = be.prepare_ggsw(dev(bsk))
        la, lb, init = dev(lwe_a), dev(lwe_b), dev(acc0)
        acc = torch.empty_like(init)
        for lwe_q in lwe_qs:
            acc.copy_(init)
            be.blind_rotate(acc, la, lb, bsk_ntt, lwe_q=lwe_q)
            side.synchronize()
            outs.append(acc.cpu().numpy().view(np.uint64).copy())
    for lwe_q, out in zip(lwe_qs, outs):
        assert_paths_equal({f"lwe_q={lwe_q}": out}, {}, oracle_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0))
    assert (outs[0] == outs[2]).all()
    assert (outs[0] != outs[1]).any()


def test_blind_rotate_explicit_lwe_modulus_multi_device_host(fg):
    """Host arrays on a multi-device context (device 0 twice on a one-GPU
    box): every per-device slice gets the call's lwe_q."""
    import torch

    nd = torch.cuda.device_count()
    devs = [0, 0] if nd < 2 else list(range(min(nd, 4)))
    n, q, bl, lv, k, b, dim, lwe_q = 1024, P62, 23, 1, 1, 5, 8, 1 << 32
    lwe_a, lwe_b = L.masks(750, n, lwe_q, b, dim), L.bodies(751, n, lwe_q, b)
    L.check_coverage(n, lwe_q, lwe_a)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q, devices=devs), bl, lv, k)
    bsk = rnd(752, q, dim, (k + 1) * lv, k + 1, n)
    acc0 = accumulators(753, q, b, k, n)
    acc = acc0.copy()
    be.blind_rotate(acc, lwe_a, lwe_b, be.prepare_ggsw(bsk), lwe_q=lwe_q)
    assert_paths_equal({"host": acc}, {}, oracle_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0))


# ------------------------------------------------------------ negacyclic mode vs Python integers
def ints(a):
    return [[int(v) for v in row] for row in a]


def pyref_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0):
    keys = [[ints(row) for row in g] for g in bsk]
    return [np.array(pyref.blind_rotate(ints(acc0[i]), [int(v) for v in lwe_a[i]], int(lwe_b[i]), lwe_q, keys, q, bl,
                                        lv, k, pyref.negacyclic_multiply), dtype=np.uint64) for i in range(len(acc0))]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n,name", [(256, "lazy_top"), (1024, "u64_top")])
def test_cmux_negacyclic_vs_pyref(fg, n, name, k):
    q = P.sweep_primes(n)[name]
    lv, b = 2, 2
    bl = -(-q.bit_length() // lv)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q, mode="negacyclic"), bl, lv, k)
    ggsw = rnd(760 + n, q, (k + 1) * lv, k + 1, n)
    ct0, ct1 = rnd(761 + n, q, b, k + 1, n), rnd(762 + n, q, b, k + 1, n)
    ct0[0, 0, :3] = ct1[1, k, :3] = [M64, q, q + 1]  # raw words on either side of the difference
    got = be.cmux(be.prepare_ggsw(ggsw), ct0, ct1)
    for i in range(b):
        exp = pyref.cmux([ints(row) for row in ggsw], ints(ct0[i]), ints(ct1[i]), q, bl, lv, k,
                         pyref.negacyclic_multiply)
        assert (got[i] == np.array(exp, dtype=np.uint64)).all(), i


@pytest.mark.parametrize("n,q,bl,lv,k,paths,b", [
    (1024, P27, 9, 3, 1, PATHS_K1, 4), (1024, P27, 9, 3, 2, PATHS_KN, 4),
    (1024, P62, 15, 2, 1, PATHS_K1, 4), (1024, P62, 15, 2, 2, PATHS_KN, 4),
    # 12 products of 4096 coefficients per step: the three planted ciphertexts only
    (4096, Q60, 10, 3, 1, PATHS_K1, 3),
    (1024, QG, 15, 2, 1, PATHS_COMPOSED, 4),
], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_blind_rotate_negacyclic_vs_pyref(fg, monkeypatch, n, q, bl, lv, k, paths, b):
    """Negacyclic blind rotation was so far compared with the library's own
    other kernels only (the C oracle is compat-only)."""
    lwe_q, dim = 1 << 32, 6
    lwe_a, lwe_b = L.masks(770 + n, n, lwe_q, b, dim), L.bodies(771 + n, n, lwe_q, b)
    L.check_coverage(n, lwe_q, lwe_a)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q, mode="negacyclic"), bl, lv, k)
    bsk = rnd(772 + n + k, q, dim, (k + 1) * lv, k + 1, n)
    acc0 = accumulators(773 + n, q, b, k, n)
    exp = pyref_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0)
    assert_raw_words_survive(exp, q)
    got, reps = run_paths(monkeypatch, be, paths, acc0, lwe_a, lwe_b, be.prepare_ggsw(bsk), lwe_q)
    assert_paths_equal(got, reps, exp)


def test_bootstrap_negacyclic_vs_pyref(fg):
    """Blind rotation by pyref; sample extract and key switch use no
    transform, so the oracle's are the same in either mode."""
    n, q, bl, lv, k, b, dim, out_dim, lwe_q = 1024, P62, 23, 1, 1, 3, 6, 12, 1 << 32
    lwe_a, lwe_b = L.masks(780, n, lwe_q, b, dim), L.bodies(781, n, lwe_q, b)
    L.check_coverage(n, lwe_q, lwe_a)
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q, mode="negacyclic"), bl, lv, k)
    bsk = rnd(782, q, dim, (k + 1) * lv, k + 1, n)
    tp = rnd(783, q, n)
    plant_raw(tp, q)
    ksk_a, ksk_b = rnd(784, q, k * n * lv, out_dim), rnd(785, q, k * n * lv)
    oa, ob = be.bootstrap(lwe_a, lwe_b, be.prepare_ggsw(bsk), tp, ksk_a, ksk_b, bl, lv, lwe_q=lwe_q)
    acc0 = np.zeros((b, k + 1, n), np.uint64)
    acc0[:, k] = tp
    for i, acc in enumerate(pyref_rows(n, q, k, bl, lv, lwe_a, lwe_b, lwe_q, bsk, acc0)):
        xa, xb = oracle.sample_extract(q, acc)
        ea, eb = oracle.key_switch(q, bl, lv, ksk_a, ksk_b, xa, xb)
        assert (oa[i] == ea).all() and int(ob[i]) == eb, i
