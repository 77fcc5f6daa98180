"""GPU parity of the non-transform TFHE kernels at the edges of their word
arithmetic: key switch (csrc/lwe.hip k_key_switch_a / k_key_switch_b /
k_ks_acc<1|4|16> / k_ks_sum and the dispatch of launch_key_switch), decompose
(elementwise.hip k_decompose), sample extract and monomial rotation (lwe.hip
k_sample_extract / k_rotate) and LWE decryption (keygen.hip k_lwe_decrypt).

The key switch takes any modulus q >= 2.  Above 2^63 the reference's running
update r = (r + q - term) % q wraps at 2^64 and the result is no longer
-sum(terms): the ladder of lwe_edges.KS_MODULI sits on both sides of that edge
and of 2^62, with keys and masks that make the wrap certain (counted by
oracle.pyref.key_switch in test_lwe_edges.py).  Every dispatch case names its
path through lwe_edges.ks_plan, which test_lwe_edges.py holds to the shapes
used here.  Bit-exact against the C oracle; decompose against the Python
restatement as well.  Host arrays and device tensors.

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import lwe_edges as E
import lwe_inputs as L
import ntt_primes as P
import oracle
from oracle import pyref

pytestmark = pytest.mark.gpu

INVALID_ARG = -9
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def D(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def H(t):
    import torch

    if isinstance(t, np.ndarray):
        return t
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def I(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


# ---------------------------------------------------------------- key switch
def oracle_key_switch(q, bl, lv, ka, kb, la, lb):
    rows = [oracle.key_switch(q, bl, lv, ka, kb, la[i], int(lb[i])) for i in range(la.shape[0])]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.uint64)


def check_key_switch(fg, q, bl, lv, ka, kb, la, lb, where, puts=(np.ascontiguousarray, D)):
    ea, eb = oracle_key_switch(q, bl, lv, ka, kb, la, lb)
    for put in puts:
        oa, ob = fg.BootstrapEngine.key_switch(q, bl, lv, put(ka), put(kb), put(la), put(lb))
        oa, ob = H(oa), H(ob)
        bad = np.argwhere(oa != ea)
        assert bad.size == 0, (where, put.__name__, "mask", bad[:4].tolist(), len(bad))
        bad = np.argwhere(ob != eb)
        assert bad.size == 0, (where, put.__name__, "body", bad[:4].tolist(), len(bad))
    return ea, eb


@pytest.mark.parametrize("qname", list(E.KS_MODULI))
@pytest.mark.parametrize("keys", E.KEY_KINDS)
def test_key_switch_modulus_ladder(fg, qname, keys):
    """in_dim 25 x level 4 (base 2^7), out_dim 5, 17 ciphertexts: every mask
    kind against every key kind at every modulus of the ladder.  With the
    column of ones the reference wraps in mask and body at every q > 2^63."""
    q = E.KS_MODULI[qname]
    S = E.LADDER
    ka, kb = E.ks_keys(keys, q, S["in_dim"] * S["level"], S["out_dim"])
    kinds, la = E.ks_masks(q, S["in_dim"], S["batch"])
    lb = E.ks_bodies(q, S["batch"])
    ea, eb = check_key_switch(fg, q, S["base_log"], S["level"], ka, kb, la, lb, (qname, keys))
    zero = kinds.index("zero")
    assert not ea[zero].any() and int(eb[zero]) == int(lb[zero])


@pytest.mark.parametrize("q", [E.P62, E.Q_TOP])
@pytest.mark.parametrize("bl,lv", E.KS_DECOMPS)
def test_key_switch_decompositions(fg, q, bl, lv):
    """One digit of one bit up to 64 levels, the top digit at shift 63
    ((21, 4)), and digits past 32 bits, which take the generic kernel at a
    fast modulus too."""
    S = E.DECOMP_CASE
    assert E.ks_plan(q, bl, lv, S["in_dim"], S["out_dim"], S["batch"])["path"] == (
        "acc" if q == E.P62 and bl <= 32 else "generic")
    _, la = E.ks_masks(q, S["in_dim"], S["batch"])
    lb = E.ks_bodies(q, S["batch"], roll=3)
    for keys in ("raw", "ones"):
        ka, kb = E.ks_keys(keys, q, S["in_dim"] * lv, S["out_dim"])
        check_key_switch(fg, q, bl, lv, ka, kb, la, lb, (q, bl, lv, keys))


def raw_key_switch(fg, q, bl, lv, in_dim, out_dim, ka, kb, la, lb, oa, ob, batch):
    """The C entry point on host arrays (None: a null pointer)."""
    def ptr(a):
        return None if a is None else a.ctypes.data

    return fg.lib().fhe_key_switch_batch(q, bl, lv, in_dim, out_dim, ptr(ka), ptr(kb), ptr(la), ptr(lb), ptr(oa),
                                         ptr(ob), batch, fg.FHE_HOST, 0, None)


@pytest.mark.parametrize("bl,lv,in_dim", [(0, 1, 3), (64, 1, 3), (32, 3, 3), (16, 5, 3), (63, 3, 3), (1, 65, 3),
                                          (4, 2, 1 << 31), (1, 64, 1 << 26)])
def test_key_switch_rejections(fg, bl, lv, in_dim):
    """base_log 0 or 64, (level - 1) base_log >= 64 and in_dim level >= 2^32
    are FHE_ERR_INVALID_ARG, and the outputs are not written."""
    q, out_dim, b = E.P62, 2, 2
    small = 3 * 65  # words the call could read with the small in_dim (never with the huge one: rejected first)
    ka = np.ones((small, out_dim), dtype=np.uint64)
    kb = np.ones(small, dtype=np.uint64)
    la = np.ones((b, 3), dtype=np.uint64)
    lb = np.ones(b, dtype=np.uint64)
    oa = np.full((b, out_dim), SENTINEL, dtype=np.uint64)
    ob = np.full(b, SENTINEL, dtype=np.uint64)
    assert raw_key_switch(fg, q, bl, lv, in_dim, out_dim, ka, kb, la, lb, oa, ob, b) == INVALID_ARG
    assert (oa == SENTINEL).all() and (ob == SENTINEL).all()


def test_key_switch_accepts_the_last_valid_decompositions(fg):
    """Next to the rejected ones: (level - 1) base_log = 63, 0, 63 and 62."""
    q = E.P62
    for bl, lv in ((21, 4), (63, 1), (63, 2), (1, 64), (31, 3)):
        ka, kb = E.ks_keys("raw", q, 3 * lv, 2)
        _, la = E.ks_masks(q, 3, 2)
        check_key_switch(fg, q, bl, lv, ka, kb, la, E.ks_bodies(q, 2), (bl, lv))


@pytest.mark.parametrize("q", [E.P27, E.P62])
@pytest.mark.parametrize("case", list(E.ACC_CASES))
def test_key_switch_deferred_dispatch(fg, q, case):
    """The deferred-reduction kernel: 1, 4 and 16 ciphertexts per workgroup
    with full and ragged last tiles, one and two output workgroups, ragged
    entry splits through k_ks_sum and the single split's negated write, a
    split of two LDS rounds, and the high word of the 96-bit sum counting
    every entry."""
    in_dim, lv, bl, out_dim, batches = E.ACC_CASES[case]
    kind = "max" if case == "carries" else "raw"
    ka, kb = E.ks_keys(kind, q, in_dim * lv, out_dim)
    for b in batches:
        plan = E.ks_plan(q, bl, lv, in_dim, out_dim, b)
        assert plan["path"] == "acc" and E.ACC_EXPECT[case](plan), (case, b, plan)
        if case == "carries":
            la = np.full((b, in_dim), E.M64, dtype=np.uint64)
            la[1::2, in_dim // 2:] = 0  # every other ciphertext stops counting half way
        else:
            _, la = E.ks_masks(q, in_dim, b)
        ea, _ = check_key_switch(fg, q, bl, lv, ka, kb, la, E.ks_bodies(q, b, roll=b), (case, b))
        assert ea.any()
    if case == "carries":  # (2^32 - 1)(2^64 - 1) = 2^64 - 2^32 + 1 mod 2^64, entries times: the high word is entries - 1
        assert (in_dim * lv * ((1 << 64) - (1 << 32) + 1)) >> 64 == in_dim * lv - 1


@pytest.mark.parametrize("q", [E.P62, E.Q_TOP])
def test_key_switch_launch_chunk_boundary(fg, q):
    """65535 * 16 + 17 ciphertexts: a second launch of one full tile and one
    ciphertext.  61 distinct ciphertexts tiled; every row compared."""
    S = E.CHUNK_CASE
    bl, lv, in_dim, out_dim, batch, distinct = (S[x] for x in ("base_log", "level", "in_dim", "out_dim", "batch",
                                                              "distinct"))
    assert E.ks_plan(q, bl, lv, in_dim, out_dim, batch)["launches"] == 2
    ka, kb = E.ks_keys("ones", q, in_dim * lv, out_dim)
    rng = np.random.default_rng([61, q % (1 << 32)])
    la = rng.integers(0, 127, size=(distinct, in_dim), dtype=np.uint64, endpoint=True)
    la[0] = 0
    lb = E.ks_bodies(q, distinct)
    ea, eb = oracle_key_switch(q, bl, lv, ka, kb, la, lb)
    assert len({tuple(r) for r in ea.tolist()}) > distinct // 2
    idx = np.arange(batch) % distinct
    oa, ob = fg.BootstrapEngine.key_switch(q, bl, lv, ka, kb, np.ascontiguousarray(la[idx]),
                                           np.ascontiguousarray(lb[idx]))
    bad = np.argwhere(oa != ea[idx])
    assert bad.size == 0, (bad[:4].tolist(), len(bad))
    bad = np.argwhere(ob != eb[idx])
    assert bad.size == 0, (bad[:4].tolist(), len(bad))


@pytest.mark.parametrize("q", [E.P27, 1 << 32, E.Q_TOP])
def test_key_switch_empty_shapes(fg, q):
    """No input coefficient: a zero mask and the raw body, raw even when it
    is not below q.  No output coefficient: the body only."""
    bl, lv, b = 7, 4, 5
    lb = np.array([0, q - 1, q, q + 1 if q + 1 <= E.M64 else q, E.M64], dtype=np.uint64)
    oa = np.full((b, 3), SENTINEL, dtype=np.uint64)
    ob = np.full(b, SENTINEL, dtype=np.uint64)
    assert raw_key_switch(fg, q, bl, lv, 0, 3, None, None, None, lb, oa, ob, b) == 0, fg.lib().fhe_last_error()
    assert not oa.any() and (ob == lb).all()
    in_dim = 6
    ka, kb = E.ks_keys("ones", q, in_dim * lv, 0)
    _, la = E.ks_masks(q, in_dim, b)
    ob[:] = SENTINEL
    assert raw_key_switch(fg, q, bl, lv, in_dim, 0, None, kb, la, lb, None, ob, b) == 0, fg.lib().fhe_last_error()
    _, eb = oracle_key_switch(q, bl, lv, ka, kb, la, lb)
    assert (ob == eb).all(), (I(ob), I(eb))


# ---------------------------------------------------------------- bootstrap
BOOT = {"n": 512, "k": 1, "dim": 8, "b": 3, "bl": 16, "lv": 4, "ks_bl": 7, "ks_lv": 2, "out_dim": 8, "lwe_q": 1 << 32}


def bootstrap_inputs(q):
    S = BOOT
    n, k, dim, b, lv = S["n"], S["k"], S["dim"], S["b"], S["lv"]
    bsk = oracle.splitmix_fill(901, q, dim * (k + 1) * lv * (k + 1) * n).reshape(dim, (k + 1) * lv, k + 1, n)
    tp = oracle.splitmix_fill(902, q, n)
    lwe_a, lwe_b = L.masks(903, n, S["lwe_q"], b, dim), L.bodies(904, n, S["lwe_q"], b)
    ksk_a, ksk_b = E.ks_keys("ones", q, k * n * S["ks_lv"], S["out_dim"])
    return bsk, tp, lwe_a, lwe_b, ksk_a, ksk_b


def test_bootstrap_at_the_top_of_the_word(fg):
    """fhe_bootstrap_batch at the last NTT prime of the word (n = 512, k = 1,
    LWE dimension 8, 3 ciphertexts) against the oracle.  In this (compat)
    mode the reference's inverse transform is identically zero above 2^63
    (its signed mod_inverse returns N^-1 = 0 and zero inverse twiddles), so
    the rotated accumulator's mask is zero: the key switch behind it meets no
    digit and hands the extracted body on raw.  The oracle says so and the
    test asserts it; the key switch that wraps inside a bootstrap is the
    negacyclic test below."""
    S = BOOT
    n, k = S["n"], S["k"]
    q = P.stream_primes(n)["u64_max"]
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), S["bl"], S["lv"], k)
    o = oracle.NTT(n, q)
    assert o.inv_n == 0
    bsk, tp, lwe_a, lwe_b, ksk_a, ksk_b = bootstrap_inputs(q)
    oa, ob = be.bootstrap(lwe_a, lwe_b, be.prepare_ggsw(bsk), tp, ksk_a, ksk_b, S["ks_bl"], S["ks_lv"],
                          lwe_q=S["lwe_q"])
    bodies = set()
    for i in range(S["b"]):
        ea, eb = o.bootstrap(k, S["bl"], S["lv"], lwe_a[i], int(lwe_b[i]), S["lwe_q"], bsk, tp, S["ks_bl"], S["ks_lv"],
                             ksk_a, ksk_b)
        assert (oa[i] == ea).all() and int(ob[i]) == eb, i
        assert not ea.any()
        bodies.add(eb)
    assert len(bodies) > 1


def test_bootstrap_negacyclic_at_the_top_of_the_word(fg):
    """The same bootstrap over the true ring product, where the accumulator's
    mask is not zero: blind rotation by the Python restatement, sample
    extract and key switch by the oracle (no transform in either).  The
    key-switching key holds the column of ones, so the key switch inside the
    bootstrap runs the generic kernels at q > 2^63 and its running update
    wraps in mask and body (counted here by pyref.key_switch)."""
    S = BOOT
    n, k, b = S["n"], S["k"], S["b"]
    q = P.stream_primes(n)["u64_max"]
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q, mode="negacyclic"), S["bl"], S["lv"], k)
    bsk, tp, lwe_a, lwe_b, ksk_a, ksk_b = bootstrap_inputs(q)
    oa, ob = be.bootstrap(lwe_a, lwe_b, be.prepare_ggsw(bsk), tp, ksk_a, ksk_b, S["ks_bl"], S["ks_lv"],
                          lwe_q=S["lwe_q"])
    keys = [[[I(p) for p in row] for row in g] for g in bsk]
    wraps = [0, 0]
    for i in range(b):
        acc = pyref.blind_rotate([[0] * n] * k + [I(tp)], I(lwe_a[i]), int(lwe_b[i]), S["lwe_q"], keys, q, S["bl"],
                                 S["lv"], k, pyref.negacyclic_multiply)
        xa, xb = oracle.sample_extract(q, np.array(acc, dtype=np.uint64))
        ea, eb = oracle.key_switch(q, S["ks_bl"], S["ks_lv"], ksk_a, ksk_b, xa, xb)
        assert (oa[i] == ea).all() and int(ob[i]) == eb, i
        pa, pb, mw, bw = pyref.key_switch(ksk_a, ksk_b, xa, xb, q, S["ks_bl"], S["ks_lv"], skip_first_body=True)
        assert pa == I(ea) and pb == eb
        wraps = [wraps[0] + mw, wraps[1] + bw]
    assert wraps[0] >= 1 and wraps[1] >= 1, wraps


# ---------------------------------------------------------------- decompose
@pytest.mark.parametrize("qname", list(E.ctx_moduli(16)))
def test_decompose_edge_digits(fg, qname):
    """n = 16: every edge digit at every level, among zero bits and among
    one bits, and stream_words(q), against the oracle and the Python
    restatement.  At q = 97 a negative digit of base_log 15 and up wraps
    before it is reduced."""
    n = 16
    q = E.ctx_moduli(n)[qname]
    ring = fg.PolynomialRing(n, q)
    for bl, lv in E.DECOMPS:
        rows = E.decompose_rows(q, n, bl, lv)
        exp = np.stack([oracle.decompose(q, r, bl, lv) for r in rows])
        assert [[I(x) for x in e] for e in exp] == [pyref.decompose(I(r), q, bl, lv) for r in rows]
        for put in (np.ascontiguousarray, D):
            got = H(fg.decompose_polynomial(ring, put(rows), bl, lv))
            bad = np.argwhere(got != exp)
            assert bad.size == 0, (qname, bl, lv, put.__name__, bad[:4].tolist())


@pytest.mark.parametrize("bl,lv", [(0, 1), (4, 0), (1, 65), (33, 2), (16, 5), (64, 1)])
def test_decompose_rejections(fg, bl, lv):
    n, q = 16, 97
    ring = fg.PolynomialRing(n, q)
    x = np.ones((2, n), dtype=np.uint64)
    out = np.full((2, max(lv, 1), n), SENTINEL, dtype=np.uint64)
    rc = fg.lib().fhe_decompose_batch(ring._h, bl, lv, x.ctypes.data, out.ctypes.data, 2, fg.FHE_HOST)
    assert rc == INVALID_ARG
    assert (out == SENTINEL).all()


# ---------------------------------------------------------------- sample extract / rotate
def check_extract(fg, be, q, k, g, where):
    exp = [oracle.sample_extract(q, g[c]) for c in range(g.shape[0])]
    ea = np.stack([e[0] for e in exp])
    eb = np.array([e[1] for e in exp], dtype=np.uint64)
    assert (eb == g[:, k, 0]).all()  # the body comes back raw
    for put in (np.ascontiguousarray, D):
        a, b = be.sample_extract(put(g))
        assert (H(a) == ea).all() and (H(b) == eb).all(), (where, put.__name__)


def check_rotate(fg, be, q, g, rots, where):
    exp = np.stack([np.stack([oracle.rotate(q, p, int(r)) for p in g[c]]) for c, r in enumerate(rots)])
    for put in (np.ascontiguousarray, D):
        got = H(be.multiply_glwe_by_monomial(put(g), rots))
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (where, put.__name__, bad[:4].tolist())


@pytest.mark.parametrize("n", [16, 1024])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_sample_extract_and_rotate_edges(fg, n, k):
    """GLWE dimension 1..3, stream_words(q) at mask indices 0, 1, n - 1 and
    body index 0, every rotation of lwe_edges.rotations against every
    ciphertext."""
    rots = E.rotations(n)
    for qname, q in P.stream_primes(n).items():
        be = fg.BootstrapEngine(fg.PolynomialRing(n, q), 4, 3, k)
        W = P.stream_words(q)
        g = E.planted_glwe(q, n, k, len(W))
        check_extract(fg, be, q, k, g, (qname, n, k))
        tiled = np.ascontiguousarray(np.repeat(g, len(rots), axis=0))
        check_rotate(fg, be, q, tiled, np.array(rots * len(W), dtype=np.int32), (qname, n, k))


@pytest.mark.parametrize("qname", ["u64_top", "u64_max"])
def test_sample_extract_and_rotate_past_the_grid_cap(fg, qname):
    """600 ciphertexts of k = 2, n = 1024: more than 2^20 words, so the
    grid-stride loop behind the 4096-workgroup cap runs twice."""
    n, k, b = 1024, 2, 600
    assert b * k * n > 1 << 20
    q = P.stream_primes(n)[qname]
    be = fg.BootstrapEngine(fg.PolynomialRing(n, q), 4, 3, k)
    g = E.planted_glwe(q, n, k, b)
    check_extract(fg, be, q, k, g, qname)
    rots = E.rotations(n)
    check_rotate(fg, be, q, g, np.array([rots[c % len(rots)] for c in range(b)], dtype=np.int32), qname)


# ---------------------------------------------------------------- LWE decryption
@pytest.mark.parametrize("qname", list(E.KS_MODULI))
def test_lwe_decrypt_edges(fg, qname):
    """Every ladder modulus, plaintext moduli up to 2^64 - 1, dimensions
    around the wavefront, keys with INT64_MIN / INT64_MAX, and bodies that
    put the phase on 0, 1, q - 1 and on both sides of the rounding steps,
    reduced and as b + q."""
    q = E.KS_MODULI[qname]
    for t in E.plaintext_moduli(q):
        for dim in E.LWE_DIMS:
            sk, a, b, want = E.lwe_cases(q, t, dim)
            exp = [oracle.lwe_decrypt(q, t, sk, a[i], int(b[i])) for i in range(len(want))]
            assert [e[1] for e in exp] == want
            assert [e[0] for e in exp] == [E.rounded(p, q, t) % (t or 4) for p in want]
            for put in (np.ascontiguousarray, D):
                if put is D and (t, dim) not in ((0, 65), (E.M64, 742)):
                    continue  # device tensors at two corners; the arithmetic is the same kernel
                vals, ph = fg.lwe_decrypt(q, t, D(sk) if put is D else sk, put(a), put(b))
                assert I(H(ph)) == want, (qname, t, dim, put.__name__)
                assert I(H(vals)) == [e[0] for e in exp], (qname, t, dim, put.__name__)
