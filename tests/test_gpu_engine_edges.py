"""GPU parity of the decode epilogue and the encoders at the plaintext-modulus
and rounding-step edges: Decoder (csrc/engine_kernels.hpp) as compiled into
k_decrypt (every degree 4..16384, both word sizes, lazy and not), k_decode
(engine_composed.hip: q >= 2^62 and N = 32768) and combine_body
(threshold.hip, two words and one word per lane), and encode1 in k_encrypt,
k_add_plain_ntt and their composed counterparts.

The phases are planted (engine_edges.py): one on either side of the rounding
steps of every t -- 0 (-> 4), 2, 3, 4, 65537, 2^32, 2^40, 2^63, q - 1, q and
2^64 - 1 -- tiled and rotated over one workgroup full of polynomials plus
one; the noise rows put each ciphertext's maximum at a chosen coefficient.
test_engine_edges.py holds the inputs to what they claim on the CPU.
Bit-exact against the C oracle.  Host arrays, and device tensors at the
smallest and the largest degree.

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import engine_edges as G
import oracle

pytestmark = pytest.mark.gpu

DEVICE_DEGREES = (G.DEGREES[0], G.DEGREES[-1])


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


def puts(n):
    return (np.ascontiguousarray, D) if n in DEVICE_DEGREES else (np.ascontiguousarray,)


def same(got, want, where):
    got, want = H(got), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (where, bad[:4].tolist(), len(bad), [int(x) for x in (got[tuple(bad[0])], want[tuple(bad[0])])])


def oracle_decrypt(o, t, sk, ct, is_ntt):
    rows = [o.decrypt(t, sk, ct[i], is_ntt) for i in range(ct.shape[0])]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], dtype=np.uint64))


def oracle_decode(o, t, phase):
    zero = np.zeros(o.n, dtype=np.uint64)
    v, ph, mx = oracle_decrypt(o, t, zero, np.stack([phase, np.zeros_like(phase)], axis=1), False)
    assert (ph == phase).all()
    return v, mx


# ---------------------------------------------------------------- decrypt
@pytest.mark.parametrize("n,qname", G.cases())
def test_decrypt_planted_phases(fg, n, qname):
    """Planted phases under a ternary key: 2 and 3 components, coefficient
    and NTT form, with and without the phase buffer, every t."""
    q = G.moduli(n)[qname]
    r = fg.PolynomialRing(n, q)
    o = oracle.NTT(n, q)
    for t in G.plaintext_moduli(q):
        eng = fg.EncryptionEngine(r, t)
        for comps in (2, 3):
            want, s, ct = G.planted_cts(o, n, q, t, comps)
            for is_ntt in G.forms(q):
                form = G.to_ntt(o, ct) if is_ntt else ct
                ev, eph, emx = oracle_decrypt(o, t, s, form, is_ntt)
                assert (eph == want).all(), (t, comps, is_ntt)
                for put in puts(n):
                    key = fg.SecretKey(r, put(s))
                    where = (qname, t, comps, is_ntt, put.__name__)
                    res = eng.decrypt(put(form), key, is_ntt=is_ntt, with_phase=True)
                    same(res.phase, eph, where + ("phase",))
                    same(res.values, ev, where + ("values",))
                    same(res.max_noise, emx, where + ("max_noise",))
                    res = eng.decrypt(put(form), key, is_ntt=is_ntt)
                    same(res.values, ev, where + ("values, no phase",))
                    same(res.max_noise, emx, where + ("max_noise, no phase",))


# ---------------------------------------------------------------- combine_partials
def check_combine(fg, eng, q, t, ct, want, ev, emx, where, put=np.ascontiguousarray):
    c0 = np.ascontiguousarray(ct[:, 0])
    # from q = 2^63 on the reference's Lagrange coefficients of 1, 2, 3 are 0, 3, 0 (engine_edges.partials_for):
    # the last set keeps three non-zero terms in the sum at every modulus
    for lams in ([1], fg.lagrange_coefficients(q, [1, 2, 3]), [q - 3, 3, q - 1]):
        par = G.partials_for(q, c0, want, lams)
        res = eng.combine_partials(put(ct), put(par), lams, with_phase=True)
        w = where + (tuple(lams),)
        same(res.phase, want, w + ("phase",))
        same(res.values, ev, w + ("values",))
        same(res.max_noise, emx, w + ("max_noise",))


@pytest.mark.parametrize("n,qname", G.cases((4, 16, 256, 4096)))
def test_combine_planted_phases(fg, n, qname):
    """The same phases through the combination: one partial c0 - want with
    lambda 1, three with the Lagrange coefficients of the ids 1, 2, 3, and
    three with the lambdas q - 3, 3, q - 1."""
    q = G.moduli(n)[qname]
    r = fg.PolynomialRing(n, q)
    o = oracle.NTT(n, q)
    rows = G.rows_for(n)
    for t in G.plaintext_moduli(q):
        eng = fg.EncryptionEngine(r, t)
        want = G.phase_rows(n, q, t, rows)
        ev, emx = oracle_decode(o, t, want)
        ct = G.below(G.rng(n, q, q >> 32, t, t >> 32, 5), q, (rows, 2, n))
        check_combine(fg, eng, q, t, ct, want, ev, emx, (qname, t))


@pytest.mark.parametrize("qname", list(G.moduli(16)))
def test_combine_one_word_per_lane(fg, qname):
    """Device tensors that start at an odd word: not 16-byte aligned, so the
    one-word-per-lane kernel runs (k_combine_partials<1, .>)."""
    import torch

    n, rows = 16, G.rows_for(16)
    q = G.moduli(n)[qname]
    r = fg.PolynomialRing(n, q)
    o = oracle.NTT(n, q)

    def odd(a):
        buf = torch.zeros(a.size + 1, dtype=torch.int64, device="cuda:0")
        buf[1:] = D(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    for t in G.plaintext_moduli(q):
        eng = fg.EncryptionEngine(r, t)
        want = G.phase_rows(n, q, t, rows)
        ev, emx = oracle_decode(o, t, want)
        ct = G.below(G.rng(n, q, q >> 32, t, t >> 32, 6), q, (rows, 2, n))
        check_combine(fg, eng, q, t, ct, want, ev, emx, (qname, t, "odd"), put=odd)


# ---------------------------------------------------------------- noise placement
@pytest.mark.parametrize("n", G.DEGREES)
@pytest.mark.parametrize("word", [0, 1])
def test_max_noise_at_every_position(fg, n, word):
    """Row i carries its only noise, i + 1, at position noise_positions(n)[i]:
    the maximum must come out whichever lane, register slot and wave holds
    it, through decrypt (zero key) and through combine_partials."""
    q = G.moduli(n)[G.word_pair(n)[word]]
    t = G.NOISE_T
    r = fg.PolynomialRing(n, q)
    eng = fg.EncryptionEngine(r, t)
    phase, vals, d = G.noise_rows(n, q, t)
    ct = np.ascontiguousarray(np.stack([phase, G.below(G.rng(n, q, 7), q, phase.shape)], axis=1))
    zero = np.zeros(n, dtype=np.uint64)
    for put in puts(n):
        res = eng.decrypt(put(ct), fg.SecretKey(r, put(zero)), with_phase=True)
        same(res.phase, phase, (n, q, put.__name__, "phase"))
        same(res.values, vals, (n, q, put.__name__, "values"))
        same(res.max_noise, d, (n, q, put.__name__, "max_noise"))
        res = eng.decrypt(put(G.to_ntt(oracle.NTT(n, q), ct)), fg.SecretKey(r, put(zero)), is_ntt=True)
        same(res.values, vals, (n, q, put.__name__, "ntt", "values"))
        same(res.max_noise, d, (n, q, put.__name__, "ntt", "max_noise"))
        other = G.below(G.rng(n, q, 8), q, ct.shape)
        check_combine(fg, eng, q, t, other, phase, vals, d, (n, q, put.__name__), put=put)


# ---------------------------------------------------------------- encoders
@pytest.mark.parametrize("n,qname", G.cases(G.ENCODE_DEGREES))
def test_add_plain_and_encrypt_edge_values(fg, n, qname):
    """encode_values for every t through add_plain (both domains, raw words
    2^64 - 1, q, q + 1 in c0) and encrypt, at the degrees the parity tests of
    test_gpu_engine.py leave out."""
    q = G.moduli(n)[qname]
    r = fg.PolynomialRing(n, q)
    o = oracle.NTT(n, q)
    rows = G.rows_for(n)
    ct = G.raw_ciphertexts(n, q, rows)
    g = G.rng(n, q, q >> 32, 9)
    pk = G.below(g, q, (2, n))
    u = g.integers(0, 3, size=(rows, n)).astype(np.uint64)
    u[u == 2] = q - 1  # ternary
    e1, e2 = G.below(g, q, (rows, n)), G.below(g, q, (rows, n))
    e1[0, :3] = [G.M64, q, q + 1]
    key = fg.PublicKey(r, pk)
    for t in G.plaintext_moduli(q):
        eng = fg.EncryptionEngine(r, t)
        vals = G.value_rows(n, q, t, rows)
        for is_ntt in (False, True):
            want = np.stack([o.add_plain(t, ct[i], vals[i], is_ntt) for i in range(rows)])
            same(eng.add_plain(ct, vals, is_ntt=is_ntt), want, (qname, t, "add_plain", is_ntt))
        want = np.stack([o.encrypt(t, pk, vals[i], u[i], e1[i], e2[i]) for i in range(rows)])
        same(eng.encrypt(vals, key, u, e1, e2), want, (qname, t, "encrypt"))
