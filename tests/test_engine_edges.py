"""CPU checks behind test_gpu_engine_edges.py and test_gpu_keygen_edges.py (no
GPU): the C oracle against the second, pure-Python restatement
(oracle/pyref.py) of decode + noise, the encoder, the GGSW gadget and rows
and the key-switching-key bodies at the plaintext-modulus, rounding-step and
shift-count edges -- and the conditions that the GPU tests rely on, asserted
instead of assumed: that a planted ciphertext decrypts to its planted phase,
that the phases sit on both sides of the rounding steps and reach every row,
that the planted noise leaves the decode alone and is the row's maximum, and
that the key parameters reach the wrap points they name.
"""
import numpy as np
import pytest

import engine_edges as G
import lwe_edges as E
import ntt_primes as P
import oracle
from oracle import pyref

M64 = G.M64


def I(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


def oracle_decode(o, t, phase):
    """decode + noise of phase rows: the oracle's decrypt with a zero key."""
    zero = np.zeros(o.n, dtype=np.uint64)
    vals, mx = np.empty_like(phase), []
    for i in range(phase.shape[0]):
        v, ph, m = o.decrypt(t, zero, np.stack([phase[i], zero]))
        assert (ph == phase[i]).all()
        vals[i] = v
        mx.append(m)
    return vals, mx


# ---------------------------------------------------------------- helpers restated
def test_polys_per_workgroup_and_case_lists():
    assert [G.polys_per_workgroup(n) for n in (4, 8, 16, 256, 1024, 2048, 4096, 8192, 16384)] == \
        [256, 256, 256, 16, 4, 2, 1, 1, 1]
    assert G.rows_for(8192) == G.rows_for(16384) == G.rows_for(G.BIG) == 2
    for n in G.DEGREES:
        for name, q in G.moduli(n).items():
            assert P.is_prime(q) and q % (2 * n) == 1, (n, name)
        a, b = (G.moduli(n)[x] for x in G.word_pair(n))
        assert P.word_bits(a) == 32 and P.word_bits(b) == 64 and b < 1 << 62
    for n in G.FULL_DEGREES:
        qs = G.moduli(n)
        assert P.is_lazy(n, qs["lazy_top"]) and not P.is_lazy(n, qs["u32_top"])
        assert qs["u64_top"] < 1 << 62 <= qs["wide_bottom"] < qs["shoup_top"] < 1 << 63 < qs["wmont_bottom"]
    assert len(G.cases()) == 4 * 8 + 9 * 2 + 2


def test_plaintext_moduli_reach_every_branch():
    """t = 0, 2, the default 65537, t >= 2^32, t near q, t > q (delta = 0)
    and 2^64 - 1, at every modulus."""
    for n in G.DEGREES:
        for q in G.moduli(n).values():
            ts = G.plaintext_moduli(q)
            assert {0, 2, 3, 4, 65537, 1 << 32, 1 << 40, 1 << 63, q - 1, q, M64} == set(ts)
            assert any(t > q for t in ts) and any(q // 2 < t < q for t in ts)


# ---------------------------------------------------------------- decode + noise
@pytest.mark.parametrize("n,qname", G.cases())
def test_decode_noise_oracle_vs_pyref(n, qname):
    """Every planted phase alone in a row of degree 4 (the row's maximum is
    that phase's noise), for every t."""
    q = G.moduli(n)[qname]
    o = oracle.NTT(4, q)
    for t in G.plaintext_moduli(q):
        L = G.phase_list(q, t)
        assert L and all(p < q for p in L)
        rows = np.ascontiguousarray(np.broadcast_to(np.array(L, dtype=np.uint64)[:, None], (len(L), 4)))
        vals, mx = oracle_decode(o, t, rows)
        for p, v, m in zip(L, vals[:, 0], mx):
            assert (int(v), m) == pyref.decode_noise(p, q, t), (qname, t, p)
            assert int(v) == E.rounded(p, q, t) % (t or 4)


def test_decode_noise_branches_are_reached():
    """The wrap branch (distance above q / 2) at t > q, where delta = 0 and
    the distance is the phase itself; the int64 sign flip at q >= 2^63; a
    carry of lo + q / 2 into the high word of p t for a 32-bit modulus."""
    q = G.moduli(16)["shoup_top"]
    assert pyref.decode_noise(q - 1, q, M64)[1] == 1
    assert pyref.decode_noise(q // 2 + 1, q, M64)[1] == q - (q // 2 + 1)
    q = G.moduli(16)["u64_max"]  # a distance of 2^63 or more is a negative int64: never above q / 2
    assert pyref.decode_noise(q - 1, q, M64)[1] == (1 << 64) - (q - 1)
    q = G.moduli(16)["lazy_top"]
    carries = [(p, t) for t in G.plaintext_moduli(q) for p in G.phase_list(q, t)
               if ((p * (t or 4)) & M64) + q // 2 > M64]
    assert carries
    assert not any(((p * 16) & M64) + q // 2 > M64 for p in range(0, q, q // 1000))  # nor can it at t = 16
    for qn in ("wmont_bottom", "u64_max"):  # |noise| differs from the wrapped int64 somewhere
        q = G.moduli(16)[qn]
        flips = 0
        for t in G.plaintext_moduli(q):
            te = t or 4
            for p in G.phase_list(q, t):
                r = (p * te + q // 2) // q
                ex = ((r * (q // te)) & M64) % q
                d = abs(p - ex)
                flips += d > q // 2 and d >= 1 << 63
        assert flips, qn


@pytest.mark.parametrize("n,qname", G.cases())
def test_phase_rows_put_every_phase_in_the_batch(n, qname):
    q = G.moduli(n)[qname]
    rows = G.rows_for(n)
    for t in G.plaintext_moduli(q):
        L = G.phase_list(q, t)
        ph = G.phase_rows(n, q, t, rows)
        assert ph.shape == (rows, n) and set(I(ph)) == set(L), (qname, t)
        assert I(ph[1, :-1]) == I(ph[0, 1:]) or len(L) == 1  # row i is row 0 rotated by i
        te = t or 4
        ups = [p for p in L if p and E.rounded(p, q, t) == E.rounded(p - 1, q, t) + 1 and p - 1 in L]
        assert ups or te > q, (qname, t)  # both sides of a rounding step
        assert {0, (q // te) % q, ((te - 1) * (q // te)) % q} <= set(L)


@pytest.mark.parametrize("n,qname", G.cases((4, 16, 256)))
@pytest.mark.parametrize("comps", [2, 3])
def test_planted_ciphertexts_decrypt_to_their_phase(n, qname, comps):
    """c0 = want + c1 s [+ c2 s^2]: the oracle returns `want` as the phase, in
    coefficient and in NTT form, and decodes it as pyref does."""
    q = G.moduli(n)[qname]
    o = oracle.NTT(n, q)
    for t in G.plaintext_moduli(q):
        want, s, ct = G.planted_cts(o, n, q, t, comps, rows=3)
        assert ct.shape == (3, comps, n) and s[:3].all() and set(I(s)) <= {0, 1, q - 1}
        dn = {p: pyref.decode_noise(p, q, t) for p in set(I(want))}
        for is_ntt in G.forms(q):
            form = G.to_ntt(o, ct) if is_ntt else ct
            for i in range(3):
                v, ph, mx = o.decrypt(t, s, form[i], is_ntt)
                assert (ph == want[i]).all(), (qname, t, comps, i)
                assert I(v) == [dn[p][0] for p in I(want[i])]
                assert mx == max(dn[p][1] for p in I(want[i]))


def test_no_inverse_transform_from_2_63_on():
    """Why forms() leaves the NTT form out there: N^-1 comes out as 0, the
    inverse transform of anything is 0, and so is every ring product."""
    n = 16
    for name, q in G.moduli(n).items():
        o = oracle.NTT(n, q)
        x = G.below(G.rng(2), q, (2, n))
        assert (o.inv_n == 0) == (q >= 1 << 63) == (G.forms(q) == (False,)), name
        assert (o.inverse(o.forward(x)) == x).all() == (q < 1 << 63)
        assert I(o.polymul(x[:1], x[1:])) == pyref.compat_polymul(I(x[0]), I(x[1]), q)


def test_partials_sum_to_the_planted_difference():
    n, q, t = 16, G.moduli(16)["wmont_bottom"], 65537
    want = G.phase_rows(n, q, t, 3)
    c0 = G.below(G.rng(1), q, (3, n))
    for lams in ([1], [q - 3, 3, q - 1], [M64, 5], [0, 3, 0]):
        par = G.partials_for(q, c0, want, lams)
        assert par.shape == (len(lams), 3, n) and (par < np.uint64(q)).all()
        tot = sum(par[i].astype(object) * (lams[i] % q) for i in range(len(lams)))
        assert ((c0.astype(object) - tot) % q == want.astype(object)).all()


# ---------------------------------------------------------------- encoders
@pytest.mark.parametrize("n,qname", G.cases())
def test_encode_values_oracle_vs_formula(n, qname):
    q = G.moduli(n)[qname]
    for t in G.plaintext_moduli(q):
        te = t or 4
        delta = q // te
        V = G.encode_values(q, t)
        assert {0, 1, te - 1, te, 1 << 63, M64} <= set(V)
        wraps = [v for v in V if v * delta > M64]
        assert wraps or delta <= 1, (qname, t)
        if delta > 1:
            w = min(wraps)
            assert w * delta > M64 >= (w - 1) * delta
        got = oracle.encode(q, t, np.array(V, dtype=np.uint64))
        assert I(got) == [((v * delta) & M64) % q for v in V], (qname, t)


def test_value_rows_and_raw_ciphertexts():
    n, q = 64, G.moduli(64)["u64_top"]
    rows = G.rows_for(n)
    for t in G.plaintext_moduli(q):
        assert set(I(G.value_rows(n, q, t, rows))) == set(G.encode_values(q, t))
    ct = G.raw_ciphertexts(n, q, rows)
    assert {M64, q, q + 1} <= set(I(ct[:, 0])) and int(ct[0, 1, 0]) == M64


# ---------------------------------------------------------------- noise placement
@pytest.mark.parametrize("n", G.DEGREES)
def test_noise_rows_premises(n):
    """delta / 2 > rows, and v (q mod t) + rows t < q / 2 for every value v
    used, so the planted noise d_i <= rows moves no value; every position
    named is hit; checked against the oracle up to n = 1024 and with pyref at
    the noisy coefficients beyond."""
    pos = G.noise_positions(n)
    assert len(set(pos)) == len(pos) and {0, n - 1} <= set(pos)
    assert len(pos) == n or ({1 << k for k in range(P.log2(n))} <= set(pos) and len(pos) >= 61 and n > 256)
    for name in G.word_pair(n):
        q = G.moduli(n)[name]
        t = G.NOISE_T
        phase, vals, d = G.noise_rows(n, q, t)
        delta = q // t
        assert delta // 2 > len(pos) == phase.shape[0] and I(d) == list(range(1, len(pos) + 1))
        assert (phase < np.uint64(q)).all() and (vals >= 1).all() and (vals <= t - 2).all()
        assert int(vals.max()) * (q % t) + len(pos) * t < q // 2 and len(set(I(vals))) >= 3
        off = phase.astype(object) - vals.astype(object) * delta
        for r, p in enumerate(pos):
            assert off[r, p] == (r + 1 if r % 2 == 0 else -(r + 1)) and np.count_nonzero(off[r]) == 1
            assert pyref.decode_noise(int(phase[r, p]), q, t) == (int(vals[r, p]), r + 1)
        if n <= 1024:
            ov, om = oracle_decode(oracle.NTT(n, q), t, phase)
            assert (ov == vals).all() and om == I(d)


# ---------------------------------------------------------------- key material
def test_ggsw_gadget_oracle_vs_pyref_and_wrap_points():
    """The gadget through oracle.ggsw_encrypt at degree 16: coefficient 0 of
    the row's own polynomial minus the plain draw.  (l + 1) base_log reaches
    64 and passes it; g exceeds q for large |v|, where (q - g) % q wraps."""
    n = 16
    shifts = {(l + 1) * bl for _, bl, lv in G.GGSW_DECOMPS for l in range(lv)}
    assert 64 in shifts and any(s > 64 for s in shifts) and 63 in shifts and any(s < 32 for s in shifts)
    for qname, q in G.moduli(n).items():
        o = oracle.NTT(n, q)
        sk = oracle.sample(1, G.SEED, 1, q, n)
        wrapped = 0
        for k, bl, lv in G.GGSW_DECOMPS:
            out = o.ggsw_encrypt(k, bl, lv, G.GGSW_VALUES, sk, G.SEED, 20, 3.2)
            rows = len(G.GGSW_VALUES) * (k + 1) * lv
            masks = oracle.sample(0, G.SEED, 20, q, rows * k * n).reshape(rows, k, n)
            err = oracle.sample(2, G.SEED, 21, q, rows * n, 3.2).reshape(rows, n)
            ref = pyref.ggsw_encrypt(G.GGSW_VALUES, I(sk), masks, err, q, k, bl, lv)
            assert out.tolist() == ref, (qname, k, bl, lv)
            for v in G.GGSW_VALUES:
                for l in range(lv):
                    g = ((abs(v) * q) & M64) >> (((l + 1) * bl) & 63)
                    wrapped += v < 0 and g > q
                    if v < 0 and g > q:
                        assert pyref.ggsw_gadget(v, q, l, bl) != (-g) % q or (1 << 64) % q == 0
        assert wrapped or q > 1 << 63, qname  # above 2^63 no |v| q mod 2^64 of these values passes q


def test_ggsw_rows_second_reference_at_degree_256():
    n, (k, bl, lv) = 256, (2, 33, 2)
    q = G.moduli(n)["wmont_bottom"]
    o = oracle.NTT(n, q)
    sk = oracle.sample(1, G.SEED, 1, q, n)
    vals = G.GGSW_VALUES[3:5]
    rows = len(vals) * (k + 1) * lv
    masks = oracle.sample(0, G.SEED, 20, q, rows * k * n).reshape(rows, k, n)
    err = oracle.sample(2, G.SEED, 21, q, rows * n, 3.2).reshape(rows, n)
    assert o.ggsw_encrypt(k, bl, lv, vals, sk, G.SEED, 20, 3.2).tolist() == \
        pyref.ggsw_encrypt(vals, I(sk), masks, err, q, k, bl, lv)


@pytest.mark.parametrize("qname", list(G.ksk_moduli()))
@pytest.mark.parametrize("std", G.KSK_STD)
def test_ksk_oracle_vs_pyref(qname, std):
    q = G.ksk_moduli()[qname]
    assert q % (2 * G.KSK_DEGREE) == 1 and P.is_prime(q)
    g = G.glwe_key_words(q)
    negative = 0
    for dim in G.KSK_DIMS:
        sk = E.secret_key(dim)
        assert {E.INT64_MIN, -1, E.INT64_MAX}.issubset(set(I(sk))) or dim == 1
        for bl, lv in G.KSK_DECOMPS:
            ka, kb = oracle.ksk_generate(q, bl, lv, g, sk, G.SEED, 40, std)
            assert ka.shape == (len(g) * lv, dim)
            assert (ka == oracle.sample(0, G.SEED, 40, q, ka.size).reshape(ka.shape)).all()
            err = oracle.sample(2, G.SEED, 41, q, kb.size, std)
            for e in range(kb.size):
                i, l = divmod(e, lv)
                assert int(kb[e]) == pyref.ksk_body(ka[e], sk, int(err[e]), int(g[i]), q, l, bl), (qname, dim, bl, e)
                ip = sum(int(a) * int(s) for a, s in zip(ka[e], sk)) & M64
                negative += ip >> 63
    assert negative  # the truncating % meets negative sums (and a negative (int64_t)q above 2^63)


def test_ksk_moduli_sit_on_both_sides_of_2_63():
    m = G.ksk_moduli()
    assert m["P27"] < 1 << 30 and m["shoup_top"] < 1 << 63 < m["QG"] < m["u64_max"]
    assert ((1 << 64) - 59) % 8 == 5  # no degree >= 4 has 2^64 - 59 as a modulus
    assert m["shoup_top"] // 2 >= 1 << 61 and m["QG"] // 2 >= 1 << 62  # ev > q / 2 at q / 2 >= 2^62
