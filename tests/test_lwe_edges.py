"""CPU checks behind test_gpu_lwe_edges.py (no GPU): the C oracle against the
second, pure-Python restatement (oracle/pyref.py) for key switch, decompose,
sample extract, monomial rotation and LWE decryption over the modulus ladder
and the input builders of lwe_edges.py -- and the conditions that the GPU
tests rely on, asserted instead of assumed: that the inputs make the
reference's running update wrap past 2^64 wherever the modulus allows it (and
nowhere else), that every dispatch case reaches the path it names, and that
the decompose words put every edge digit at every level.
"""
import numpy as np
import pytest

import lwe_edges as E
import ntt_primes as P
import oracle
from oracle import pyref

M64 = E.M64
ladder = pytest.mark.parametrize("qname", list(E.KS_MODULI))


def I(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


def both_key_switch(q, bl, lv, ka, kb, la, lb, skip_first_body=True):
    """Per ciphertext: oracle == pyref; -> (mask wraps, body wraps) summed."""
    mw = bw = 0
    for i in range(la.shape[0]):
        oa, ob = oracle.key_switch(q, bl, lv, ka, kb, la[i], int(lb[i]))
        pa, pb, m, b = pyref.key_switch(ka, kb, la[i], int(lb[i]), q, bl, lv, out_dim=ka.shape[1],
                                        skip_first_body=skip_first_body)
        assert I(oa) == pa and ob == pb, (q, bl, lv, i)
        mw, bw = mw + m, bw + b
    return mw, bw


# ---------------------------------------------------------------- key switch
@ladder
@pytest.mark.parametrize("keys", E.KEY_KINDS)
def test_key_switch_ladder_oracle_vs_pyref_and_wraps(qname, keys):
    """Every mask kind against every key kind at every ladder modulus.  The
    running update r + q - term (r < q after the first body update, term < q)
    stays below 2q: it cannot wrap at q <= 2^63, and with the column of ones
    it must at every q above."""
    q = E.KS_MODULI[qname]
    L = E.LADDER
    ka, kb = E.ks_keys(keys, q, L["in_dim"] * L["level"], L["out_dim"])
    kinds, la = E.ks_masks(q, L["in_dim"], L["batch"])
    assert set(kinds) == set(E.MASK_KINDS)
    lb = E.ks_bodies(q, L["batch"])
    assert any(int(b) >= q for b in lb)
    mw, bw = both_key_switch(q, L["base_log"], L["level"], ka, kb, la, lb)
    if q <= 1 << 63:
        assert (mw, bw) == (0, 0), (qname, keys, mw, bw)
    elif keys == "ones":
        assert mw >= 1 and bw >= 1, (qname, mw, bw)
        # the row of digits 1 alone: its second update wraps in the column of ones, and from its
        # body of 0 (q - 1 after the first update) in the body as well
        ones = kinds.index("ones")
        assert int(lb[ones]) == 0
        _, _, m, b = pyref.key_switch(ka, kb, la[ones], 0, q, L["base_log"], L["level"], skip_first_body=True)
        assert m >= 1 and b >= 1, (qname, m, b)
    # the raw body: without a digit it comes back as it is
    zero = kinds.index("zero")
    assert oracle.key_switch(q, L["base_log"], L["level"], ka, kb, la[zero], int(lb[zero]))[1] == int(lb[zero])


def test_only_the_column_of_ones_wraps_just_above_2_63():
    """Why one modulus just above 2^63 proves nothing without it: at 2^63 + 29
    the seeded keys wrap in no update at all."""
    q = E.KS_MODULI["2^63+29"]
    L = E.LADDER
    kinds, la = E.ks_masks(q, L["in_dim"], L["batch"])
    lb = E.ks_bodies(q, L["batch"])
    ka, kb = E.ks_keys("canonical", q, L["in_dim"] * L["level"], L["out_dim"])
    assert both_key_switch(q, L["base_log"], L["level"], ka, kb, la, lb) == (0, 0)


@pytest.mark.parametrize("q", [E.P62, E.Q_TOP])
@pytest.mark.parametrize("bl,lv", E.KS_DECOMPS)
def test_key_switch_decompositions_oracle_vs_pyref(q, bl, lv):
    C = E.DECOMP_CASE
    plan = E.ks_plan(q, bl, lv, C["in_dim"], C["out_dim"], C["batch"])
    assert plan["path"] == ("acc" if q == E.P62 and bl <= 32 else "generic")
    assert plan["literal"] == (q == E.Q_TOP)
    for keys in ("raw", "ones"):
        ka, kb = E.ks_keys(keys, q, C["in_dim"] * lv, C["out_dim"])
        _, la = E.ks_masks(q, C["in_dim"], C["batch"])
        mw, bw = both_key_switch(q, bl, lv, ka, kb, la, E.ks_bodies(q, C["batch"], roll=3))
        assert (mw > 0 and bw > 0) if (q == E.Q_TOP and keys == "ones") else q == E.Q_TOP or (mw, bw) == (0, 0)


@ladder
def test_ladder_paths(qname):
    q = E.KS_MODULI[qname]
    L = E.LADDER
    plan = E.ks_plan(q, L["base_log"], L["level"], L["in_dim"], L["out_dim"], L["batch"])
    odd_below = q % 2 == 1 and q < 1 << 63
    assert plan["path"] == ("acc" if odd_below else "generic")
    assert plan["literal"] == (q >= 1 << 63)
    if odd_below:
        assert plan["ct"] == 16 and plan["splits"] > 1  # 17 ciphertexts: a ragged second tile; k_ks_sum


def test_ladder_reaches_every_kernel():
    L = E.LADDER
    got = {(p["path"], p["literal"]) for p in (E.ks_plan(q, L["base_log"], L["level"], L["in_dim"], L["out_dim"],
                                                          L["batch"]) for q in E.KS_MODULI.values())}
    assert got == {("acc", False), ("generic", False), ("generic", True)}


@pytest.mark.parametrize("q", [E.P27, E.P62])
@pytest.mark.parametrize("case", list(E.ACC_CASES))
def test_deferred_dispatch_cases_reach_their_path(q, case):
    in_dim, lv, bl, out_dim, batches = E.ACC_CASES[case]
    cts = set()
    for b in batches:
        plan = E.ks_plan(q, bl, lv, in_dim, out_dim, b)
        assert plan["path"] == "acc" and plan["launches"] == 1, (case, b)
        assert plan["ct"] == (16 if b >= 16 else 4 if b >= 4 else 1), (case, b)
        assert E.ACC_EXPECT[case](plan), (case, b, plan)
        assert plan["splits"] * plan["per_split"] >= in_dim * lv > (plan["splits"] - 1) * plan["per_split"]
        cts.add((plan["ct"], b % plan["ct"] != 0))
    if batches == E.ACC_BATCHES:  # every template, with a full and with a ragged last tile
        assert cts == {(1, False), (4, False), (4, True), (16, False), (16, True)}


@pytest.mark.parametrize("q", [E.P62, E.Q_TOP])
def test_chunk_case_takes_two_launches(q):
    C = E.CHUNK_CASE
    plan = E.ks_plan(q, C["base_log"], C["level"], C["in_dim"], C["out_dim"], C["batch"])
    assert plan["path"] == ("acc" if q == E.P62 else "generic")
    assert plan["ct"] == 16 and plan["chunk"] == 65535 * 16 and plan["launches"] == 2 and plan["splits"] == 1
    assert C["batch"] - plan["chunk"] == 17  # the second launch: one full tile and one ciphertext
    assert C["batch"] % C["distinct"] and plan["chunk"] % C["distinct"]  # the tiling is not aligned to the chunk


# ---------------------------------------------------------------- decompose
@pytest.mark.parametrize("qname", list(E.ctx_moduli(16)))
@pytest.mark.parametrize("bl,lv", E.DECOMPS)
def test_decompose_oracle_vs_pyref(qname, bl, lv):
    q = E.ctx_moduli(16)[qname]
    rows = E.decompose_rows(q, 16, bl, lv)
    for r in rows:
        assert [I(x) for x in oracle.decompose(q, r, bl, lv)] == pyref.decompose(I(r), q, bl, lv), (qname, bl, lv)


@pytest.mark.parametrize("bl,lv", E.DECOMPS)
def test_decompose_words_put_every_edge_digit_at_every_level(bl, lv):
    words = I(E.decompose_rows(97, 16, bl, lv))
    seen = {(l, d) for w in words for l, d in enumerate(E.digits_of(w, bl, lv))}
    want = {(l, d) for l in range(lv) for d in E.edge_digits(bl)}
    assert want <= seen, sorted(want - seen)
    base = 1 << bl
    assert {0, 1, base - 1, base // 2} <= set(E.edge_digits(bl)) | {base}  # bl = 1: half + 1 = base is no digit


def test_decompose_below_the_digit_base_wraps_like_u64():
    """A negative digit d - B is stored as (q - (B - d)) % q in u64 words.
    B - d < B / 2, so at q = 97 nothing wraps up to base_log 7; at base_log
    15 the digit half + 1 has B - d = 2^14 - 1 > q: the difference wraps and
    the stored word is 2^64 mod q away from the centred digit."""
    q = 97
    assert pyref.decompose([65], q, 7, 1) == [[q - 63]]
    d, gap = (1 << 14) + 1, (1 << 14) - 1
    got = pyref.decompose([d], q, 15, 1)[0][0]
    assert got == ((q - gap) & M64) % q == ((q - gap) % q + (1 << 64)) % q != (q - gap) % q
    assert got == int(oracle.decompose(q, np.array([d], np.uint64), 15, 1)[0][0])


# ---------------------------------------------------------------- sample extract / rotate
@pytest.mark.parametrize("n", [16, 1024])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_sample_extract_and_rotate_oracle_vs_pyref(n, k):
    for qname, q in P.stream_primes(n).items():
        W = P.stream_words(q)
        g = E.planted_glwe(q, n, k, len(W))
        for c in range(len(W)):
            oa, ob = oracle.sample_extract(q, g[c])
            pa, pb = pyref.sample_extract(g[c], q)
            assert I(oa) == pa and ob == pb == int(g[c, k, 0]), (qname, c)
        seen = {int(v) for v in g[:, :k, (0, 1, n - 1)].reshape(-1)} | {int(v) for v in g[:, k, 0]}
        assert set(W) <= seen
        rots = E.rotations(n)
        for c in range(len(W) if n == 16 else 3):
            for rot in rots:
                assert I(oracle.rotate(q, g[c, 0], rot)) == pyref.rotate(I(g[c, 0]), rot, q), (qname, c, rot)


# ---------------------------------------------------------------- LWE decryption
@ladder
def test_lwe_decrypt_oracle_vs_pyref(qname):
    q = E.KS_MODULI[qname]
    for t in E.plaintext_moduli(q):
        for dim in (1, 65) if qname != "2^64-59" else E.LWE_DIMS:
            sk, a, b, want = E.lwe_cases(q, t, dim)
            assert {0, 1 % q, q - 1} <= set(want)
            assert any(int(x) >= q for x in b) or q > 1 << 63  # b + q fits the word below 2^63
            for i in range(len(want)):
                v, ph = oracle.lwe_decrypt(q, t, sk, a[i], int(b[i]))
                assert (v, ph) == pyref.lwe_decrypt(I(sk), I(a[i]), int(b[i]), q, t), (qname, t, dim, i)
                assert ph == want[i] and v == E.rounded(ph, q, t) % (t or 4)


def test_edge_phases_sit_on_the_rounding_boundaries():
    for q in E.KS_MODULI.values():
        for t in E.plaintext_moduli(q):
            ph = E.edge_phases(q, t)
            ups = [p for p in ph if p and E.rounded(p, q, t) == E.rounded(p - 1, q, t) + 1]
            assert ups or (t or 4) > q or q < 4, (q, t)  # t > q: every step of the phase is a step of the value
