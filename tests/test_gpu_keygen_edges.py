"""Device key generation (csrc/keygen.hip) at the wrap points of the
reference's u64 / int64 arithmetic, bit for bit against the C oracle
(test_engine_edges.py holds the oracle to oracle/pyref.py there):

  ggsw_gadget / k_ggsw_finish  (l + 1) base_log at 63, 64 and beyond (the
      shift count mod 64), |v| up to 2^63, so that the gadget passes q and
      (q - g) % q wraps in u64; every stream_primes modulus, the wide ones on
      the composed key product
  k_ksk_body  LWE dimensions around its 64-lane stride (one, two and three
      trips), int64 keys with INT64_MIN and INT64_MAX, raw GLWE key words,
      moduli on both sides of 2^63: the negative (int64_t)q in s % q and
      ev > q / 2 at q / 2 >= 2^62

Run on an MI355X with ``pytest -m gpu``.
"""
import numpy as np
import pytest

import engine_edges as G
import lwe_edges as E
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fg():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fhe_gpu

    return fhe_gpu


def same(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (where, bad[:4].tolist(), len(bad), [int(x) for x in (got[tuple(bad[0])], want[tuple(bad[0])])])


@pytest.mark.parametrize("n,qname", G.cases(G.GGSW_DEGREES))
def test_ggsw_at_the_shift_and_sign_edges(fg, n, qname):
    q = G.moduli(n)[qname]
    ring = fg.PolynomialRing(n, q)
    ref = oracle.NTT(n, q)
    kg = fg.KeyGenerator(ring, G.SEED, noise_std=3.2)
    sk = oracle.sample(1, G.SEED, 1, q, n)
    vals = np.array(G.GGSW_VALUES, dtype=np.int64)
    for k, bl, lv in G.GGSW_DECOMPS:
        got = kg.ggsw(vals, sk, k, bl, lv, 20)
        same(got, ref.ggsw_encrypt(k, bl, lv, vals, sk, G.SEED, 20, 3.2), (qname, k, bl, lv))


@pytest.mark.parametrize("qname", list(G.ksk_moduli()))
@pytest.mark.parametrize("dim", G.KSK_DIMS)
def test_key_switch_key_at_the_stride_and_sign_edges(fg, qname, dim):
    q = G.ksk_moduli()[qname]
    ring = fg.PolynomialRing(G.KSK_DEGREE, q)
    kg = fg.KeyGenerator(ring, G.SEED)
    g = G.glwe_key_words(q)
    sk = E.secret_key(dim)
    for bl, lv in G.KSK_DECOMPS:
        for std in G.KSK_STD:
            ka, kb = kg.key_switch_key(g, sk, bl, lv, 40, std_dev=std)
            ra, rb = oracle.ksk_generate(q, bl, lv, g, sk, G.SEED, 40, std)
            same(ka, ra, (qname, dim, bl, lv, std, "mask"))
            same(kb, rb, (qname, dim, bl, lv, std, "body"))
