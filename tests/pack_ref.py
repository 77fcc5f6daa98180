"""The contract of fhe_lwe_pack_batch and fhe_pack_key_generate
(include/fhe_gpu.h) restated on the CPU, shared by tests/test_pack_abi.py and
tests/test_gpu_pack.py.

pack_formula_int   the header formula word by word in Python integers (small
                   shapes).
pack_formula       the same words with numpy: the u64 product wraps natively,
                   the canonical terms are summed exactly as two 32-bit halves.
pack_gadget        m_e of fhe_pack_key_generate.
"""
import numpy as np

M64 = (1 << 64) - 1


def digits(word, base_log, level):
    """d(s, e) for e = i level + l, l = 0 .. level - 1, of one raw mask word."""
    mask = (1 << base_log) - 1
    return [(int(word) >> ((level - 1 - l) * base_log)) & mask for l in range(level)]


def pack_formula_int(q, n, base_log, level, key, lwe_a, lwe_b, slots, prev=None):
    """key [entries][2][n], lwe_a [S][in_dim], lwe_b [S] of ONE output
    ciphertext -> out [2][n]; prev [2][n] is `out` before an accumulating call."""
    out = [[0] * n for _ in range(2)]
    for s, h in enumerate(slots):
        d = [x for word in lwe_a[s] for x in digits(word, base_log, level)]
        W = [[0] * n for _ in range(2)]
        for p in range(2):
            for j in range(n):
                total = sum(((d[e] * int(key[e][p][j])) & M64) % q for e in range(len(d)))
                W[p][j] = (-total + (int(lwe_b[s]) % q if p == 0 and j == 0 else 0)) % q
        for p in range(2):
            for j in range(n):
                out[p][j] += W[p][j - h] if j >= h else (q - W[p][n + j - h]) % q
    for p in range(2):
        for j in range(n):
            out[p][j] = (out[p][j] + (int(prev[p][j]) % q if prev is not None else 0)) % q
    return out


def pack_formula(q, n, base_log, level, key, lwe_a, lwe_b, slots, prev=None):
    """key [entries, 2, n], lwe_a [batch, S, in_dim], lwe_b [batch, S] (uint64)
    -> out [batch, 2, n] uint64."""
    key = np.ascontiguousarray(key, dtype=np.uint64)
    lwe_a = np.asarray(lwe_a, dtype=np.uint64)
    lwe_b = np.asarray(lwe_b, dtype=np.uint64)
    batch, S, in_dim = lwe_a.shape
    shifts = np.array([(level - 1 - l) * base_log for l in range(level)], dtype=np.uint64)
    dig = (lwe_a[..., None] >> shifts) & np.uint64((1 << base_log) - 1)  # [batch, S, in_dim, level]
    dig = dig.reshape(batch, S, in_dim * level)
    qq, lo32 = np.uint64(q), np.uint64(0xFFFFFFFF)
    out = np.empty((batch, 2, n), dtype=np.uint64)
    for c in range(batch):
        acc = np.zeros((2, n), dtype=object)
        for s, h in enumerate(slots):
            terms = (dig[c, s][:, None, None] * key) % qq  # u64 product wraps at 2^64
            total = (terms >> np.uint64(32)).sum(axis=0).astype(object) * (1 << 32) + (terms & lo32).sum(axis=0).astype(object)
            W = (-total) % q
            W[0, 0] = (W[0, 0] + int(lwe_b[c, s]) % q) % q
            R = np.roll(W, h, axis=1)
            R[:, :h] = (q - R[:, :h]) % q
            acc = acc + R
        if prev is not None:
            acc = acc + (np.asarray(prev[c], dtype=np.uint64) % qq).astype(object)
        out[c] = (acc % q).astype(np.uint64)
    return out


def pack_gadget(q, v, l, base_log, level):
    """m_e of row e = i level + l for the LWE key coefficient v = lwe_sk[i]."""
    g = (abs(int(v)) % q) * ((1 << ((level - 1 - l) * base_log)) % q) % q
    return (q - g) % q if v < 0 else g
