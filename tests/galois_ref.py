"""The contract of fhe_poly_galois_batch, fhe_switch_key_generate,
fhe_ct_galois_batch and fhe_ct_trace_batch (include/fhe_gpu.h) restated on the
CPU, shared by tests/test_galois_abi.py and tests/test_gpu_galois.py.

sigma_int, ct_galois_int, trace_int   the header formulas word by word in
        Python integers (small shapes); the ring product is passed in.
switch_key_int                        b_l of fhe_switch_key_generate over given
        draws.
sigma, ct_galois, trace               the same words with numpy for the GPU
        side; the product takes and returns [rows, n] uint64 arrays.
negacyclic_schoolbook                 this file's own X^n = -1 product.
"""
import numpy as np

M64 = (1 << 64) - 1


def negacyclic_schoolbook(a, b, q):
    """a * b mod (X^n + 1, q) on Python integers."""
    n = len(a)
    c = [0] * n
    for i, x in enumerate(a):
        if x % q == 0:
            continue
        for j, y in enumerate(b):
            if i + j < n:
                c[i + j] += x * y
            else:
                c[i + j - n] -= x * y
    return [v % q for v in c]


def trace_elements(n, steps):
    """g_i = n / 2^i + 1."""
    return [(n >> i) + 1 for i in range(steps)]


def sigma_int(p, g, q):
    """The definition: out[j g mod 2n] = +-p[j] (a scatter)."""
    n = len(p)
    assert g % 2 == 1 and 1 <= g < 2 * n
    out = [None] * n
    for j in range(n):
        k = j * g % (2 * n)
        if k < n:
            out[k] = int(p[j]) % q
        else:
            out[k - n] = (q - int(p[j]) % q) % q
    assert None not in out
    return out


def digits_int(word, base_log, level):
    """Relinearisation's unsigned LSB-first digits of one word."""
    return [(int(word) >> (l * base_log)) & ((1 << base_log) - 1) for l in range(level)]


def ct_galois_int(q, base_log, level, g, key, ct, add_input, mul):
    """key [level][2][n] = (a_l, b_l) in coefficient form, ct [2][n] raw words
    -> out [2][n]; mul(a, b, q) is the context's product."""
    n = len(ct[0])
    s0, s1 = sigma_int(ct[0], g, q), sigma_int(ct[1], g, q)
    out0 = [(x + (int(c) % q if add_input else 0)) % q for x, c in zip(s0, ct[0])]
    out1 = [int(c) % q if add_input else 0 for c in ct[1]]
    for l in range(level):
        d = [digits_int(w, base_log, level)[l] for w in s1]
        out0 = [(x + y) % q for x, y in zip(out0, mul(d, key[l][1], q))]
        out1 = [(x + y) % q for x, y in zip(out1, mul(d, key[l][0], q))]
    assert len(out0) == n
    return [out0, out1]


def trace_int(q, base_log, level, steps, keys, ct, mul):
    """keys [steps][level][2][n], ct [2][n] -> out [2][n]."""
    n = len(ct[0])
    inv = pow(pow(2, steps, q), -1, q)
    x = [[int(c) % q * inv % q for c in row] for row in ct]
    for i, g in enumerate(trace_elements(n, steps)):
        x = ct_galois_int(q, base_log, level, g, keys[i], x, True, mul)
    return x


def switch_key_int(q, base_log, g, sk_to, sk_from, masks, errs, mul):
    """(a_l, b_l) of fhe_switch_key_generate over the draws masks [level][n]
    and errs [level][n] (signed integers): b_l = a_l (*) sk_to + e_l +
    m * power_l with m = -sigma_g(sk_from) and the u64 power update."""
    m = [(q - v) % q for v in sigma_int(sk_from, g, q)]
    key, power = [], 1
    for a, e in zip(masks, errs):
        b = [(x + int(err) + v * (power % q)) % q for x, err, v in zip(mul(a, [s % q for s in sk_to], q), e, m)]
        key.append([[int(v) % q for v in a], b])
        power = ((power * (1 << base_log)) & M64) % q
    return key


# ---- numpy ---------------------------------------------------------------
def _addq(a, b, q):
    """mod_add of canonical uint64 arrays, any q < 2^64."""
    s = a + b
    return np.where((s < a) | (s >= np.uint64(q)), s - np.uint64(q), s)


def sigma(a, g, q):
    """sigma_g along the last axis of a uint64 array, as a gather with g^-1:
    out[k] = +-a[k g^-1 mod 2n]."""
    a = np.asarray(a, dtype=np.uint64)
    n = a.shape[-1]
    assert g % 2 == 1 and 1 <= g < 2 * n
    j = np.arange(n, dtype=np.int64) * pow(g, -1, 2 * n) % (2 * n)
    x = a[..., j % n] % np.uint64(q)
    return np.where((j >= n) & (x != 0), np.uint64(q) - x, x)


def ct_galois(q, base_log, level, g, key, ct, add_input, mul):
    """key [level, 2, n] coefficient form, ct [batch, 2, n] -> [batch, 2, n];
    mul(a, b) multiplies [rows, n] uint64 arrays row by row."""
    ct = np.asarray(ct, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    batch, _, n = ct.shape
    s = sigma(ct, g, q)
    zero = np.zeros((batch, n), dtype=np.uint64)
    out0 = _addq(s[:, 0], ct[:, 0] % np.uint64(q) if add_input else zero, q)
    out1 = ct[:, 1] % np.uint64(q) if add_input else zero
    for l in range(level):
        d = (s[:, 1] >> np.uint64(l * base_log)) & np.uint64((1 << base_log) - 1)
        out0 = _addq(out0, mul(d, np.broadcast_to(key[l, 1], d.shape)), q)
        out1 = _addq(out1, mul(d, np.broadcast_to(key[l, 0], d.shape)), q)
    return np.stack([out0, out1], axis=1)


def mul_scalar(a, s, q):
    """(a mod q) * s mod q, exact."""
    a = np.asarray(a, dtype=np.uint64) % np.uint64(q)
    return ((a.astype(object) * int(s)) % q).astype(np.uint64)


def trace(q, base_log, level, steps, keys, ct, mul):
    """keys [steps, level, 2, n], ct [batch, 2, n] -> [batch, 2, n]."""
    n = np.shape(ct)[-1]
    x = mul_scalar(ct, pow(pow(2, steps, q), -1, q), q)
    for i, g in enumerate(trace_elements(n, steps)):
        x = ct_galois(q, base_log, level, g, keys[i], x, True, mul)
    return x
