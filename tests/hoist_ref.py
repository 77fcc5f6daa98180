"""The contracts of fhe_ct_hoist_batch, fhe_ct_hoisted_galois_batch and
fhe_ct_hoisted_linear_batch (include/fhe_gpu.h) restated on the CPU, shared by
tests/test_hoist_abi.py and tests/test_gpu_hoist.py.  Built on
galois_ref.sigma / sigma_int / digits_int; the ring product (and, for the
hoisted rows, the forward transform) is passed in.

pi                                    the spectrum action of sigma_g.
hoist_int, hoisted_galois_int,
hoisted_linear_int                    the header formulas in Python integers.
hoist_rows, hoisted_galois,
hoisted_linear                        the same words with numpy; mul(a, b)
        multiplies [rows, n] uint64 arrays row by row.
"""
import numpy as np

import galois_ref as G


def pi(n, g, k):
    """pi_g(k) = (((2k + 1) g mod 2n) - 1) / 2: fwd(sigma_g(a))[k] = fwd(a)[pi_g(k)]."""
    assert g % 2 == 1 and 1 <= g < 2 * n
    return (((2 * k + 1) * g) % (2 * n) - 1) // 2


# ---- Python integers -------------------------------------------------------
def digit_rows_int(q, base_log, level, c1):
    """d_l [level][n]: the unsigned digits of c1 mod q itself."""
    red = [int(w) % q for w in c1]
    return [[G.digits_int(w, base_log, level)[l] for w in red] for l in range(level)]


def hoist_int(q, base_log, level, ct, fwd):
    """ct [2][n] raw words -> [1 + level][n]; fwd(poly) is the context's transform of canonical words."""
    return [fwd([int(w) % q for w in ct[0]])] + [fwd(d) for d in digit_rows_int(q, base_log, level, ct[1])]


def hoisted_galois_int(q, base_log, level, g, key, ct, mul):
    """key [level][2][n] = (a_l, b_l) in coefficient form, ct [2][n] raw words
    -> [2][n]: out0 = sigma_g(c0) + sum_l sigma_g(d_l) (*) b_l, out1 = sum_l
    sigma_g(d_l) (*) a_l; mul(a, b, q) is the context's product."""
    n = len(ct[0])
    out0 = G.sigma_int(ct[0], g, q)
    out1 = [0] * n
    for l, d in enumerate(digit_rows_int(q, base_log, level, ct[1])):
        sd = G.sigma_int(d, g, q)
        out0 = [(x + y) % q for x, y in zip(out0, mul(sd, key[l][1], q))]
        out1 = [(x + y) % q for x, y in zip(out1, mul(sd, key[l][0], q))]
    return [out0, out1]


def hoisted_linear_int(q, base_log, level, gs, keys, pts, ct, mul, acc=None):
    """keys[r] the key of gs[r], pts[r] the plaintext polynomial of term r
    (coefficient form, canonical), acc an optional [2][n] addend."""
    n = len(ct[0])
    out = [[int(w) % q for w in row] for row in acc] if acc is not None else [[0] * n, [0] * n]
    for g, key, p in zip(gs, keys, pts):
        rot = hoisted_galois_int(q, base_log, level, g, key, ct, mul)
        for j in range(2):
            out[j] = [(x + y) % q for x, y in zip(out[j], mul(rot[j], p, q))]
    return out


# ---- numpy -----------------------------------------------------------------
def digit_rows(q, base_log, level, c1):
    """c1 [batch, n] raw -> [batch, level, n]."""
    red = np.asarray(c1, dtype=np.uint64) % np.uint64(q)
    mask = np.uint64((1 << base_log) - 1)
    return np.stack([(red >> np.uint64(l * base_log)) & mask for l in range(level)], axis=1)


def hoist_rows(q, base_log, level, ct):
    """ct [batch, 2, n] -> the coefficient rows [batch, 1 + level, n] whose transforms are the hoisted rows."""
    ct = np.asarray(ct, dtype=np.uint64)
    return np.concatenate([(ct[:, :1] % np.uint64(q)), digit_rows(q, base_log, level, ct[:, 1])], axis=1)


def hoisted_galois(q, base_log, level, gs, key_idx, keys, ct, mul):
    """keys [nkeys, level, 2, n] coefficient form, ct [batch, 2, n] -> [batch, len(gs), 2, n]."""
    ct = np.asarray(ct, dtype=np.uint64)
    keys = np.asarray(keys, dtype=np.uint64)
    batch, _, n = ct.shape
    rows = hoist_rows(q, base_log, level, ct)
    out = np.zeros((batch, len(gs), 2, n), dtype=np.uint64)
    for r, (g, ki) in enumerate(zip(gs, key_idx)):
        s = G.sigma(rows, g, q)  # [batch, 1 + level, n]
        out0, out1 = s[:, 0], np.zeros((batch, n), dtype=np.uint64)
        for l in range(level):
            d = np.ascontiguousarray(s[:, 1 + l])
            out0 = G._addq(out0, mul(d, np.broadcast_to(keys[ki, l, 1], d.shape)), q)
            out1 = G._addq(out1, mul(d, np.broadcast_to(keys[ki, l, 0], d.shape)), q)
        out[:, r, 0], out[:, r, 1] = out0, out1
    return out


def hoisted_linear(q, rots, pts, mul, acc=None):
    """rots [batch, nterms, 2, n] (hoisted_galois), pts [nterms, n] coefficient
    form -> [batch, 2, n] = sum_r pts[r] (*) rots[:, r] (+ acc mod q)."""
    batch, nterms, _, n = rots.shape
    out = (np.asarray(acc, dtype=np.uint64) % np.uint64(q)) if acc is not None else np.zeros((batch, 2, n), np.uint64)
    for r in range(nterms):
        for j in range(2):
            x = np.ascontiguousarray(rots[:, r, j])
            out[:, j] = G._addq(out[:, j], mul(x, np.broadcast_to(pts[r], x.shape)), q)
    return out
