"""SIMD (CRT) batching of BFV plaintexts in Python integers: the definitions
of include/fhe_gpu.h written out directly.  Decode evaluates the polynomial
by Horner's rule at the powers of psi and encode is the inverse map as a
direct sum (checked against decode); nothing here goes through a transform of
the project.

n a power of two >= 4, t an odd prime with t = 1 (mod 2n), psi a primitive
2n-th root of unity mod t.  Slot s = r n/2 + i evaluates the message at
psi^e(s), e(s) = 3^i mod 2n (r = 0) or 2n - 3^i mod 2n (r = 1)."""


def exponents(n):
    """e(s) for s = 0 .. n - 1."""
    half, two_n = n // 2, 2 * n
    row0 = [pow(3, i, two_n) for i in range(half)]
    return row0 + [two_n - e for e in row0]


def slot_index(n):
    """k(s) = (e(s) - 1) / 2, the transform index of slot s."""
    return [(e - 1) // 2 for e in exponents(n)]


def find_psi(n, t):
    """The root fhe_ctx_create picks: the smallest g >= 2 whose power
    g^((t-1)/2n) has order exactly 2n."""
    assert (t - 1) % (2 * n) == 0
    for g in range(2, t):
        w = pow(g, (t - 1) // (2 * n), t)
        if pow(w, n, t) == t - 1:
            return w
    raise ValueError("no primitive 2n-th root")


def horner(poly, x, t):
    acc = 0
    for c in reversed(poly):
        acc = (acc * x + int(c)) % t
    return acc


def decode(poly, t, psi):
    """out[s] = poly(psi^e(s)) mod t; poly any integers, read mod t."""
    n = len(poly)
    return [horner(poly, pow(psi, e, t), t) for e in exponents(n)]


def encode(values, t, psi):
    """The polynomial m of degree < n with m(psi^e(s)) = values[s] mod t, by
    the inverse of the evaluation map written as a sum: m_j = n^-1 sum_s
    values[s] psi^(-j e(s)) (the roots psi^e, e odd, are the zeros of X^n + 1,
    and sum over odd e of psi^(e (j - j')) = n [j = j'] for |j - j'| < n)."""
    n = len(values)
    ninv = pow(n, -1, t)
    roots_inv = [pow(psi, -e, t) for e in exponents(n)]
    vals = [int(v) % t for v in values]
    out, powers = [], [1] * n  # powers[s] = psi^(-j e(s))
    for _ in range(n):
        out.append(ninv * sum(v * p for v, p in zip(vals, powers)) % t)
        powers = [p * r % t for p, r in zip(powers, roots_inv)]
    return out


def lift(poly, t, q):
    """The centred representative mod q of words in [0, t)."""
    return [c if c <= (t - 1) // 2 else q - (t - c) for c in poly]


def rotation_element(n, steps, swap=False):
    """g(steps, swap) = 3^(steps mod n/2) (2n - 1)^swap mod 2n."""
    g = pow(3, steps % (n // 2), 2 * n)
    return g * (2 * n - 1) % (2 * n) if swap else g


def rotate(values, steps, swap=False):
    """w[r][i] = v[r xor swap][(i + steps) mod n/2]."""
    n = len(values)
    half = n // 2
    return [values[((s // half) ^ int(bool(swap))) * half + (s % half + steps) % half] for s in range(n)]


def slot_sum_elements(n):
    """3^(2^i) mod 2n for i < log2(n/2), then 2n - 1."""
    return [pow(3, 1 << i, 2 * n) for i in range((n // 2).bit_length() - 1)] + [2 * n - 1]
