"""Exact-integer model of the scale-invariant BFV product (helpers of
test_scaled_abi.py and test_gpu_scaled.py).  Pure Python integers; nothing
here touches the library.

  lift(x, q)            centred residue of any integer x mod q
  rnd(Y, q)             the integer nearest to Y / q (q odd: no ties)
  negacyclic(a, b)      a (*) b in Z[X]/(X^n + 1), schoolbook
  negacyclic_kron(a, b) the same through one big-integer product (n >= 256)
  multiply_scaled, dot_scaled, square_scaled
                        the words of include/fhe_gpu.h's definition
  three_channel(...)    rnd(t X) mod q from X mod q, X mod p1, X mod p2 alone:
                        the method of bfv_scale.hip, written out separately
                        from the direct rounding
"""
from __future__ import annotations

import random

# the library's auxiliary primes (fhe_scale_info.aux reports the two in use)
AUX_PRIMES = (4611686018326724609, 1152921504606584833, 4611686018425815041)


def aux_for(q: int):
    """The two auxiliary primes of a context with modulus q."""
    return tuple(p for p in AUX_PRIMES if p != q)[:2]


def lift(x: int, q: int) -> int:
    r = x % q
    return r if r <= (q - 1) // 2 else r - q


def centred(y: int, q: int) -> int:
    return lift(y, q)


def rnd(y: int, q: int) -> int:
    """(Y - c) / q with c the centred remainder of Y mod q."""
    c = centred(y, q)
    assert (y - c) % q == 0
    return (y - c) // q


def negacyclic(a, b):
    """Schoolbook product of integer rows mod X^n + 1 (no modulus)."""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x == 0:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                out[k] += x * y
            else:
                out[k - n] -= x * y
    return out


def _pack(a, nbytes):
    """sum_i a_i 256^(nbytes i) for signed a_i, through byte strings (linear time)."""
    pos = b"".join((x if x > 0 else 0).to_bytes(nbytes, "little") for x in a)
    neg = b"".join((-x if x < 0 else 0).to_bytes(nbytes, "little") for x in a)
    return int.from_bytes(pos, "little") - int.from_bytes(neg, "little")


def negacyclic_kron(a, b):
    """Kronecker substitution: evaluate both rows at 2^width, multiply once,
    read the 2n - 1 signed digits back, fold mod X^n + 1."""
    n = len(a)
    ma = max(1, max(abs(x) for x in a))
    mb = max(1, max(abs(x) for x in b))
    nbytes = ((n * ma * mb).bit_length() + 2 + 7) // 8  # |coefficient| <= n ma mb < 2^(width - 2)
    width = 8 * nbytes
    prod = _pack(a, nbytes) * _pack(b, nbytes)
    # signed digits: add half to every digit, so that all are in [0, 2^width), and read the bytes
    half = 1 << (width - 1)
    digits = 2 * n - 1
    prod += int.from_bytes(half.to_bytes(nbytes, "little") * digits, "little")
    assert 0 <= prod < 1 << (width * digits)
    raw = prod.to_bytes(nbytes * digits, "little")
    full = [int.from_bytes(raw[k * nbytes:(k + 1) * nbytes], "little") - half for k in range(digits)]
    return [full[k] - (full[k + n] if k + n < digits else 0) for k in range(n)]


def ring_mul(a, b):
    return negacyclic_kron(a, b) if len(a) >= 256 else negacyclic(a, b)


def tensor(ct1, ct2, q):
    """(X0, X1, X2) over the integers for one pair of [2][n] ciphertexts of raw words."""
    a0, a1 = ([lift(int(x), q) for x in row] for row in ct1)
    b0, b1 = ([lift(int(x), q) for x in row] for row in ct2)
    x1 = [u + v for u, v in zip(ring_mul(a0, b1), ring_mul(a1, b0))]
    return [ring_mul(a0, b0), x1, ring_mul(a1, b1)]


def scale_rows(X, q, t):
    return [[rnd(t * x, q) % q for x in row] for row in X]


def multiply_scaled(ct1, ct2, q, t):
    return scale_rows(tensor(ct1, ct2, q), q, t)


def dot_scaled(a, b, q, t):
    """One rescale after the sum over the pairs of one group."""
    acc = None
    for x, y in zip(a, b):
        X = tensor(x, y, q)
        acc = X if acc is None else [[u + v for u, v in zip(r, s)] for r, s in zip(acc, X)]
    return scale_rows(acc, q, t)


def sub_ct(ct, ref, q):
    return [[(int(x) % q - int(y) % q) % q for x, y in zip(r, s)] for r, s in zip(ct, ref)]


def square_scaled(ct, ref, q, t):
    d = ct if ref is None else sub_ct(ct, ref, q)
    return multiply_scaled(d, d, q, t)


def max_count(n, q, t, p1, p2):
    return (p1 * p2 - 1) // (t * n * q)


def max_t(n, q, p1, p2):
    """The largest plaintext modulus the bound allows at count 1."""
    return min(q - 1, (p1 * p2 - 1) // (n * q))


def three_channel(xq, x1, x2, q, t, p1, p2):
    """rnd(t X) mod q from the three residues, in single-word modular steps."""
    c = centred(t * xq % q, q)
    y1 = (t * x1 - c) * pow(q, -1, p1) % p1
    y2 = (t * x2 - c) * pow(q, -1, p2) % p2
    v = (y2 - y1) * pow(p1, -1, p2) % p2
    y = y1 + p1 * v
    neg = y > (p1 * p2 - 1) // 2
    return (y1 + (p1 % q) * v - (p1 * p2 % q if neg else 0)) % q


def edge_values(q, t, p1, p2, count=24, seed=0):
    """Integers X for the scale-and-round step: 0, +-1, t X mod q on either
    side of q/2 (both signs), |rnd(t X)| at the bound p1 p2 / 2, and random
    values of every size up to it."""
    bound = (p1 * p2 - 1) // 2          # |y| <= bound
    xmax = (bound * q) // t - q         # t xmax / q <= bound - 1
    xs = [0, 1, -1, xmax, -xmax, xmax - 1, 1 - xmax]
    # rnd(t X) = +-bound exactly: a multiple of t within (q - 1) / 2 of bound q (t < q: one exists)
    xb = -(-(bound * q - (q - 1) // 2) // t)
    if rnd(t * xb, q) == bound:
        xs += [xb, -xb]
    tinv = pow(t, -1, q) if _coprime(t, q) else None
    if tinv is not None:
        for r in ((q - 1) // 2, (q + 1) // 2):
            x0 = r * tinv % q
            xs += [x0, x0 - q, x0 + q * (xmax // (2 * q)), x0 - q * (xmax // (2 * q))]
    rng = random.Random((q, t, seed).__hash__())
    for i in range(count):
        bits = 1 + (i * xmax.bit_length()) // count
        x = rng.getrandbits(bits) % (xmax + 1)
        xs.append(x if i % 2 else -x)
    assert all(abs(rnd(t * x, q)) <= bound for x in xs)
    return xs


def _coprime(a, b):
    while b:
        a, b = b, a % b
    return a == 1


# ---------------------------------------------------------------- meaning (BFV with real keys)
def sample_ternary(rng, n):
    return [rng.randrange(-1, 2) for _ in range(n)]


def sample_gauss(rng, n, sigma=3.2):
    return [int(round(rng.gauss(0, sigma))) for _ in range(n)]


def polymod(a, q):
    return [x % q for x in a]


def keygen(rng, n, q):
    s = sample_ternary(rng, n)
    a = [rng.randrange(q) for _ in range(n)]
    e = sample_gauss(rng, n)
    b = [(x + y) % q for x, y in zip(negacyclic(a, s) if n < 256 else negacyclic_kron(a, s), e)]
    return s, (a, b)  # b = a s + e: phase c0 - c1 s


def encrypt(rng, m, pk, q, t):
    a, b = pk
    n = len(a)
    delta = q // t
    u, e1, e2 = sample_ternary(rng, n), sample_gauss(rng, n), sample_gauss(rng, n)
    c0 = [(x + y + delta * (mi % t)) % q for x, y, mi in zip(ring_mul(b, u), e1, m)]
    c1 = [(x + y) % q for x, y in zip(ring_mul(a, u), e2)]
    return [c0, c1]


def phase3(ct3, s, q):
    """c0 - c1 s + c2 s^2 mod q, centred."""
    s2 = ring_mul(s, s)
    c1s = ring_mul([lift(x, q) for x in ct3[1]], s)
    c2s = ring_mul([lift(x, q) for x in ct3[2]], s2)
    return [lift(x - y + z, q) for x, y, z in zip(ct3[0], c1s, c2s)]


def phase2(ct, s, q):
    c1s = ring_mul([lift(int(x), q) for x in ct[1]], s)
    return [lift(int(x) - y, q) for x, y in zip(ct[0], c1s)]


def decode(phase, q, t):
    return [((p % q) * t + q // 2) // q % t for p in phase]


def noise(phase, m, q, t):
    """Largest |phase - Delta m| over the coefficients (m reduced mod t)."""
    delta = q // t
    return max(abs(lift(p - delta * (mi % t), q)) for p, mi in zip(phase, m))


def plain_product(m1, m2, t):
    return [x % t for x in ring_mul(list(m1), list(m2))]


def relin_key(rng, s, q, base_log, level):
    """rlk[l] = (a_l, b_l) with b_l = a_l s + e_l + 2^(l base_log) s^2: the
    layout of fhe_eval_key_generate (unsigned LSB-first digits of c2)."""
    n = len(s)
    s2 = ring_mul(s, s)
    key = []
    for l in range(level):
        a = [rng.randrange(q) for _ in range(n)]
        e = sample_gauss(rng, n)
        b = [(x + y + (z << (l * base_log))) % q for x, y, z in zip(ring_mul(a, s), e, s2)]
        key.append((a, b))
    return key


def relinearize(ct3, key, q, base_log):
    """c0 + sum_l d_l b_l, c1 + sum_l d_l a_l with d_l the base-2^base_log
    digits of c2 (phase c0 - c1 s gains + c2 s^2 + sum d_l e_l)."""
    n = len(ct3[0])
    mask = (1 << base_log) - 1
    c0, c1 = list(ct3[0]), list(ct3[1])
    for l, (a, b) in enumerate(key):
        d = [(x >> (l * base_log)) & mask for x in ct3[2]]
        c0 = [(x + y) % q for x, y in zip(c0, ring_mul(d, b))]
        c1 = [(x + y) % q for x, y in zip(c1, ring_mul(d, a))]
    assert base_log * len(key) >= (q - 1).bit_length() and n
    return [c0, c1]
