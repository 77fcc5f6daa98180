"""Independent big-integer restatement (TEST INFRASTRUCTURE ONLY).

A second, independently written oracle used to cross-check ``ref_cpu.c``.  It
follows the reference's own TypeScript restatement of the C++ transform,
``src/test-utils/ntt-round-trip.prop.test.ts:156-244`` (forward Cooley-Tukey
with twiddle ``psi^(j*n/groupSize)`` after a bit-reversal, inverse
Gentleman-Sande + bit-reversal + N^-1), its primitive-root search
(``findPrimitiveRoot``) and the negacyclic reference of
``src/test-utils/homomorphic-multiplication.prop.test.ts:126-189`` / schoolbook
convolution.  Pure Python ints: only for small cases.

``negacyclic_multiply`` is a third, transform-free route to the ring product
(one big-integer multiplication), fast enough for n = 16384.

``decompose`` .. ``blind_rotate`` restate the TFHE pieces of BootstrapEngine
over a ring product passed in, with an explicit LWE modulus: the shared
reference of the CPU checks of ``ref_cpu.c`` (compat product) and of the GPU
tests of negacyclic blind rotation (true ring product).  ``sample_extract``,
``key_switch`` (which also counts the updates that wrap past 2^64) and
``lwe_decrypt`` restate the LWE side the same way.  ``decode_noise``,
``ggsw_gadget``, ``ggsw_encrypt`` and ``ksk_body`` restate the decode epilogue
of the BFV decryptions and the key generation with their u64 / int64 wraps.
"""
from __future__ import annotations


def mod_pow(b, e, m):
    return pow(b, e, m)


def find_psi(n, q):
    two_n = 2 * n
    if (q - 1) % two_n:
        raise ValueError("not NTT-friendly")
    e = (q - 1) // two_n
    g = 2
    while g < q:
        w = pow(g, e, q)
        if pow(w, two_n, q) == 1 and pow(w, n, q) == q - 1:
            return w
        g += 1
    raise ValueError("no root")


def bitrev(i, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (i & 1)
        i >>= 1
    return r


def _bitrev_perm(a):
    n = len(a)
    bits = n.bit_length() - 1
    return [a[bitrev(i, bits)] for i in range(n)]


def forward(coeffs, q):
    n = len(coeffs)
    logn = n.bit_length() - 1
    psi = find_psi(n, q)
    tw = [pow(psi, i, q) for i in range(n)]
    r = _bitrev_perm([c % q for c in coeffs])
    for s in range(logn):
        m = 1 << s
        gs = 2 * m
        for k in range(0, n, gs):
            for j in range(m):
                w = tw[j * (n // gs)]
                a, b = r[k + j], r[k + j + m]
                wb = (w * b) % q
                r[k + j] = (a + wb) % q
                r[k + j + m] = (a - wb) % q
    return r


def inverse(coeffs, q):
    n = len(coeffs)
    logn = n.bit_length() - 1
    psi = find_psi(n, q)
    pinv = pow(psi, -1, q)
    tw = [pow(pinv, i, q) for i in range(n)]
    r = [c % q for c in coeffs]
    for s in range(logn - 1, -1, -1):
        m = 1 << s
        gs = 2 * m
        for k in range(0, n, gs):
            for j in range(m):
                w = tw[j * (n // gs)]
                a, b = r[k + j], r[k + j + m]
                r[k + j] = (a + b) % q
                r[k + j + m] = ((a - b) * w) % q
    r = _bitrev_perm(r)
    ninv = pow(n, -1, q)
    return [(c * ninv) % q for c in r]


def polymul(a, b, q):
    fa, fb = forward(a, q), forward(b, q)
    return inverse([(x * y) % q for x, y in zip(fa, fb)], q)


def negacyclic_schoolbook(a, b, q):
    n = len(a)
    c = [0] * n
    for i in range(n):
        for j in range(n):
            k = i + j
            if k < n:
                c[k] = (c[k] + a[i] * b[j]) % q
            else:
                c[k - n] = (c[k - n] - a[i] * b[j]) % q
    return c


def negacyclic_multiply(a, b, q):
    """a * b mod (X^n + 1, q), exact, by Kronecker substitution: the
    coefficients (any integers, read mod q) are packed into one Python integer
    each, in slots wide enough for a coefficient of the plain product
    (< n (q-1)^2, so 2 bits(q-1) + bits(n) bits, rounded up to bytes); one
    big-integer product gives the 2n-1 plain coefficients c, and X^n = -1
    folds them to c[i] - c[i+n].  Shares nothing with the transforms above:
    no root of unity, no twiddle table, no butterfly."""
    n = len(a)
    if len(b) != n:
        raise ValueError("operand lengths differ")
    slot = (2 * (q - 1).bit_length() + n.bit_length() + 7) // 8

    def pack(p):
        return int.from_bytes(b"".join((int(c) % q).to_bytes(slot, "little") for c in p), "little")

    prod = (pack(a) * pack(b)).to_bytes(2 * n * slot, "little")
    c = [int.from_bytes(prod[i * slot:(i + 1) * slot], "little") for i in range(2 * n)]
    return [(c[i] - c[i + n]) % q for i in range(n)]


def negacyclic_forward(coeffs, q):
    """homomorphic-multiplication.prop.test.ts:126-189: twist by psi^i, then a
    cyclic DIT with omega = psi^2 (bit-reversed input, natural output)."""
    n = len(coeffs)
    logn = n.bit_length() - 1
    psi = find_psi(n, q)
    omega = psi * psi % q
    r = [(c % q) * pow(psi, i, q) % q for i, c in enumerate(coeffs)]
    r = _bitrev_perm(r)
    for s in range(logn):
        m = 1 << s
        gs = 2 * m
        wm = pow(omega, n // gs, q)
        for k in range(0, n, gs):
            w = 1
            for j in range(m):
                a, b = r[k + j], r[k + j + m] * w % q
                r[k + j] = (a + b) % q
                r[k + j + m] = (a - b) % q
                w = w * wm % q
    return r


def negacyclic_inverse(vals, q):
    n = len(vals)
    logn = n.bit_length() - 1
    psi = find_psi(n, q)
    omega_inv = pow(psi * psi % q, -1, q)
    r = _bitrev_perm([v % q for v in vals])
    for s in range(logn):
        m = 1 << s
        gs = 2 * m
        wm = pow(omega_inv, n // gs, q)
        for k in range(0, n, gs):
            w = 1
            for j in range(m):
                a, b = r[k + j], r[k + j + m] * w % q
                r[k + j] = (a + b) % q
                r[k + j + m] = (a - b) % q
                w = w * wm % q
    ninv = pow(n, -1, q)
    pinv = pow(psi, -1, q)
    return [r[i] * ninv % q * pow(pinv, i, q) % q for i in range(n)]


# ---------------------------------------------------------------- TFHE pieces
# BootstrapEngine's decompose / external_product / rotate_polynomial / cmux /
# blind_rotate (bootstrap_engine.cpp:122-185, 431-577) restated over Python
# integers.  The ring product is a parameter ``mul(a, b, q)``: ``polymul``
# gives the reference's (compat) product inv(fwd(a) . fwd(b)),
# ``negacyclic_multiply`` the true product mod X^n + 1.  Sums and differences
# are plain ``% q`` (ModularArithmetic::mod_add / mod_sub reduce their
# operands first, so they are the same function).  u64 words wrap where the
# reference's wrap: the rotation amount and the negation of a raw coefficient.
M64 = (1 << 64) - 1


def c_int32_trunc(x):
    """(int32_t)(uint32_t)x"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def rot_amount(a, n, lwe_q):
    """blind_rotate's rotation amount (:560): (int32)((a * 2N + lwe_q / 2) /
    lwe_q) in u64 arithmetic -- the product wraps at 2^64 and so does the
    sum; a is used raw (not reduced mod lwe_q)."""
    s = (((int(a) * 2 * n) & M64) + lwe_q // 2) & M64
    return c_int32_trunc(s // lwe_q)


def decompose(poly, q, bl, lv):
    """decompose (:152-185): signed digits of the raw word, most significant
    level first, a negative digit d - B stored as (q - (B - d)) % q in u64
    arithmetic: below q = B - d the difference wraps at 2^64 before it is
    reduced, so the word is off the centred digit by 2^64 mod q."""
    base = 1 << bl
    out = []
    for l in range(lv):
        sh = (lv - 1 - l) * bl
        row = []
        for c in poly:
            d = (int(c) >> sh) & (base - 1)
            row.append(((q - (base - d)) & M64) % q if d > base // 2 else d)
        out.append(row)
    return out


def external_product(glwe, ggsw, q, bl, lv, k=1, mul=polymul):
    """external_product (:431-518): out_j = sum over the rows (i, l) of
    digit_l(glwe_i) * ggsw[i lv + l][j]; glwe [k+1][n], ggsw [(k+1) lv][k+1][n]."""
    n = len(glwe[0])
    res = [[0] * n for _ in range(k + 1)]
    row = 0
    for i in range(k + 1):
        for d in decompose(glwe[i], q, bl, lv):
            for j in range(k + 1):
                p = mul(d, [int(v) for v in ggsw[row][j]], q)
                res[j] = [(a + b) % q for a, b in zip(res[j], p)]
            row += 1
    return res


def rotate(poly, rot, q):
    """rotate_polynomial (:122-145): X^rot * poly mod X^n + 1, rot any int32.
    A coefficient that keeps its sign is copied raw; one that crosses X^n
    becomes ((q - c) mod 2^64) % q."""
    n = len(poly)
    two_n = 2 * n
    r = c_int32_trunc(rot) % two_n  # same residue as C's ((rot % 2N) + 2N) % 2N
    out = [0] * n
    for i, c in enumerate(poly):
        ni = (i + r) % two_n
        if ni < n:
            out[ni] = int(c)
        else:
            out[ni - n] = ((q - int(c)) & M64) % q
    return out


def cmux(ggsw, ct0, ct1, q, bl, lv, k=1, mul=polymul):
    """cmux (:520-540): ct0 + ggsw (x) (ct1 - ct0)."""
    diff = [[(int(a) - int(b)) % q for a, b in zip(ct1[i], ct0[i])] for i in range(k + 1)]
    p = external_product(diff, ggsw, q, bl, lv, k, mul)
    return [[(a + int(b)) % q for a, b in zip(p[i], ct0[i])] for i in range(k + 1)]


def blind_rotate(acc, lwe_a, lwe_b, lwe_q, bsk, q, bl, lv, k=1, mul=polymul):
    """blind_rotate (:547-577): acc <- X^-rot(b) acc, then for every mask word
    with a non-zero amount acc <- cmux(bsk[i], acc, X^rot(a_i) acc).  Amount
    0 skips the step (the accumulator keeps its raw words); any other amount,
    a non-zero multiple of 2N included, computes it."""
    n = len(acc[0])
    acc = [[int(v) for v in p] for p in acc]
    b_rot = -rot_amount(lwe_b, n, lwe_q)
    acc = [rotate(p, b_rot, q) for p in acc]
    for i, a in enumerate(lwe_a):
        a_rot = rot_amount(a, n, lwe_q)
        if a_rot == 0:
            continue
        rot = [rotate(p, a_rot, q) for p in acc]
        acc = cmux(bsk[i], acc, rot, q, bl, lv, k, mul)
    return acc


def sample_extract(glwe, q):
    """sample_extract (:594-624) of glwe [k+1][n] -> (a [k n], b): a[i n] =
    mask_i[0] and the body b = body[0] are copied raw; a[i n + j] =
    ((q - mask_i[n - j]) mod 2^64) % q for j > 0 (:616)."""
    k, n = len(glwe) - 1, len(glwe[0])
    a = []
    for i in range(k):
        m = [int(v) for v in glwe[i]]
        a.append(m[0])
        a.extend(((q - m[n - j]) & M64) % q for j in range(1, n))
    return a, int(glwe[k][0])


def key_switch(ksk_a, ksk_b, lwe_a, lwe_b, q, bl, lv, out_dim=None, skip_first_body=False):
    """key_switch (:626-674) -> (a [out_dim], b, mask_wraps, body_wraps).

    ksk_a [in_dim lv][out_dim], ksk_b [in_dim lv], entry i lv + l.  Digit
    (coeff >> (lv - 1 - l) bl) & (B - 1) of the raw mask word (:649-650); a
    zero digit skips its entry (:652-655); every other one updates
      a[j] = (a[j] + q - (digit * key_a[j]) % q) % q        (:661)
      b    = (b    + q - (digit * key_b)    % q) % q        (:664)
    in u64 arithmetic: the product wraps at 2^64, and so does the sum
    r + q - term, which passes 2^64 only when q > 2^63 or when r is the raw
    body (>= q) in its first update.  The body starts as the raw lwe_b (:640)
    and is returned raw when every digit is zero.

    mask_wraps / body_wraps count the updates whose sum passed 2^64;
    skip_first_body leaves the first body update (the one that meets the raw
    body) out of body_wraps.  out_dim is only needed without key rows."""
    if out_dim is None:
        out_dim = len(ksk_a[0])
    mask = (1 << bl) - 1
    ra, rb = [0] * out_dim, int(lwe_b)
    mask_wraps = body_wraps = 0
    first = True
    idx = 0
    for c in lwe_a:
        c = int(c)
        for l in range(lv):
            d = (c >> ((lv - 1 - l) * bl)) & mask
            if d == 0:
                idx += 1
                continue
            row = ksk_a[idx] if out_dim else ()
            for j in range(out_dim):
                s = ra[j] + q - ((d * int(row[j])) & M64) % q
                mask_wraps += s > M64
                ra[j] = (s & M64) % q
            s = rb + q - ((d * int(ksk_b[idx])) & M64) % q
            if not (first and skip_first_body):
                body_wraps += s > M64
            first = False
            rb = (s & M64) % q
            idx += 1
    return ra, rb, mask_wraps, body_wraps


def lwe_decrypt(sk, lwe_a, lwe_b, q, t):
    """The library's LWE decryption (include/fhe_gpu.h, fhe_lwe_decrypt_batch)
    -> (value, phase): phase = b - sum_j a_j s_j mod q over the integers (s_j
    any int64, a_j and b raw words), value = ((phase t + q / 2) / q) % t with
    decode_plaintext's 128-bit numerator (encryption.cpp:136-149: nothing
    wraps) and its t == 0 -> 4 (:138)."""
    t = t if t else 4
    p = (int(lwe_b) - sum(int(a) * int(s) for a, s in zip(lwe_a, sk))) % q
    return ((p * t + q // 2) // q) % t, p


# ---------------------------------------------------------------- decode / key material
# EncryptionEngine's decode + noise measure and the closed forms of
# BootstrapEngine's key generation, with the reference's u64 / int64
# wrap-around spelled out: the second reference of tests/test_engine_edges.py.
def _i64(x):
    """(int64_t)x of a wrapped 64-bit word."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def decode_noise(p, q, t):
    """decode_packed (encryption.cpp:150-163) and the distance of
    compute_noise_budget (:364-400) for a canonical phase p < q -> (value,
    |noise|).  rounded = (p t + q / 2) / q over a 128-bit numerator (nothing
    wraps); expected = (rounded delta) % q with the u64 product; the distance
    is an int64: wrapped to q - noise above q / 2, where (int64_t)q is
    negative for q >= 2^63 (the sign flip), then |.| taken."""
    t = t if t else 4
    delta = q // t
    r = (p * t + q // 2) // q
    expected = ((r * delta) & M64) % q
    noise = _i64(p - expected if p >= expected else expected - p)
    if noise > _i64(q // 2):
        noise = _i64(_i64(q) - noise)
    return r % t, (-noise if noise < 0 else noise) & M64


def ggsw_gadget(v, q, l, base_log):
    """encrypt_ggsw's gadget term (bootstrap_engine.cpp:287-291): (|v| q) >>
    ((l + 1) base_log) with the u64 product and the shift count taken mod 64;
    for v < 0 it is (q - g) % q with the subtraction in u64 -- for g > q that
    wraps and is not the residue of -g."""
    av = (-v if v < 0 else v) & M64  # |INT64_MIN| = 2^63 as a u64
    g = ((av * q) & M64) >> (((l + 1) * base_log) & 63)
    return ((q - g) & M64) % q if v < 0 else g


def ksk_body(a_row, lwe_sk, err, glwe_word, q, l, base_log):
    """One body word of generate_key_switch_key (:367-420): the int64 inner
    product of the mask row with the LWE key (wrapping), plus the centred
    error (err > q / 2 reads as err - q, both as int64), reduced with C's
    truncating % by (int64_t)q -- negative for q >= 2^63 -- then the gadget
    (glwe_word q) >> ((l + 1) base_log) added in u64 and % q."""
    ip = sum(int(a) * int(s) for a, s in zip(a_row, lwe_sk)) & M64
    ev = _i64(err)
    if ev > _i64(q // 2):
        ev = _i64(ev - _i64(q))
    s = _i64(ip + ev)
    qi = _i64(q)
    rem = abs(s) % abs(qi)
    rem = -rem if s < 0 else rem  # C: the remainder takes the dividend's sign
    gadget = ((int(glwe_word) * q) & M64) >> (((l + 1) * base_log) & 63)
    return (((rem & M64) + gadget) & M64) % q


def compat_polymul(a, b, q):
    """The ring product as the reference's transforms compute it: polymul
    below 2^63.  From 2^63 on the signed extended Euclid of
    ntt_processor.cpp:64-90 reads the modulus as a negative int64 and returns
    N^-1 = 0, so every inverse transform, and with it every product, is 0."""
    return polymul(a, b, q) if q < 1 << 63 else [0] * len(a)


def ggsw_encrypt(values, sk, masks, err, q, k, base_log, level, mul=compat_polymul):
    """encrypt_ggsw (:268-306) over given draws -> [count][(k+1) level][k+1][n]
    as nested lists.  masks [rows][k][n] and err [rows][n] are the uniform and
    the error draws of the rows (row = c (k+1) level + grp level + l); body =
    sum_i mask_i * sk + err (encrypt_glwe_zero, :190-227), then the gadget
    added to coefficient 0 of mask[grp] (grp < k) or of the body."""
    n = len(sk)
    sk = [int(x) for x in sk]
    per = (k + 1) * level
    out = []
    for c, v in enumerate(values):
        ct = []
        for rr in range(per):
            r = c * per + rr
            grp, l = divmod(rr, level)
            row = [[int(x) for x in masks[r][i]] for i in range(k)]
            body = [0] * n
            for i in range(k):
                body = [(x + y) % q for x, y in zip(body, mul(row[i], sk, q))]
            body = [(x + int(e)) % q for x, e in zip(body, err[r])]
            g = ggsw_gadget(int(v), q, l, base_log)
            if grp < k:
                row[grp][0] = ((row[grp][0] + g) & M64) % q
            else:
                body[0] = ((body[0] + g) & M64) % q
            ct.append(row + [body])
        out.append(ct)
    return out
