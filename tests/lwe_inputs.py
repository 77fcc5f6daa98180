"""LWE masks for blind-rotation tests that reach every kind of rotation.

With ``lwe_q`` near 2^62 the reference's rotation amount
``(int32)((a * 2N + lwe_q / 2) / lwe_q)`` (u64 arithmetic, the product wraps)
of a uniform mask word is 0..4, so the wrap branch of the rotation, a rotation
by 2N and the int32 truncation are hardly reached.  The words below are built
for a given (N, lwe_q), and ``classes`` names what a set of masks reaches;
the amounts come from ``oracle.pyref.rot_amount``, never from the library
under test.  Used by the CPU checks of the restatements and by the GPU tests.
"""
import numpy as np

import oracle
from oracle import pyref

M64 = (1 << 64) - 1
INT32_MIN = -(1 << 31)
LWE_QS = {"2^32": 1 << 32, "4N": None, "257": 257, "P27": 132120577}  # 4N: filled in per degree


def lwe_modulus(name, n):
    return 4 * n if name == "4N" else LWE_QS[name]


def words(n, lwe_q):
    """Mask words by the kind of step they give (lwe_q <= 2^32, so that none
    of the products below wraps)."""
    return {
        "zero": 0,                       # amount 0: the step is skipped
        "top": lwe_q - 1,                # amount exactly 2N when lwe_q >= 4N: computed, not skipped
        "low": lwe_q // 8,               # amount in (0, N)
        "high": 5 * lwe_q // 8,          # amount in (N, 2N): every coefficient past N - amount changes sign twice
        "multiple": 3 * lwe_q,           # raw word >= lwe_q; amount 6N, a non-zero multiple of 2N
        "negative": ((1 << 31) * lwe_q) // (2 * n) + lwe_q // 3,  # amount 2^31 + about 2N/3: a negative int32
        "raw": M64,                      # product and sum both wrap
    }


def planted(n, lwe_q, dim):
    """The first `dim` of the words above, the ones a small lwe_q needs first."""
    w = words(n, lwe_q)
    order = ["zero", "top", "low", "high", "multiple"] + (["negative", "raw"] if lwe_q < 2 * n else ["raw", "negative"])
    return [w[x] for x in order[:dim]]


def masks(seed, n, lwe_q, batch, dim):
    """[batch][dim] mask words below lwe_q; row 0 starts with the planted
    words, row 1 (if any) is all zero: every step skipped; row 2 (if any)
    alternates lwe_q, 2 lwe_q, .. with zeros: its only steps rotate by
    multiples of 2N, so all they do is reduce the accumulator's raw words --
    a kernel that skipped them would hand the raw words back."""
    a = oracle.splitmix_fill(seed, lwe_q, batch * dim).reshape(batch, dim)
    p = planted(n, lwe_q, dim)
    a[0, :len(p)] = p
    if batch > 1:
        a[1, :] = 0
    if batch > 2:
        a[2, :] = identity_steps(lwe_q, dim)
    return a


def identity_steps(lwe_q, dim):
    """lwe_q, 0, 2 lwe_q, 0, ..: amounts 2N, 0, 4N, 0, .."""
    return [(i // 2 + 1) * lwe_q if i % 2 == 0 else 0 for i in range(dim)]


def bodies(seed, n, lwe_q, batch):
    """Bodies below lwe_q, the last one a raw 2^64 - 1.  No body's amount is
    INT32_MIN, whose negation the reference leaves undefined."""
    b = oracle.splitmix_fill(seed, lwe_q, batch)
    b[batch - 1] = M64
    assert all(pyref.rot_amount(int(v), n, lwe_q) != INT32_MIN for v in b)
    return b


def amounts(n, lwe_q, lwe_a):
    return [[pyref.rot_amount(int(v), n, lwe_q) for v in row] for row in np.asarray(lwe_a).reshape(-1, lwe_a.shape[-1])]


def classes(n, lwe_q, lwe_a):
    """The kinds of step and of ciphertext in lwe_a [batch][dim]."""
    two_n = 2 * n
    rows = amounts(n, lwe_q, lwe_a)
    flat = [r for row in rows for r in row]
    got = set()
    if any(r == 0 for r in flat):
        got.add("skipped step")
    if any(r == two_n for r in flat):
        got.add("amount 2N")
    if any(0 < r < n for r in flat):
        got.add("amount in (0, N)")
    if any(n < r < two_n for r in flat):
        got.add("amount in (N, 2N)")
    if any(r < 0 for r in flat):
        got.add("negative amount")
    if any(r != 0 and r % two_n == 0 for r in flat):
        got.add("non-zero multiple of 2N")
    if any(int(v) >= lwe_q for v in np.asarray(lwe_a).ravel()):
        got.add("raw word")
    if any(all(r == 0 for r in row) for row in rows):
        got.add("skipped ciphertext")
    if any(any(row) and all(r % two_n == 0 for r in row) for row in rows):
        got.add("identity-only ciphertext")
    return got


def required(n, lwe_q):
    need = {"skipped step", "amount in (0, N)", "amount in (N, 2N)", "raw word", "skipped ciphertext",
            "non-zero multiple of 2N", "identity-only ciphertext"}
    if lwe_q >= 4 * n:
        need.add("amount 2N")
    if lwe_q < 2 * n:
        need.add("negative amount")
    return need


def executed(n, lwe_q, lwe_a):
    """(steps executed, steps) over the ciphertexts that are not wholly skipped."""
    rows = [row for row in amounts(n, lwe_q, lwe_a) if any(r != 0 for r in row)]
    return sum(r != 0 for row in rows for r in row), sum(len(row) for row in rows)


def check_coverage(n, lwe_q, lwe_a):
    """Fails when the masks do not reach every class that applies to lwe_q, or
    when fewer than half of the steps of the live ciphertexts are executed."""
    missing = required(n, lwe_q) - classes(n, lwe_q, lwe_a)
    assert not missing, (n, lwe_q, sorted(missing))
    done, total = executed(n, lwe_q, lwe_a)
    assert 2 * done >= total > 0, (n, lwe_q, done, total)
