"""Python-integer restatement of the exact ring product over moduli without a CRT basis (lolhip_ringmul_*,
include/lolhip.h): the powerful-basis product of Z[zeta_m] reduced mod q, the growth constant C_m, the exactness bound
2 C_m H^2 and the rule that chooses the default NTT primes.  Object arrays and Python integers throughout: no int64
ceiling anywhere.  Since the device's product is exact over the integers, its result mod q_t does not depend on the
representative an operand coefficient is lifted to: the oracle multiplies the canonical residues."""
import functools
import math

import numpy as np

import crtset_ref as cr
from oracle import lolmath as lm


# ---- the growth constant ------------------------------------------------------------------------------------------------
def growth_pp(p, e):
    """max_k sum_{i,j} |(z^i z^j)_k| over the powerful basis z^0 .. z^(phi-1) of index p^e: pairs (i, j) by their
    exponent sum t (a convolution of two all-ones rows), z^t folded through z^(p^e) = 1 and
    z^(phi + r) = -sum_{l < p-1} z^(l p^(e-1) + r)."""
    pk, pk1 = p ** e, p ** (e - 1)
    phi = pk - pk1
    pairs = np.convolve(np.ones(phi, dtype=np.int64), np.ones(phi, dtype=np.int64))
    acc = np.zeros(phi, dtype=np.int64)
    for t, c in enumerate(pairs):
        tt = t % pk
        if tt < phi:
            acc[tt] += c
        else:
            acc[(tt - phi) % pk1::pk1] += c
    return int(acc.max())


def growth(m):
    """C_m: the product over the prime powers of m (the powerful basis is their tensor product)"""
    return math.prod(growth_pp(p, e) for p, e in lm.factor_pps(m))


def growth_by_definition(m):
    """C_m straight from the definition, through the full product table of a small index"""
    R = cr.ring(m)
    tot = np.zeros(R.n, dtype=np.int64)
    for i in range(R.n):
        tot += np.abs(R.red[(R.expo[i] + R.expo) % m]).sum(axis=0)
    return int(tot.max())


# ---- the bound and the moduli rule --------------------------------------------------------------------------------------
def bound(m, qs):
    """2 C_m H^2, H = max_t floor(q_t / 2): the product of the NTT primes must exceed it"""
    H = max(int(q) // 2 for q in qs)
    return 2 * growth(m) * H * H


def root_up(x, k):
    """the smallest r with r^k >= x"""
    lo, hi = 0, 1
    while hi ** k < x:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid ** k < x else (lo, mid)
    return hi


def moduli(m, qs):
    """The default primes: for K = 1, 2, 3 the K consecutive primes = 1 mod m above the K-th root (rounded up) of the
    bound; the first K whose primes all lie below 2^61.  None when no K serves."""
    b = bound(m, qs)
    for K in (1, 2, 3):
        r = root_up(b, K)
        if r >= 2 ** 61:
            continue
        g = lm.good_qs(m, r)
        Qs = [next(g) for _ in range(K)]
        while math.prod(Qs) <= b:                       # never taken: every prime exceeds r
            Qs = Qs[1:] + [next(g)]
        if all(Q < 2 ** 61 for Q in Qs):
            return Qs
    return None


def accepts(m, qs, Qs):
    return len(set(Qs)) == len(Qs) and bound(m, qs) < math.prod(Qs)


# prime sets at whose bound create and the fold are probed: m = 16 with tiny primes for K = 2 and 3, and one
# index that is not a power of two
BOUNDARY = [(16, (65537,)), (16, (193, 257)), (16, (17, 97, 113)), (9, (73, 109, 127))]


@functools.lru_cache(maxsize=None)
def boundary_pair(m, Qs, odd):
    """(q accepted, q rejected) of the given parity for the prime set Qs: the largest q with 2 C_m floor(q/2)^2 below
    prod Qs and the next one of its parity, together with how close the accepted bound comes to prod Qs"""
    P, C = math.prod(Qs), growth(m)
    H = math.isqrt((P - 1) // (2 * C))
    assert 2 * C * H * H < P <= 2 * C * (H + 1) ** 2
    q = 2 * H + (1 if odd else 0)
    return q, q + 2, 2 * C * H * H / P


# ---- the product --------------------------------------------------------------------------------------------------------
def mul_int(m, a, b):
    """a * b over the integers, powerful basis of index m: a, b [n] sequences of Python integers -> [n] object array"""
    R = cr.ring(m)
    a, b = np.array(list(a), dtype=object), np.array(list(b), dtype=object)
    by_expo = np.zeros(m, dtype=object)
    for i in range(R.n):
        if a[i]:
            by_expo[(R.expo[i] + R.expo) % m] += a[i] * b            # the exponents of a basis are distinct mod m
    return by_expo.dot(R.red.astype(object))


def mul(m, a, b, qs):
    """a * b in R_q: a, b [B][n][T] of any integers -> [B][n][T] int64 residues in [0, q_t)"""
    a, b = np.asarray(a), np.asarray(b)
    B, n, T = a.shape
    out = np.zeros((B, n, T), dtype=np.int64)
    for r in range(B):
        for t, q in enumerate(qs):
            q = int(q)
            c = mul_int(m, [int(x) % q for x in a[r, :, t]], [int(x) % q for x in b[r, :, t]])
            out[r, :, t] = [int(x) % q for x in c]
    return out


def negacyclic_kronecker(a, b, q):
    """a * b in Z_q[x] / (x^n + 1) (the powerful basis of a two-power index 2n) by Kronecker substitution: the
    coefficients packed into one Python integer each, one integer product, unpacked and folded through x^n = -1"""
    q, n = int(q), len(a)
    a, b = [int(x) % q for x in a], [int(x) % q for x in b]
    nbytes = (2 * q.bit_length() + n.bit_length() + 8) // 8
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(nbytes, "little") for x in v), "little")
    raw = (pack(a) * pack(b)).to_bytes(2 * n * nbytes, "little")
    d = [int.from_bytes(raw[i * nbytes:(i + 1) * nbytes], "little") for i in range(2 * n)]
    return np.array([(d[k] - d[k + n]) % q for k in range(n)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def pow2_expo(m):
    """expo[j]: the powerful basis of a two-power index holds zeta^expo[j] at position j (a bit reversal)"""
    pe = lm.factor_pps(m)[0]
    assert pe[0] == 2 and pe[0] ** pe[1] == m
    return np.array([lm.index_to_pow(pe, j) for j in range(m // 2)], dtype=np.int64)


def mul_pow2(m, a, b, q):
    """a * b in R_q for one element of a two-power index, powerful basis in and out, through the Kronecker product"""
    expo = pow2_expo(m)
    x, y = np.zeros(m // 2, dtype=object), np.zeros(m // 2, dtype=object)
    x[expo], y[expo] = [int(v) for v in a], [int(v) for v in b]
    return negacyclic_kronecker(x, y, q)[expo]
