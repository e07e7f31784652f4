"""Inputs that drive the lazy accumulators of the SymmSHE pipeline kernels to their bound (helpers of
test_saturation_host.py and test_saturation.py).

The pipeline kernels add raw products into a wide accumulator and reduce every few terms; each interval rests on an
inequality that is tightest at the largest modulus of the arithmetic class and for residues q - 1.  The digits of a key
switch are produced inside the kernel, so a test chooses c2:

    v = -(b^k - 1) / (b - 1),  k = gadlen(b, q)

has every centred base-b digit equal to -1, "what is left" (the last digit) included, provided v is the centred lift of
its residue: 2 |v| <= q - 1.  With v mod q_t in coefficient 0 of component t and 0 elsewhere, every digit polynomial is
the constant -1, whose CRT is q_s - 1 at every slot of every target component.  A hint of q_s - 1 everywhere then makes
every raw product (q_s - 1)^2, and the switched value is L mod q_s at every slot: a closed form without a transform.

Edge of the construction ((q, base) pairs without an all-(-1) value; all_minus_one returns None):
    base 2 and 3, always     |v| = 2^k - 1 resp. (3^k - 1) / 2 is above q / 2 because q < b^k
    base 4 below 2^29        the primes just below 2^29 have k = 15 and |v| = (4^15 - 1) / 3 > q / 2; the same just
                             below 2^27, 2^31 and 2^61 (base 4 works just below 2^30, 2^32 and 2^62)
    powers of two just above 2^30: the modulus has one digit more than just below 2^30 and |v| ~ b^k / (b - 1) > q / 2
                             for b = 2, 4, 8, 32, 64; only 16 (k = 8, |v| = (2^32 - 1) / 15) works there
Base 0 (TrivGad) always works: the one digit is the lift itself, v = -1.
"""
from math import isqrt

import numpy as np

from oracle import lolmath as lm
from oracle import she_ref as sr
from test_rns_width_host import B13
from test_rns_width_host import good_below as _largest_below

# exclusive upper bounds of the arithmetic classes, by name
BOUNDS = {"27": 2 ** 27, "29": 2 ** 29, "30": 2 ** 30, "B13": B13 + 1, "31": 2 ** 31, "32": 2 ** 32, "61": 2 ** 61,
          "62": 2 ** 62}
assert B13 == isqrt((2 ** 64 - 1) // 13) + 1


def good_below(m, bound, count=None):
    """the largest prime q = 1 (mod m) below bound; with count, the `count` largest, descending"""
    if count is None:
        return _largest_below(m, bound)
    out = []
    for _ in range(count):
        bound = _largest_below(m, bound)
        out.append(bound)
    return out


def class_top(m, kind, count=1):
    """the `count` largest good primes of index m below the bound named `kind` (a key of BOUNDS), descending:
    q < 2^27 (32-bit lazy classes), 2^29 (Q32 knapsack), 2^30 (fused key switch), q <= B13 (13 (q-1)^2 < 2^64, class 2
    of the vector interpreter), 2^31 (Q32 decompose), 2^32 (Q32 KHPRF node), 2^61 and 2^62 (64-bit classes)"""
    return good_below(m, BOUNDS[kind], count)


def all_minus_one(q, base):
    """the integer whose centred base-`base` digits over Z_q are all -1 (base 0, TrivGad: the one digit is the lift),
    or None where there is none"""
    if base == 0:
        return -1
    if base < 2:
        return None
    k = sr.gadlen(base, q)
    v = -((base ** k - 1) // (base - 1))
    if 2 * -v > q - 1:
        return None
    x, digits = v, []                          # the digits as ZqBasic.hs:258-264 peels them
    for _ in range(k - 1):
        shift = base // 2
        x, r = (x + shift) // base, (x + shift) % base - shift
        digits.append(r)
    digits.append(x)
    return v if all(d == -1 for d in digits) else None


def pick_base(qs, lo=2, hi=64):
    """the first base in [lo, hi] with an all-(-1) value at every modulus (None if there is none)"""
    for b in range(lo, hi + 1):
        if all(all_minus_one(q, b) is not None for q in qs):
            return b
    return None


def saturating_c2(R, base):
    """[n][T] powerful-basis residues: v_t mod q_t at coefficient 0 of component t, 0 elsewhere"""
    c = np.zeros((R.n, R.T), dtype=np.int64)
    for t, q in enumerate(R.qs):
        v = all_minus_one(q, base)
        assert v is not None, (q, base)
        c[0, t] = v % q
    return c


def neg_rep(y, qs):
    """the same residues as representatives in (-q, 0]"""
    return np.where(y > 0, y - np.asarray(qs, dtype=np.int64), 0)


def full_q1(shape, qs):
    """q_t - 1 everywhere, component t innermost"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(qs, dtype=np.int64) - 1, tuple(shape) + (len(qs),)))


# ---- the tuples the GPU tests run, shared with the host test that proves their inputs saturate ------------------
# (m, kind, T): moduli = class_top(m, kind, T), base = pick_base(moduli)
KEYSWITCH_POW2 = [(32, "30", 3), (32, "27", 3), (2048, "30", 3), (2048, "27", 3), (2 ** 15, "30", 3), (2 ** 15, "27", 3)]
KEYSWITCH_MIXED = [(45, "B13", 2), (45, "27", 2), (1728, "B13", 2), (1728, "27", 2), (11648, "B13", 2), (11648, "27", 2)]
KHPRF_M = 64


def knapsack_wide(m):
    """the tuples of the 128-bit knapsack: the widest modulus moves the whole plan off Q32 (with the top of
    [2^29, 2^30), 17 terms would already overflow the Q32 form's 64-bit sum)"""
    return [[class_top(m, "29")[0], lm.first_good_q(m, 2 ** 29)],
            [class_top(m, "29")[0], class_top(m, "30")[0]],
            [class_top(m, "32")[0], class_top(m, "31")[0]],
            [class_top(m, "62")[0], class_top(m, "61")[0]]]


def khprf_moduli(m=KHPRF_M):
    """one-modulus plans of the KHPRF: the top of every fold_for step, the first 128-bit modulus, the top of class 1"""
    return [class_top(m, "29")[0], class_top(m, "30")[0], class_top(m, "31")[0], class_top(m, "32")[0],
            lm.first_good_q(m, 2 ** 32), class_top(m, "61")[0]]


def fold_for(q, ell):
    """khprf_api.cpp fold_for, restated: Q32 digits per 64-bit sum of k_khprf_node"""
    if q >= 2 ** 32:
        return 8
    F = (2 ** 64 - 1 - (q - 1)) // ((q - 1) ** 2)
    return min(F, ell)
