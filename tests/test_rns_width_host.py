"""Wide and mixed-width RNS tuples on host-only plans (no GPU).

  plan limit            a plan takes up to 64 moduli and refuses 65
  gadget at T = 16      decomposeLen / gadget equal oracle/she_ref.py for uniform and mixed-width tuples and base 2;
                        T = 17 is refused (every pipeline carries its per-component constants in 16-entry arrays)
  class of a tuple      the vector interpreter picks one arithmetic class per plan (plan.cpp): the widest modulus wins,
                        whatever its position.  Read through the stage program a lone crt launches: class 2 merges
                        3^2 into one dense stage and 3 (x) 5 into one Kronecker stage; classes 0, 1 and 3 keep the
                        staged form.
"""
from math import isqrt

import numpy as np
import pytest

from oracle import lolmath as lm
from oracle import she_ref as sr
from oracle.oracle import Params

ERR_INVALID = -1
B13 = isqrt((2 ** 64 - 1) // 13) + 1          # q - 1 < B13  <=>  13 (q - 1)^2 < 2^64: one 64-bit accumulator per dot product


def good_below(m, bound):
    """largest prime q = 1 (mod m) below bound"""
    q = (bound - 2) // m * m + 1
    while not lm.is_prime(q):
        q -= m
    return q


def mixed_moduli(m):
    """one modulus per arithmetic boundary: below 2^27; either side of 13 (q-1)^2 = 2^64; below 2^31 and 2^32;
    either side of 2^61"""
    qs = [good_below(m, 2 ** 27), good_below(m, B13 + 1), lm.first_good_q(m, B13), good_below(m, 2 ** 31),
          good_below(m, 2 ** 32), good_below(m, 2 ** 61), lm.first_good_q(m, 2 ** 61)]
    assert 13 * (qs[1] - 1) ** 2 < 2 ** 64 <= 13 * (qs[2] - 1) ** 2 and qs[6] < 2 ** 62
    return qs


def mixed16(m):
    """16 distinct moduli, two or three from each class, interleaved (neither sorted order)"""
    cls = [[good_below(m, 2 ** 27), lm.first_good_q(m, 2 ** 20), lm.first_good_q(m, 2 ** 26)],
           [good_below(m, B13 + 1), lm.first_good_q(m, 2 ** 29)],
           [lm.first_good_q(m, B13), good_below(m, 2 ** 31), good_below(m, 2 ** 32), lm.first_good_q(m, 2 ** 31)],
           [good_below(m, 2 ** 61), lm.first_good_q(m, 2 ** 40), lm.first_good_q(m, 2 ** 59)],
           [lm.first_good_q(m, 2 ** 61), lm.first_good_q(m, 2 ** 61 + 2 ** 50), good_below(m, 2 ** 62), ]]
    out = []
    while any(cls):
        for c in cls:
            if c:
                out.append(c.pop())
    out.append(lm.first_good_q(m, 2 ** 16))
    assert len(set(out)) == 16 and max(out) < 2 ** 62
    return out


def test_plan_takes_64_moduli_and_refuses_65(lolhip):
    g = lm.good_qs(16, 2 ** 40)
    qs = [next(g) for _ in range(65)]
    P = lolhip.Plan([(2, 4)], qs[:64], host_only=True)
    assert P.T == 64 and P.n == 8
    assert [int(q) for q in P._table(5)] == qs[:64]
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.Plan([(2, 4)], qs, host_only=True)
    assert ei.value.code == ERR_INVALID


@pytest.mark.parametrize("m", [64, 45])
@pytest.mark.parametrize("kind", ["uniform", "mixed", "mixed_desc", "mixed16"])
@pytest.mark.parametrize("base", [0, 2, 3, 256, 2 ** 20])
def test_decompose_len_and_gadget_at_wide_tuples(lolhip, m, kind, base):
    if kind == "uniform":
        g = lm.good_qs(m, 2 ** 59)
        qs = [next(g) for _ in range(16)]
    elif kind == "mixed16":
        qs = mixed16(m)
    else:
        qs = mixed_moduli(m)
        if kind == "mixed_desc":
            qs = sorted(qs, reverse=True)
    pps = lm.factor_pps(m)
    P, R = lolhip.Plan(pps, qs, host_only=True), Params(pps, qs)
    assert P.decomposeLen(base) == sum(sr.digit_counts(R, base))
    assert np.array_equal(P.gadget(base), sr.gadget(R, base))
    if base == 2 and kind == "mixed16":
        assert P.decomposeLen(base) > 500


def test_decompose_len_refuses_17_moduli(lolhip):
    g = lm.good_qs(64, 2 ** 30)
    qs = [next(g) for _ in range(17)]
    P = lolhip.Plan([(2, 6)], qs, host_only=True)
    for base in (0, 2, 256):
        with pytest.raises(lolhip.LolHipError) as ei:
            P.decomposeLen(base)
        assert ei.value.code == ERR_INVALID
        with pytest.raises(lolhip.LolHipError):
            P.gadget(base)
    assert lolhip.Plan([(2, 6)], qs[:16], host_only=True).decomposeLen(0) == 16


def _prog(lolhip, m, qs, inverse=False):
    """the program of the one-launch poly-mul, which both indices below have in every class (a lone crt of 14400 with
    64-bit residues launches the odd primes' stages alone: test_scalar_interp_host.py)"""
    return [tuple(int(v) for v in r) for r in lolhip.Plan(lm.factor_pps(m), qs, host_only=True).program(inverse, polymul=True)]


def test_mixed_width_tuples_take_the_class_of_their_widest_modulus(lolhip):
    # m = 14400 = 64 * 9 * 25: class 2 merges 3^2 into one 6-vector stage (kind 2, length 6); 5^2 merges only while
    # 20 (q-1)^2 fits 64 bits (q < 2^27 here); the staged form runs 3^2 as CRT_3 (length 2) + DFT_3 (length 3)
    m = 14400
    q26, qs = lm.first_good_q(m, 2 ** 26), mixed_moduli(m)
    q27, lo13, hi13 = qs[0], qs[1], qs[2]
    small = [(12, 1, 4, 1), (12, 5, 1, 16), (2, 3, 6, 32), (2, 5, 20, 192)]
    class2 = [(12, 1, 4, 1), (12, 5, 1, 16), (2, 3, 6, 32), (2, 5, 4, 192), (1, 5, 5, 768)]
    staged = [(12, 1, 4, 1), (12, 5, 1, 16), (2, 3, 2, 32), (1, 3, 3, 64), (2, 5, 4, 192), (1, 5, 5, 768)]
    assert _prog(lolhip, m, [q26, q27]) == small
    for tup in ([q27, lo13], [lo13, q26, q27], [q27, q26, lo13]):
        assert _prog(lolhip, m, tup) == class2, tup
    for wide in qs[2:]:                                       # class 1 (13 (q-1)^2 >= 2^64, q < 2^32), 3 (< 2^61), 0
        for tup in ([wide, q27, lo13], [q27, lo13, wide], [lo13, wide, q26]):
            assert _prog(lolhip, m, tup) == staged, tup
            assert _prog(lolhip, m, tup, True) == _prog(lolhip, m, [wide], True), tup
    assert _prog(lolhip, m, qs) == _prog(lolhip, m, qs[::-1]) == staged
    # m = 15015 = 3 * 5 * 7 * 11 * 13: class 2 runs 3 (x) 5 as one 8-vector stage; every other class keeps CRT_3, CRT_5
    m = 15015
    qs = mixed_moduli(m)
    kron = [(2, 3, 8, 1), (2, 7, 6, 8), (2, 11, 10, 48), (2, 13, 12, 480)]
    plain = [(2, 3, 2, 1), (2, 5, 4, 2), (2, 7, 6, 8), (2, 11, 10, 48), (2, 13, 12, 480)]
    assert _prog(lolhip, m, qs[:2]) == _prog(lolhip, m, qs[1::-1]) == kron
    for wide in qs[2:]:
        assert _prog(lolhip, m, [wide] + qs[:2]) == plain, wide
        assert _prog(lolhip, m, qs[:2] + [wide]) == plain, wide
    assert _prog(lolhip, m, mixed16(m)) == plain
