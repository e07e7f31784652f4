"""The roundings of the key-homomorphic ring PRF on chosen residues: k_khprf_round (q an odd prime) and the LIFT_ROUND /
LIFT_FROM_Q / LIFT_TO_Q modes of k_khprf_lift (q = 2^k), khprf.hip.

Technique: a one-leaf family has A_T(x) = a_x, and the key "1" (all ones in the CRT basis; the unit vector on the lifted
side) makes s A = A, so lolhip_khprf_batch rounds exactly the residues put into a0 and a1: at a two-power index lInv
is the identity and a0 = crt(X) rounds X itself.  The expected value is ((p lift(x) + q div 2) div q) mod p in Python
integers, cross-checked here against khprf_ref.rescale_dec and khprf_lifted_ref.rescale_dec.

Without a GPU (the tests not marked gpu):
    the chosen residues hold 0, 1, q - 1, (q -+ 1) / 2, both neighbours of the rounding boundaries (2j + 1) q / (2p) for
    j = 0, 1, p/2 - 1, p/2, p - 2, p - 1 and random j, and the negatives of all of these; both sides of min(12, p)
    distinct boundaries are present per (q, p) (there are only p boundaries mod q);
    k_khprf_round's unsigned form a = p (lift x + q) + q div 2 is replayed in Python integers with its ranges asserted
    (a < 2^64, quotient < 2p, the quotient exact through q^-1 mod 2^64), and reaches a >= 2^63 wherever
    p = floor((2^63 - 1) / q) is a valid p; k_khprf_lift's signed form likewise (|p lift r| < 2^62).
On the device:
    plain    index 32, base 2 (2 L n slots), q at the top of the 29-, 31- and 32-bit classes, just above 2^32, at 40
             bits and just below 2^61 and 2^62; p in {2, 3, floor((2^63 - 1) / q) or q - 1, an odd p near its root}
    lifted   (m, q) = (128, 2^10): every residue of Z_q, p in {2, 3, 5, 512, 1023}; (8, 2^30): boundary neighbours,
             p in {2, 3, 2^29, 2^30 - 1}; (8, 4): p in {2, 3}; (8, 2): eval only, p = 2 is refused; 8*5*7*13 over q = 8,
             where lInv sits between LIFT_FROM_Q and LIFT_ROUND; a two-leaf TrivGad family whose product with 1 sends
             the extremes -q/2 and q/2 - 1 through LIFT_TO_Q, the node kernel and LIFT_FROM_Q
"""
from math import isqrt

import numpy as np
import pytest

import khprf_lifted_ref as klr
import khprf_ref as kr
from oracle import lolmath as lm
from oracle import she_ref as sr
from oracle.oracle import Params
from saturate import class_top

M = 32                                                         # n = 16, lInv is the identity
BASE = 2
PLAIN_Q = [class_top(M, "29")[0], class_top(M, "31")[0], class_top(M, "32")[0], lm.first_good_q(M, 2 ** 32),
           lm.first_good_q(M, 2 ** 39), class_top(M, "61")[0], class_top(M, "62")[0]]
RANDOM_J = 8


def valid_p(q, p):
    """lolhip_khprf_batch's own condition"""
    return 2 <= p < q and p * q < 2 ** 63


def largest_p(q):
    pmax = (2 ** 63 - 1) // q
    return pmax if pmax < q else q - 1


def round_ps(q):
    """{2, 3, the largest valid p, an odd p near its root}, those lolhip_khprf_batch accepts"""
    big = largest_p(q)
    return sorted({p for p in (2, 3, big, isqrt(big) | 1) if valid_p(q, p)})


def lift(x, q):
    """the centred representative: [-q/2, q/2) (for odd q: |v| <= (q - 1) / 2)"""
    return x - q if 2 * x >= q else x


def expected(x, q, p):
    return ((p * lift(x, q) + q // 2) // q) % p


def chosen(q, p, rng):
    """the residues next to where the rounding to Z_p changes, the ends of Z_q and of the centred lift, and their
    negatives"""
    xs = [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2, q // 2, q // 2 - 1]
    js = [0, 1, p // 2 - 1, p // 2, p - 2, p - 1] + [int(j) for j in rng.integers(0, p, RANDOM_J)]
    for j in dict.fromkeys(js):
        if 0 <= j < p:
            b = (2 * j + 1) * q // (2 * p)
            xs += [b - 1, b, b + 1]
    xs += [-x for x in xs]
    return [x % q for x in xs]


def residues(q, ps, slots, seed=0):
    """`slots` residues of Z_q: chosen(q, p) for every p, then random fill (all of Z_q first when it fits)"""
    rng = np.random.default_rng([seed, q % 2 ** 32, q >> 32])
    xs = []
    for p in ps:
        xs += chosen(q, p, rng)
    xs = list(dict.fromkeys(xs))
    if q <= slots:
        xs = list(dict.fromkeys(xs + list(range(q))))
    assert len(xs) <= slots, (q, len(xs), slots)
    xs += [int(v) for v in rng.integers(0, q, slots - len(xs))]
    return xs


def boundaries_straddled(xs, q, p):
    """the x with x and x + 1 both present and rounded differently"""
    have = set(xs)
    return {x for x in have if (x + 1) % q in have and expected(x, q, p) != expected((x + 1) % q, q, p)}


def plain_slots(q):
    return 2 * sr.gadlen(BASE, q) * 16


# ---- without a GPU ----------------------------------------------------------------------------------------------------
def test_moduli_and_ps_are_what_the_header_says():
    assert [q.bit_length() for q in PLAIN_Q] == [29, 31, 32, 33, 40, 61, 62]
    for q in PLAIN_Q:
        assert q % M == 1 and lm.is_prime(q)
        ps = round_ps(q)
        assert 2 in ps and ps == sorted(set(ps)) and all(valid_p(q, p) for p in ps)
        big = largest_p(q)
        assert big in ps and not valid_p(q, big + 1)
    assert [round_ps(q) for q in PLAIN_Q[-2:]] == [[2, 3, 4], [2]]
    assert all(len(round_ps(q)) == 4 for q in PLAIN_Q[:5])
    # the host check of lolhip_khprf_batch accepts floor((2^63 - 1) / q) and refuses one more: from 32 bits on
    assert [largest_p(q) == (2 ** 63 - 1) // q for q in PLAIN_Q] == [False, False, True, True, True, True, True]


@pytest.mark.parametrize("q", PLAIN_Q)
def test_round_formula_replayed_on_the_chosen_residues(q):
    """k_khprf_round in Python integers, every stated range asserted"""
    ps = round_ps(q)
    xs = residues(q, ps, plain_slots(q))
    assert len(xs) == plain_slots(q) and all(0 <= x < q for x in xs)
    assert {0, 1, q - 1, (q - 1) // 2, (q + 1) // 2} <= set(xs)
    qinv = pow(q, -1, 2 ** 64)
    for p in ps:
        top = 0
        for x in xs:
            vq = x + q if 2 * x < q else x                      # lift x + q
            assert q // 2 < vq <= q + q // 2
            a = p * vq + (q >> 1)
            assert a < 2 ** 64
            top = max(top, a)
            quot = ((a - a % q) * qinv) % 2 ** 64
            assert quot == a // q and quot < 2 * p
            assert (quot - p if quot >= p else quot) == expected(x, q, p), (q, p, x)
        if p == (2 ** 63 - 1) // q:                             # p q ~ 2^63: the sum passes the sign bit
            assert top >= 2 ** 63, (q, p)
        # only p boundaries exist mod q; both sides of min(12, p) distinct ones are among the residues
        assert len(boundaries_straddled(xs, q, p)) >= min(2 * 6, p), (q, p)


def test_expected_value_is_the_restated_rescale(cpuref):
    for q in (PLAIN_Q[0], PLAIN_Q[3], PLAIN_Q[5]):
        P = Params([(2, 5)], [q])
        for p in round_ps(q):
            xs = residues(q, round_ps(q), plain_slots(q))
            X = np.array(xs, dtype=np.int64).reshape(-1, 16)
            got = kr.rescale_dec(cpuref, P, cpuref.crt(P, X.reshape(-1, 16, 1)).reshape(X.shape), p)
            assert got.reshape(-1).tolist() == [expected(x, q, p) for x in xs], (q, p)
    R = klr.LiftedRing(cpuref, 128, 2 ** 10)
    for p in (2, 3, 5, 512, 1023):
        xs = list(range(1024))
        got = klr.rescale_dec(R, np.array(xs, dtype=np.int64).reshape(-1, 64), p)
        assert got.reshape(-1).tolist() == [expected(x, 2 ** 10, p) for x in xs], p


LIFTED = [  # m, q, base, ps
    (128, 2 ** 10, 2, (2, 3, 5, 512, 1023)),
    (8, 2 ** 30, 2, (2, 3, 2 ** 29, 2 ** 30 - 1)),
    (8, 4, 2, (2, 3)),
]


def lifted_Q(m, q, base):
    """the first NTT prime above the creation bound of include/lolhip.h.  For a wide q the key product decides it:
    C_m (q/2)^2 >= L C_m (q/2) max|digit| as soon as L max|digit| <= q/2, and base-2 digits are at most 1"""
    if q <= 2 ** 12:
        return lm.first_good_q(m, klr.bound(m, q, base) + 1)
    assert base == 2 and sr.gadlen(2, q) <= q // 2
    return lm.first_good_q(m, 2 * klr.growth(m) * (q // 2) ** 2 + 1)


def test_lifted_moduli_and_slots(lolhip):
    assert [lifted_Q(m, q, b) for m, q, b, _ in LIFTED] == [33555073, 2305843009213694009, 73]
    assert lifted_Q(8, 2, 2) == 41
    slots = []
    for m, q, base, ps in LIFTED:
        Pq = lolhip.Plan.for_index(m, [q], host_only=True)
        PQ = lolhip.Plan.for_index(m, [lifted_Q(m, q, base)], host_only=True)
        L = Pq.decomposeLen(base)
        lolhip.KHPRF.lifted(Pq, PQ, base, [1], np.zeros((L, Pq.n)), np.zeros((L, Pq.n)))
        slots.append(2 * L * Pq.n)
        assert all(valid_p(q, p) for p in ps)
    assert slots == [1408, 248, 24]
    assert not valid_p(2, 2)                                    # q = 2 has no p


@pytest.mark.parametrize("m,q,base,ps", LIFTED)
def test_lift_formula_replayed_on_the_chosen_residues(m, q, base, ps):
    """lift_one<LIFT_FROM_Q | LIFT_ROUND> in Python integers: the centred lift mod Q comes back as the residue, the
    product stays inside int64 and the arithmetic shift is the floor"""
    n = lm.totient_pps(lm.factor_pps(m))
    slots = 2 * sr.gadlen(base, q) * n
    xs = residues(q, ps, slots)
    if q <= slots:
        assert set(xs) == set(range(q))
    Q, k = lifted_Q(m, q, base), q.bit_length() - 1
    for p in ps:
        for x in xs:
            xq = lift(x, q) % Q                                 # what LIFT_TO_Q and an exact product by 1 leave
            v = xq if 2 * xq < Q else xq - Q
            r = v & (q - 1)
            assert r == x
            lr = r - q if r >= q // 2 else r
            assert abs(p * lr) < 2 ** 62
            y = (p * lr + q // 2) >> k
            assert -p <= 2 * y <= p
            assert (y + p if y < 0 else y) == expected(x, q, p), (q, p, x)
        if q > 4:
            assert len(boundaries_straddled(xs, q, p)) >= min(2 * 6, p), (q, p)


# ---- on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("q", PLAIN_Q)
def test_round_on_chosen_residues(gpu, cpuref, q):
    import torch
    T = gpu.tensor
    P = Params([(2, 5)], [q])
    plan = gpu.Plan([(2, 5)], [q])
    L = plan.decomposeLen(BASE)
    ps = round_ps(q)
    xs = residues(q, ps, 2 * L * P.n)
    X = np.array(xs, dtype=np.int64).reshape(2, L, P.n)
    a = cpuref.crt(P, X.reshape(-1, P.n, 1)).reshape(X.shape)
    f = gpu.KHPRF(plan, BASE, [1], a[0], a[1])
    assert np.array_equal(f.eval(0, 2).cpu().numpy(), a)
    one = np.ones(P.n, dtype=np.int64)                          # crt(1)
    for p in ps:
        got = f(one, p, 0, 2).cpu().numpy()
        want = np.array([expected(x, q, p) for x in xs], dtype=np.int64).reshape(X.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (q, p, [(xs[int(np.ravel_multi_index(tuple(i), X.shape))]) for i in bad[:4]])
        # the second input alone, the key as representatives in (-q, 0]: 1 = 1 - q
        got1 = f(one - q, p, 1, 1).cpu().numpy()
        assert np.array_equal(got1[0], want[1]), (q, p)
    # one past the largest p is refused before any launch
    out = torch.full((2, L, P.n), 0x5A5A, dtype=torch.int64, device="cuda")
    s = torch.ones((1, P.n), dtype=torch.int64, device="cuda")
    for p in (largest_p(q) + 1, 1, q):
        rc = gpu.lib().lolhip_khprf_batch(f._h, None, s.data_ptr(), 1, p, 0, 2, out.data_ptr(), out.data_ptr())
        assert rc == T.ERR_MODULUS, (q, p)
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())


def _lifted_family(gpu, m, q, base, tree, a0, a1):
    Pq, PQ = gpu.Plan.for_index(m, [q]), gpu.Plan.for_index(m, [lifted_Q(m, q, base)])
    return gpu.KHPRF.lifted(Pq, PQ, base, tree, a0, a1)


@pytest.mark.gpu
@pytest.mark.parametrize("m,q,base,ps", LIFTED)
def test_lift_round_on_chosen_residues(gpu, m, q, base, ps):
    n = lm.totient_pps(lm.factor_pps(m))
    L = sr.gadlen(base, q)
    xs = residues(q, ps, 2 * L * n)
    X = np.array(xs, dtype=np.int64).reshape(2, L, n)
    f = _lifted_family(gpu, m, q, base, [1], X[0], X[1])
    assert np.array_equal(f.eval(0, 2).cpu().numpy(), X)
    one = np.zeros(n, dtype=np.int64)
    one[0] = 1                                                  # the powerful basis' first element is 1
    for p in ps:
        got = f(one, p, 0, 2).cpu().numpy()
        want = np.array([expected(x, q, p) for x in xs], dtype=np.int64).reshape(X.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (q, p, [(xs[int(np.ravel_multi_index(tuple(i), X.shape))]) for i in bad[:4]])


@pytest.mark.gpu
def test_lift_over_one_bit(gpu):
    """q = 2: qbits = 1, the residue 1 lifts to -1; there is no p with 2 <= p < q"""
    import torch
    m, q, base = 8, 2, 2
    rng = np.random.default_rng(2)
    X = rng.integers(0, 2, size=(2, 2, 4), dtype=np.int64)
    f = _lifted_family(gpu, m, q, base, [1], X[0], X[1])
    assert f.L == 2 and np.array_equal(f.eval(0, 2).cpu().numpy(), X)
    out = torch.full((2, 2, 4), 0x5A5A, dtype=torch.int64, device="cuda")
    s = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    rc = gpu.lib().lolhip_khprf_batch(f._h, None, s.data_ptr(), 1, 2, 0, 2, out.data_ptr(), out.data_ptr())
    assert rc == gpu.tensor.ERR_MODULUS
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())
    # a two-leaf tree: the products a_l G^-1(a_r) over Z_2[x] / (x^4 + 1), through every lift mode but the rounding
    g = _lifted_family(gpu, m, q, base, [2, 1, 1], X[0], X[1])
    R = klr.LiftedRing(None, m, q)
    got = g.eval(0, 4).cpu().numpy()
    for x in range(4):
        assert np.array_equal(got[x], klr.eval_tree(R, base, [2, 1, 1], X[0], X[1], x)), x


@pytest.mark.gpu
@pytest.mark.parametrize("m,q", [(128, 2 ** 10), (8, 2 ** 30), (8, 4), (8, 2)])
def test_lift_extremes_through_a_product_by_one(gpu, m, q):
    """tree [2, 1, 1] under TrivGad with a1 = 1: A(1) = a0 G^-1(1) = a0 and A(2) = 1 G^-1(a0) = a0, so a0's residues
    (-q/2 and q/2 - 1 among them) go through LIFT_TO_Q, the node product mod Q, crtInv and LIFT_FROM_Q, once as the
    left factor and once as the digit"""
    n = lm.totient_pps(lm.factor_pps(m))
    rng = np.random.default_rng([m, q % 2 ** 32])
    a0 = rng.integers(0, q, size=(1, n), dtype=np.int64)
    a0[0, :4] = [q // 2, q // 2 - 1, q - 1, 0]
    a1 = np.zeros((1, n), dtype=np.int64)
    a1[0, 0] = 1
    Pq = gpu.Plan.for_index(m, [q])
    PQ = gpu.Plan.for_index(m, [lm.first_good_q(m, 2 * klr.growth(m) * (q // 2) ** 2 + 1)])   # TrivGad: both terms are C (q/2)^2
    f = gpu.KHPRF.lifted(Pq, PQ, 0, [2, 1, 1], a0, a1)
    got = f.eval(1, 3).cpu().numpy()
    assert np.array_equal(got[0], a0) and np.array_equal(got[1], a0) and np.array_equal(got[2], a1)


@pytest.mark.gpu
def test_lift_round_behind_linv_at_a_mixed_index(gpu, cpuref):
    """m = 8*5*7*13, q = 8: LIFT_FROM_Q, then lInv mod q, then LIFT_ROUND alone, on residues that hold every value of
    Z_8 in every position class"""
    m, q, base = 8 * 5 * 7 * 13, 8, 2
    R = klr.LiftedRing(cpuref, m, q)
    L = sr.gadlen(base, q)
    rng = np.random.default_rng(m)
    X = rng.integers(0, q, size=(2, L, R.n), dtype=np.int64)
    X[0, 0] = np.arange(R.n) % q
    X[0, 1] = q // 2
    X[1, 0] = q // 2 - 1
    X[1, 1] = q - 1
    f = _lifted_family(gpu, m, q, base, [1], X[0], X[1])
    assert np.array_equal(f.eval(0, 2).cpu().numpy(), X)
    one = np.zeros(R.n, dtype=np.int64)
    one[0] = 1
    for p in (2, 3, 7):
        got = f(one, p, 0, 2).cpu().numpy()
        want = klr.rescale_dec(R, X.reshape(-1, R.n), p).reshape(X.shape)
        assert np.array_equal(got, want), p
