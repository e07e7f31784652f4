"""Host side of the lifted key-homomorphic ring PRF (include/lolhip.h lolhip_khprf_create_lifted): no GPU.

 - the entry is exported and declared, and KHPRF.lifted exists;
 - its statuses: plans of different indices, T != 1, q not a power of two, Q without a CRT basis, malformed trees;
 - the creation bound: C_m restated per prime power agrees with the products of the powerful basis through the CPU
   oracle, and creation accepts exactly the Q above 2 max(L C_m (q/2) max|digit|, C_m (q/2)^2);
 - lolhip_khprf_create still refuses Zq 8 with LOLHIP_ERR_NO_CRT;
 - work_len and every status of the compute entries on a host-only lifted family, the output untouched;
 - the restatement of tests/khprf_lifted_ref.py passes prop_keyHomom at the reference's benchmark shape (F128,
   Zq 2^k -> Zp, BaseBGad 2) at p > 2, and the ring product agrees between its two routes.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import khprf_lifted_ref as klr
from oracle import lolmath as lm
from oracle import she_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x5A5A5A5A


def _lifted(lolhip, m, q, Q, base, tree):
    Pq = lolhip.Plan.for_index(m, [q], host_only=True)
    PQ = lolhip.Plan.for_index(m, [Q], host_only=True)
    z = np.zeros((Pq.decomposeLen(base), Pq.n), dtype=np.int64)
    return Pq, PQ, lolhip.KHPRF.lifted(Pq, PQ, base, tree, z, z)


def test_lifted_entry_is_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    assert "lolhip_khprf_create_lifted" in names
    assert hasattr(C.CDLL(lolhip.lib_path()), "lolhip_khprf_create_lifted")
    assert callable(getattr(lolhip.KHPRF, "lifted", None))


def test_lifted_create_statuses(lolhip):
    T = lolhip.tensor
    Q = lm.first_good_q(128, 2 ** 30)
    Pq = lolhip.Plan.for_index(128, [8], host_only=True)
    PQ = lolhip.Plan.for_index(128, [Q], host_only=True)
    z = np.zeros((Pq.decomposeLen(2), Pq.n), dtype=np.int64)
    tree = lolhip.balanced_tree(5)

    def code(*args, **kw):
        with pytest.raises(lolhip.LolHipError) as e:
            lolhip.KHPRF.lifted(*args, **kw)
        return e.value.code

    # another index
    P64 = lolhip.Plan.for_index(64, [lm.first_good_q(64, 2 ** 30)], host_only=True)
    assert code(Pq, P64, 2, tree, z, z) == T.ERR_INVALID
    # T != 1 on either side
    PQ2 = lolhip.Plan.for_index(128, [Q, lm.first_good_q(128, Q + 1)], host_only=True)
    assert code(Pq, PQ2, 2, tree, z, z) == T.ERR_INVALID
    # q not a power of two; Q without a CRT basis
    P12 = lolhip.Plan.for_index(128, [12], host_only=True)
    z12 = np.zeros((P12.decomposeLen(2), P12.n), dtype=np.int64)
    assert code(P12, PQ, 2, tree, z12, z12) == T.ERR_MODULUS
    assert code(Pq, lolhip.Plan.for_index(128, [2 ** 31 - 1], host_only=True), 2, tree, z, z) == T.ERR_NO_CRT
    # malformed trees, a bad base, NULL pointers
    for bad in ([2, 1], [3, 1, 1, 1], [0], [63]):
        assert code(Pq, PQ, 2, bad, z, z) == T.ERR_INVALID
    L = lolhip.lib()
    h = C.c_void_p()
    tr = (C.c_int32 * 1)(1)
    ptr = z.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.lolhip_khprf_create_lifted(Pq._h, PQ._h, 1, tr, 1, ptr, ptr, C.byref(h)) == T.ERR_INVALID
    assert L.lolhip_khprf_create_lifted(Pq._h, None, 2, tr, 1, ptr, ptr, C.byref(h)) == T.ERR_INVALID
    assert L.lolhip_khprf_create_lifted(Pq._h, PQ._h, 2, tr, 1, ptr, None, C.byref(h)) == T.ERR_INVALID
    # the one-modulus constructor is unchanged: Zq 8 has no CRT basis
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.KHPRF(Pq, 2, tree, z, z)
    assert e.value.code == T.ERR_NO_CRT
    # fine: q = 2, 8, 32, 2^20 and a one-leaf tree
    for q in (2, 8, 32):
        _lifted(lolhip, 128, q, Q, 2, tree)
    _lifted(lolhip, 128, 2 ** 20, lm.first_good_q(128, 2 ** 55), 0, [1])


@pytest.mark.parametrize("m", [7, 9, 16, 15, 45, 40, 28])
def test_growth_restatement_matches_the_powerful_basis(cpuref, m):
    assert klr.growth(m) == klr.growth_bruteforce(cpuref, m)


def test_growth_of_two_powers_is_n():
    for e in range(1, 12):
        assert klr.growth(2 ** e) == max(1, 2 ** (e - 1))


@pytest.mark.parametrize("m,q,base", [(128, 8, 2), (128, 32, 2), (128, 8, 0), (64, 256, 4), (45, 8, 2),
                                      (8 * 5 * 7 * 13, 8, 2), (40, 16, 0)])
def test_creation_accepts_exactly_the_certified_Q(lolhip, m, q, base):
    need = klr.bound(m, q, base)                      # accepted iff Q > need
    above = lm.first_good_q(m, need + 1)
    below = None
    for cand in range(need - (need % m) + 1, 1, -m):  # the largest good prime <= need
        if cand <= need and lm.is_prime(cand):
            below = cand
            break
    _lifted(lolhip, m, q, above, base, [2, 1, 1])
    if below is not None:
        with pytest.raises(lolhip.LolHipError) as e:
            _lifted(lolhip, m, q, below, base, [2, 1, 1])
        assert e.value.code == lolhip.tensor.ERR_MODULUS


def test_lifted_work_len_and_statuses_on_a_host_only_family(lolhip):
    T = lolhip.tensor
    L = lolhip.lib()
    Q = lm.first_good_q(128, 2 ** 30)
    tree = lolhip.balanced_tree(5)
    Pq, PQ, f = _lifted(lolhip, 128, 8, Q, 2, tree)
    nL = Pq.decomposeLen(2)
    assert nL == 4
    out = np.full((2, 32, nL, Pq.n), SENT, dtype=np.int64)
    work = np.zeros(max(f.workLen(0, 32), 1), dtype=np.int64)
    s = np.zeros((2, Pq.n), dtype=np.int64)
    o, w, sp = out.ctypes.data, work.ctypes.data, s.ctypes.data
    ev = lambda x0, B: L.lolhip_khprf_eval_batch(f._h, None, x0, B, o, w)
    pr = lambda nk, p, x0, B: L.lolhip_khprf_batch(f._h, None, sp, nk, p, x0, B, o, w)
    assert ev(-1, 1) == T.ERR_INVALID
    assert ev(31, 2) == T.ERR_INVALID
    assert ev(0, 32) == T.ERR_NO_DEVICE
    assert pr(0, 2, 0, 32) == T.ERR_INVALID
    assert pr(1, 1, 0, 32) == T.ERR_MODULUS                            # p < 2
    assert pr(1, 8, 0, 32) == T.ERR_MODULUS                            # p >= q
    assert pr(2, 2, 0, 32) == T.ERR_NO_DEVICE
    assert L.lolhip_khprf_work_len(f._h, 0, 33) == -1
    assert (out == SENT).all()
    with pytest.raises(lolhip.NoDeviceError):
        f.eval(0, 32)


def test_lifted_work_len_follows_the_slot_formula(lolhip):
    import test_khprf_host as th
    rng = np.random.default_rng(5)
    for base, q in ((2, 8), (0, 32), (4, 2 ** 10)):
        Q = lm.first_good_q(128, 2 ** 50)
        for tree in (lolhip.balanced_tree(7), lolhip.right_spine_tree(6), [3, 1, 2, 1, 1], [1]):
            Pq, PQ, f = _lifted(lolhip, 128, q, Q, base, tree)
            k, nL = tree[0], Pq.decomposeLen(base)
            wins = [(0, 2 ** k), (0, 1), (2 ** k - 1, 1), (0, 0)] + \
                   [(int(a), int(rng.integers(0, 2 ** k - a + 1))) for a in rng.integers(0, 2 ** k, 4)]
            for x0, B in wins:
                assert f.workLen(x0, B) == th._work_len(tree, nL, Pq.n, x0, B), (tree, base, x0, B)


def test_lifted_restatement_matches_the_prime_restatement_on_products(cpuref):
    """the lifted ring product (negacyclic convolution, or the oracle at Q') reduced mod q equals the CPU oracle's
    product at a prime, reduced, for m = 2^e and for a composite m"""
    rng = np.random.default_rng(1)
    for m, q in ((128, 8), (64, 32), (8 * 5 * 7, 16)):
        R = klr.LiftedRing(cpuref, m, q)
        R2 = klr.LiftedRing(cpuref, m, q, prime_lower=2 ** 45)
        a, b = (rng.integers(0, q, size=(3, R.n), dtype=np.int64) for _ in range(2))
        got = R.mul(a, b)
        assert got.min() >= 0 and got.max() < q
        assert R.Qp != R2.Qp
        assert np.array_equal(got, R2.mul(a, b))
        if R.pow2:
            R.pow2 = False                              # the oracle route over the same ring
            assert np.array_equal(got, R.mul(a, b))


@pytest.mark.parametrize("m,q,p,size", [(128, 32, 4, 3), (128, 16, 8, 5), (8 * 5 * 7, 32, 4, 2)])
def test_lifted_restatement_is_key_homomorphic(cpuref, m, q, p, size):
    """prop_keyHomom (KHPRFTests.hs) over q = 2^k, BaseBGad 2, every input: F(s1 + s2) - F(s1) - F(s2) is -1, 0 or 1
    per coefficient (centred mod p, p > 2 so that this can fail), and not always 0"""
    rng = np.random.default_rng(size + q)
    base = 2
    R = klr.LiftedRing(cpuref, m, q)
    nL = sr.gadlen(base, q)
    a0, a1 = (rng.integers(0, q, size=(nL, R.n), dtype=np.int64) for _ in range(2))
    s1, s2 = (rng.integers(0, q, size=(R.n,), dtype=np.int64) for _ in range(2))
    s3 = (s1 + s2) % q

    def rtree(k):
        if k == 1:
            return [1]
        a = int(rng.integers(1, k))
        return [k] + rtree(a) + rtree(k - a)

    tree = rtree(size)
    nonzero = 0
    for x in range(2 ** size):
        f1, f2, f3 = (klr.ring_prf(R, base, tree, a0, a1, s, p, x) for s in (s1, s2, s3))
        d = (f3 - f1 - f2) % p
        d = np.where(2 * d < p, d, d - p)
        assert np.abs(d).max() <= 1, (tree, x)
        nonzero += int(np.count_nonzero(d))
    assert nonzero > 0


def test_key_homomorphism_check_rejects_an_unrelated_key(cpuref):
    """the check above is not vacuous: with an unrelated third key the centred difference leaves [-1, 1]"""
    rng = np.random.default_rng(7)
    q, p, base = 32, 4, 2
    R = klr.LiftedRing(cpuref, 128, q)
    nL = sr.gadlen(base, q)
    a0, a1 = (rng.integers(0, q, size=(nL, R.n), dtype=np.int64) for _ in range(2))
    s1, s2, s3 = (rng.integers(0, q, size=(R.n,), dtype=np.int64) for _ in range(3))
    f1, f2, f3 = (klr.ring_prf(R, base, [3, 2, 1, 1, 1], a0, a1, s, p, 5) for s in (s1, s2, s3))
    d = (f3 - f1 - f2) % p
    assert np.abs(np.where(2 * d < p, d, d - p)).max() == 2
