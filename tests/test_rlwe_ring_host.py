"""Host side of the RLWE / RLWR entries over moduli without a CRT basis (lolhip_rlwe_ring_*, include/lolhip.h): no GPU.

 - rlwe-challenges' parameter list (tests/golden/rlwe_challenge_params.txt) classified by the project's rules: 168 lines
   on the plan route, 212 on the ring route (83 distinct (m, q)), 136 refused by the sampler's index limits;
 - every ring pair over host-only handles: one NTT prime, the restated work length, and NO_DEVICE from the sample call,
   which is answered only after every host check has passed;
 - every status of the header and its order, as far as a host-only handle can show it;
 - the restatement of tests/rlwe_ring_ref.py against the plan route's restatement on primes q = 1 mod m.
"""
import ctypes as C

import numpy as np
import pytest

import rlwe_ring_ref as rg
from oracle import lolmath as lm
from oracle.oracle import Params

OK, ERR_INVALID, ERR_NO_CRT, ERR_NO_DEVICE = 0, -1, -3, -5
KEY = bytes(range(32))
PAIRS = rg.ring_pairs()


def test_the_challenge_list_splits_168_212_136():
    lines = rg.challenge_lines()
    assert len(lines) == 516
    by = {}
    for kind, m, q, _ in lines:
        by.setdefault(rg.classify(kind, m, q), []).append(kind)
    assert {k: len(v) for k, v in by.items()} == {"plan": 168, "ring": 212, "index": 136}
    assert {k: by["ring"].count(k) for k in ("Cont", "Disc", "RLWR")} == {"Cont": 84, "Disc": 84, "RLWR": 44}
    assert set(by["index"]) == {"Cont", "Disc"}
    assert len(PAIRS) == 83


class Handles:
    """host-only pq, RingMul and the raw entries"""

    def __init__(self, lolhip, m, q):
        self.L = lolhip.lib()
        self.pq = lolhip.Plan.for_index(m, [q], host_only=True)
        self.ring = lolhip.RingMul(self.pq)
        self.n, self.K = self.pq.n, self.ring.K

    def sample(self, kind, p=2, svar=1.0, B=3, h=True, pq=True, ptr=None, key=KEY):
        return self.L.lolhip_rlwe_ring_sample_batch(self.ring._h if h is True else h, self.pq._h if pq is True else pq,
                                                    None, kind, p, ptr, svar, key, 0, ptr, ptr, ptr, B)

    def error(self, kind, B=3, ptr=None):
        return self.L.lolhip_rlwe_ring_error_batch(self.ring._h, self.pq._h, None, kind, ptr, ptr, ptr, ptr, ptr, ptr, B)

    def rounded(self, p=2, B=3, ptr=None):
        return self.L.lolhip_rlwr_ring_rounded_prod_batch(self.ring._h, self.pq._h, p, None, ptr, ptr, ptr, ptr, B)

    def check(self, p=2, B=3, ptr=None):
        return self.L.lolhip_rlwr_ring_check_batch(self.ring._h, self.pq._h, p, None, ptr, ptr, ptr, ptr, ptr, B)

    def work_len(self, kind, B, pq=True):
        return self.L.lolhip_rlwe_ring_work_len(self.ring._h, self.pq._h if pq is True else pq, kind, B)


@pytest.mark.parametrize("m,q", PAIRS)
def test_every_ring_pair_passes_the_host_checks(lolhip, m, q):
    assert not (rg.is_prime(q) and q % m == 1)
    assert lolhip.RingMul.moduli(m, [q]) == rg.rm.moduli(m, [q]) and len(rg.rm.moduli(m, [q])) == 1
    H = Handles(lolhip, m, q)
    assert H.K == 1 and not lolhip.lib().lolhip_plan_has_crt(H.pq._h)
    for kind in (rg.DISC, rg.CONT, rg.RLWR):
        for B in (1, 3):
            got = H.work_len(kind, B)
            assert got == rg.work_len(kind, B, H.n, H.K) > 0
    kinds = [k for k, mm, qq, _ in rg.challenge_lines() if (mm, qq) == (m, q)]
    assert kinds
    for kind in sorted(set(kinds)):
        assert H.sample(rg.KINDS[kind], p=2, svar=7.8125e-3) == ERR_NO_DEVICE, kind
    # the plan route refuses the same plan for want of a CRT basis
    L = lolhip.lib()
    assert L.lolhip_rlwe_sample_batch(H.pq._h, None, rg.RLWR, 2, None, 1.0, KEY, 0, None, None, None, 3) == ERR_NO_CRT


def test_status_table_and_its_order(lolhip):
    L = lolhip.lib()
    H = Handles(lolhip, 12, 105)
    other_index = lolhip.Plan.for_index(8, [105], host_only=True)
    other_q = lolhip.Plan.for_index(12, [104], host_only=True)
    two_moduli = lolhip.Plan.for_index(12, [105, 104], host_only=True)
    big_prime = Handles(lolhip, 23, 64)                       # beyond the sampler's prime limit
    # 1. INVALID, each cause alone, every other argument valid
    assert H.sample(rg.RLWR, h=None) == ERR_INVALID and H.sample(rg.RLWR, pq=None) == ERR_INVALID
    assert H.sample(3) == ERR_INVALID and H.sample(-1) == ERR_INVALID
    assert H.sample(rg.RLWR, B=-1) == ERR_INVALID
    for bad in (other_index, other_q, two_moduli):
        assert H.sample(rg.RLWR, pq=bad._h) == ERR_INVALID
        assert H.work_len(rg.RLWR, 3, pq=bad._h) == ERR_INVALID
    for p in (1, 0, -5, 105, 106):
        assert H.sample(rg.RLWR, p=p) == ERR_INVALID and H.rounded(p=p) == ERR_INVALID and H.check(p=p) == ERR_INVALID
    assert H.sample(rg.RLWR, p=104) == ERR_NO_DEVICE
    for svar in (0.0, -1.0, float("nan"), float("inf")):
        assert H.sample(rg.DISC, svar=svar) == ERR_INVALID and H.sample(rg.CONT, svar=svar) == ERR_INVALID
    assert H.sample(rg.RLWR, svar=float("nan")) == ERR_NO_DEVICE              # svar is not read for RLWR
    assert H.sample(rg.DISC, p=0) == ERR_NO_DEVICE                             # p is read for RLWR only
    assert big_prime.sample(rg.DISC) == ERR_INVALID and big_prime.sample(rg.CONT) == ERR_INVALID
    assert big_prime.error(rg.DISC) == ERR_INVALID and big_prime.error(rg.CONT) == ERR_INVALID
    assert big_prime.sample(rg.RLWR) == ERR_NO_DEVICE                          # RLWR has no sampler
    assert H.error(rg.RLWR) == ERR_INVALID and H.error(2) == ERR_INVALID and H.error(rg.DISC, B=-1) == ERR_INVALID
    assert H.rounded(B=-1) == ERR_INVALID and H.check(B=-1) == ERR_INVALID
    assert H.work_len(3, 1) == ERR_INVALID and H.work_len(rg.DISC, -1) == ERR_INVALID
    assert L.lolhip_rlwe_ring_work_len(None, H.pq._h, 0, 1) == ERR_INVALID
    # 2. NO_DEVICE comes before the NULL pointers (all of them are null here) and before B = 0's OK
    for B in (0, 3):
        assert H.sample(rg.DISC, B=B) == H.sample(rg.CONT, B=B) == H.sample(rg.RLWR, B=B) == ERR_NO_DEVICE
        assert H.error(rg.DISC, B=B) == H.error(rg.CONT, B=B) == ERR_NO_DEVICE
        assert H.rounded(B=B) == H.check(B=B) == ERR_NO_DEVICE
    # the secret: the plan check, then the device, then the pointers
    sec = lambda h, pq, key: L.lolhip_rlwe_ring_secret(h, pq, None, key, 0, None, None)
    assert sec(H.ring._h, other_q._h, KEY) == ERR_INVALID and sec(None, H.pq._h, KEY) == ERR_INVALID
    assert sec(H.ring._h, H.pq._h, None) == ERR_NO_DEVICE
    # work_len answers on host-only handles, 0 for an empty batch
    assert H.work_len(rg.DISC, 0) == 0 and H.work_len(rg.RLWR, 5) == rg.work_len(rg.RLWR, 5, H.n, H.K)


def test_a_modulus_with_a_crt_basis_is_accepted_too(lolhip):
    q = rg.good_prime(16, 1000)
    H = Handles(lolhip, 16, q)
    assert lolhip.lib().lolhip_plan_has_crt(H.pq._h) == 1
    assert H.sample(rg.DISC) == ERR_NO_DEVICE and H.work_len(rg.CONT, 2) == rg.work_len(rg.CONT, 2, 8, H.K)


def test_binding_and_switch_exist(lolhip):
    assert lolhip.RingRLWE.errorBound(256, 7.8125e-3, kind="disc") == lolhip.RLWE.errorBound(256, 7.8125e-3, kind="disc")
    L = lolhip.lib()
    assert L.lolhip_debug_set(b"RLWE_RING_UNFUSED", 1) == 0 and L.lolhip_debug_set(b"RLWE_RING_UNFUSED", 0) == 0
    r = lolhip.RingRLWE(lolhip.Plan.for_index(27, [81], host_only=True))
    assert r.K == 1 and r.ring.plan_Q.qs == rg.rm.moduli(27, [81])
    with pytest.raises(lolhip.NoDeviceError):
        r.sampleRLWR(np.zeros((18, 1), dtype=np.int64), 3, 3)


@pytest.mark.parametrize("m", [8, 12, 45])
def test_restatement_agrees_with_the_plan_route_on_a_crt_prime(cpuref, m):
    """x = lInv (a s): the ring route's restatement (exact product, integer L^-1) against the plan route's (pointwise in
    the CRT basis, crtInv, lInv of the CPU oracle), operands changed of basis by the oracle's crt"""
    q = rg.good_prime(m, 2 ** 20)
    P = Params(lm.factor_pps(m), [q])
    rng = np.random.default_rng(m)
    B = 3
    a_pow = rng.integers(0, q, size=(B, P.n), dtype=np.int64)
    s_pow = rng.integers(0, q, size=(P.n,), dtype=np.int64)
    a_crt = cpuref.crt(P, a_pow[..., None]).reshape(B, P.n)
    s_crt = cpuref.crt(P, s_pow[None, :, None]).reshape(P.n)
    prod = ((a_crt.astype(object) * s_crt.astype(object)[None]) % q).astype(np.int64)
    want = cpuref.linv(P, cpuref.crtinv(P, prod[..., None])).reshape(B, P.n)
    assert np.array_equal(rg.x_dec(m, q, a_pow, s_pow), want)
    # and L over the integers against the oracle's L mod q
    e = rng.integers(-50, 50, size=(B, P.n), dtype=np.int64)
    assert np.array_equal(rg.l_mod(m, e, q), cpuref.l(P, (e % q)[..., None]).reshape(B, P.n))
