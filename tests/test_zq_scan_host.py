"""Host side of the scan route of the prime ops (LOLHIP_ROUTE_SCAN_ZQ, include/lolhip.h): no GPU.

 - the new query, the constant, the switch and the two hooks in the header, with the ctypes row;
 - lolhip_plan_create_opts accepts the bit with every defined flag and route beside it, lolhip_plan_create_routes keeps
   refusing it, the value 2 stays undefined;
 - lolhip_plan_scan_route on host-only plans against a restatement of the rule: opted in, GENERIC_SCALAR off,
   n <= 8192, a prime above 13 in the index (the programs of such an index go to the scalar interpreter); ZQ_SCAN drops
   the prime condition;
 - an opted-in plan is otherwise the plan without the bit: the same tables, programs and sibling routes;
 - rlwe-challenges' parameter list: lol_amd.challenges opts in at exactly the 144 lines whose index has a prime above 13.
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import rlwe_ring_ref as rg
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_NO_DEVICE = 0, -1, -5
OPS = range(4, 10)                 # LOLHIP_OP_L ... LOLHIP_OP_DIVGDEC


def _plan(lolhip, m, qs=None, scan=True, **kw):
    return lolhip.Plan.for_index(m, qs or [lm.first_good_q(m, 1000)], host_only=True, scan_zq=scan, **kw)


def _rule(m, scan=True, scalar=False, forced=False):
    """lolhip_plan_scan_route of any of the six ops by the documented rule.  An index with a prime above 13 is refused by
    the vector interpreter whatever the moduli, so the moduli do not enter; an index without an odd prime has no
    prime-op stage at all."""
    pps = lm.factor_pps(m)
    odd = [p for p, _ in pps if p != 2]
    if not scan or scalar or lm.totient_pps(pps) > 8192 or not odd:
        return 0
    return 1 if forced or max(odd) > 13 else 0


def _routes(P):
    return [P.scanRoute(op) for op in OPS]


# ---- the binding ---------------------------------------------------------------------------------------------------------
def test_header_names_and_the_abi_row():
    from lol_amd import _abi
    from test_abi_host import RETURNS, _ctypes_kind, prototypes
    header = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    protos = prototypes()
    restype, argtypes = _abi.ABI["lolhip_plan_scan_route"]
    assert restype is RETURNS[protos["lolhip_plan_scan_route"][0]]
    assert [_ctypes_kind(t) for t in argtypes] == protos["lolhip_plan_scan_route"][1]
    assert protos["lolhip_plan_scan_route"] == ("int", ["ptr", "int"])
    (value,) = re.findall(r"#define\s+LOLHIP_ROUTE_SCAN_ZQ\s+(\d+)u?\b", header)
    assert int(value) == _abi.ROUTE_SCAN_ZQ == 4
    import lol_amd.tensor as t
    assert t.ROUTE_SCAN_ZQ == 4
    assert re.search(r"\bZQ_SCAN\b", header) and "LOLHIP_ZQ_SCAN_INFO" in header and "LOLHIP_ZQ_SCAN_GRID" in header


def test_the_creators(lolhip):
    L = lolhip.lib()
    Opts = lolhip.tensor._PlanOpts
    assert C.sizeof(Opts) == 12
    _, arr, npp = lolhip.tensor._pps(lm.factor_pps(17))
    q = (C.c_int64 * 1)(103)
    for routes in (4, 5):
        for flags in range(4):
            h = C.c_void_p()
            opts = Opts(12, flags, routes)
            assert L.lolhip_plan_create_opts(arr, npp, q, 1, 1, C.byref(opts), C.byref(h)) == OK and h, (flags, routes)
            assert [L.lolhip_plan_scan_route(h, op) for op in OPS] == [1] * 6
            assert L.lolhip_plan_zq_route(h, 0) == routes & 1 and L.lolhip_plan_gauss_route(h) == (2 if flags & 1 else 0)
            L.lolhip_plan_destroy(h)
        h = C.c_void_p()
        assert L.lolhip_plan_create_routes(arr, npp, q, 1, 1, 0, routes, C.byref(h)) == ERR_INVALID and not h
    for routes in (2, 3, 6, 7, 8, 0x80000004):                 # 2 stays undefined, with or without the new bit
        h = C.c_void_p()
        opts = Opts(12, 0, routes)
        assert L.lolhip_plan_create_opts(arr, npp, q, 1, 1, C.byref(opts), C.byref(h)) == ERR_INVALID and not h, routes
    h = C.c_void_p()
    opts = Opts(12, 0, 1)                                      # without the bit: no scan anywhere
    assert L.lolhip_plan_create_opts(arr, npp, q, 1, 1, C.byref(opts), C.byref(h)) == OK
    assert [L.lolhip_plan_scan_route(h, op) for op in OPS] == [0] * 6
    # arguments out of range
    assert [L.lolhip_plan_scan_route(h, op) for op in (-1, 0, 1, 2, 3, 10, 11, 12, 1 << 20)] == [0] * 9
    L.lolhip_plan_destroy(h)
    assert L.lolhip_plan_scan_route(None, 4) == 0
    with pytest.raises(ValueError):
        lolhip.Plan.for_index(17, [103], host_only=True, scan_zq=True, omega_pp=[1])
    with pytest.raises(ValueError):
        lolhip.Plan.for_index(17, [103], host_only=True, scan_zq=True, mhatinv=[1])


# ---- the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [17, 34, 136, 221, 289, 323, 797, 15015, 2 ** 10, 2 ** 11 * 17, 2 ** 14 * 3, 7 * 13, 45])
def test_scan_route_of_host_only_plans(lolhip, m):
    n = lm.totient_pps(lm.factor_pps(m))
    for qs in ([lm.first_good_q(m, 1000)], [lm.first_good_q(m, 2 ** 58)], [lm.first_good_q(m, 2 ** 20), lm.first_good_q(m, 2 ** 40)]):
        P, D = _plan(lolhip, m, qs), _plan(lolhip, m, qs, scan=False)
        assert P.scan_zq and not D.scan_zq
        assert _routes(P) == [_rule(m)] * 6, (m, qs)
        assert _routes(D) == [0] * 6, (m, qs)
        assert [P.scanRoute(op) for op in (-1, 0, 3, 10, 11, 12)] == [0] * 6
    assert (_rule(m) == 1) == (m in (17, 34, 136, 221, 289, 323, 797))
    assert (n > 8192) == (m in (2 ** 11 * 17, 2 ** 14 * 3))


def test_moduli_without_a_crt_basis_and_up_to_16(lolhip):
    for q in (2 ** 20, 2, 16, 17, 2 ** 40 + 2):
        P = _plan(lolhip, 17, [q])
        assert not P.has_crt and _routes(P) == [1] * 6, q
    P = _plan(lolhip, 221, [2 ** 20, 16])
    assert not P.has_crt and _routes(P) == [1] * 6
    # primes up to 13 over a modulus <= 16 stay on the scalar interpreter: the rule asks for a prime above 13
    assert _routes(_plan(lolhip, 45, [8])) == [0] * 6


def test_switches_move_the_answer(lolhip):
    big, small, two, off = _plan(lolhip, 257), _plan(lolhip, 7 * 13), _plan(lolhip, 64), _plan(lolhip, 7 * 13, scan=False)
    long = _plan(lolhip, 2 ** 14 * 3)
    assert (_routes(big), _routes(small)) == ([1] * 6, [0] * 6)
    try:
        lolhip.debug_set("ZQ_SCAN", True)
        assert _routes(big) == _routes(small) == _routes(_plan(lolhip, 45)) == [1] * 6
        assert _routes(two) == _routes(off) == _routes(long) == [0] * 6         # no odd prime; not opted in; n > 8192
        assert all(_routes(_plan(lolhip, m)) == [_rule(m, forced=True)] * 6 for m in (3, 12, 15015, 2 ** 11 * 17))
        lolhip.debug_set("GENERIC_SCALAR", True)                                  # wins over it
        assert _routes(big) == _routes(small) == [0] * 6
        lolhip.debug_set("ZQ_SCAN", False)
        assert _routes(big) == [_rule(257, scalar=True)] * 6 == [0] * 6
    finally:
        lolhip.debug_set("ZQ_SCAN", False)
        lolhip.debug_set("GENERIC_SCALAR", False)
    assert (_routes(big), _routes(small)) == ([1] * 6, [0] * 6)


def test_an_opted_in_plan_is_otherwise_the_plan_without_the_bit(lolhip):
    for m in (17, 51, 289, 221, 544, 45):
        qs = [lm.first_good_q(m, 2 ** 26)]
        for kw in ({}, {"dense_zq": True, "dense_gauss": True, "dense_cplx": True}):
            P, D = _plan(lolhip, m, qs, **kw), _plan(lolhip, m, qs, scan=False, **kw)
            for inv in (False, True):
                assert np.array_equal(P.program(inv), D.program(inv))
            assert all(np.array_equal(P._table(w), D._table(w)) for w in (2, 3, 4, 5, 10, 11, 12))
            assert all(np.array_equal(P._table(w, k), D._table(w, k)) for w in (0, 1) for k in range(len(P.pps)))
            assert [P.zqRoute(w) for w in range(4)] == [D.zqRoute(w) for w in range(4)] and P.zqRoute(3) == 0
            assert (P.gaussRoute(), P.cplxRoute()) == (D.gaussRoute(), D.cplxRoute())
            assert (P.n, P.m, P.T, P.has_crt) == (D.n, D.m, D.T, D.has_crt)


def test_compute_calls_of_host_only_plans_need_a_device(lolhip):
    L = lolhip.lib()
    P = _plan(lolhip, 257)
    for name in ("l", "linv", "mulgpow", "mulgdec", "divgpow", "divgdec"):
        assert getattr(L, f"lolhip_{name}_batch")(P._h, None, None, 0) == ERR_NO_DEVICE


def test_ringmul_hands_the_option_on(lolhip):
    P = _plan(lolhip, 17, [2 ** 20])
    assert lolhip.RingMul(P).plan_Q.scan_zq and _routes(lolhip.RingMul(P).plan_Q) == [1] * 6
    assert not lolhip.RingMul(P, scan_zq=False).plan_Q.scan_zq
    D = _plan(lolhip, 17, [2 ** 20], scan=False)
    assert not lolhip.RingMul(D).plan_Q.scan_zq and lolhip.RingMul(D, scan_zq=True).plan_Q.scan_zq


# ---- the challenge list --------------------------------------------------------------------------------------------------
def test_challenge_plans_opt_in_at_the_large_prime_lines(lolhip):
    from lol_amd import challenges as ch
    lines = rg.challenge_lines()
    assert len(lines) == 516
    cache, scans = {}, []
    for kind, m, q, _ in lines:
        if (m, q) not in cache:
            which, plan = ch.route(SimpleNamespace(m=m, q=q))
            side = plan if which == "plan" else lolhip.RingMul(plan).plan_Q
            assert plan.scan_zq == side.scan_zq == ch.large_prime(m)
            cache[(m, q)] = min(_routes(plan) + _routes(side))
        scans.append(cache[(m, q)])
    large = [max(p for p, _ in lm.factor_pps(m)) > 13 for _, m, _, _ in lines]
    assert sum(large) == 144 and len(large) - sum(large) == 372
    assert [r == 1 for r in scans] == large
