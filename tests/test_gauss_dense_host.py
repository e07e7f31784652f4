"""Host side of the dense Gaussian stage (LOLHIP_PLAN_DENSE_GAUSS, include/lolhip.h): no GPU.

 - the flag, the route accessor and the table read-back in the ctypes table, with the header's types and constant;
 - host-only plans at m = 17, 23, 797 and 3 2^14: a default plan answers LOLHIP_ERR_INVALID from every sampler (the
   index is beyond its limits), an opted-in plan LOLHIP_ERR_NO_DEVICE (every host check passed) at the first three and
   still LOLHIP_ERR_INVALID at 3 2^14 (n = 16384 > 8192); unknown flag bits are refused;
 - rlwe-challenges' parameter list: with opted-in plans every one of the 516 lines passes the host checks of its route,
   with default plans exactly 136 do not;
 - the transposed table is the transpose of the table the plan already builds, and only the primes of the dense route
   have one.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rlwe_ring_ref as rg
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_NO_CRT, ERR_NO_DEVICE = 0, -1, -3, -5
KEY = bytes(range(32))
INDICES = [17, 23, 797, 3 * 2 ** 14]


def _plan(lolhip, m, dense, q=None):
    return lolhip.Plan.for_index(m, [q or lm.first_good_q(m, 1000)], host_only=True, dense_gauss=dense)


# ---- the binding ---------------------------------------------------------------------------------------------------------
def test_abi_rows_and_the_flag_constant():
    from lol_amd import _abi
    from test_abi_host import RETURNS, _ctypes_kind, prototypes
    header = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    protos = prototypes()
    for name in ("lolhip_plan_create_flags", "lolhip_plan_gauss_route", "lolhip_plan_gauss_table"):
        restype, argtypes = _abi.ABI[name]
        assert restype is RETURNS[protos[name][0]], name
        assert [_ctypes_kind(t) for t in argtypes] == protos[name][1], name
    assert protos["lolhip_plan_create_flags"][1] == ["ptr", "int", "ptr", "int", "int", "uint32_t", "ptr"]
    assert protos["lolhip_plan_gauss_route"] == ("int", ["ptr"])
    assert protos["lolhip_plan_gauss_table"] == ("int64_t", ["ptr", "int", "int", "ptr", "int64_t"])
    (value,) = re.findall(r"#define\s+LOLHIP_PLAN_DENSE_GAUSS\s+(\d+)u?\b", header)
    assert int(value) == _abi.PLAN_DENSE_GAUSS == 1
    import lol_amd.tensor as t
    assert t.PLAN_DENSE_GAUSS == 1


def test_flags_zero_is_the_default_creator_and_unknown_bits_are_refused(lolhip):
    L = lolhip.lib()
    _, arr, npp = lolhip.tensor._pps(lm.factor_pps(17))
    q = (C.c_int64 * 1)(103)
    for flags, rc, route in ((0, OK, 0), (1, OK, 2), (2, ERR_INVALID, None), (3, ERR_INVALID, None), (0x80000000, ERR_INVALID, None),
                             (0x80000001, ERR_INVALID, None)):
        h = C.c_void_p()
        assert L.lolhip_plan_create_flags(arr, npp, q, 1, 1, flags, C.byref(h)) == rc, flags
        assert bool(h) == (rc == OK)
        if h:
            assert L.lolhip_plan_gauss_route(h) == route
            L.lolhip_plan_destroy(h)
    assert L.lolhip_plan_gauss_route(None) == 0
    with pytest.raises(ValueError):
        lolhip.Plan.for_index(17, [103], host_only=True, dense_gauss=True, omega_pp=[1])


@pytest.mark.parametrize("m,default,opted", [(17, 0, 2), (23, 0, 2), (797, 0, 2), (3 * 2 ** 14, 0, 0), (45, 1, 1), (2 ** 13 * 3, 1, 1),
                                             (2 ** 14, 1, 1), (51, 0, 2), (2 ** 10 * 17, 0, 2), (2 ** 11 * 17, 0, 0)])
def test_route_is_a_function_of_the_index_and_the_flag(lolhip, m, default, opted):
    """0 refused, 1 register stages only, 2 a dense stage: n <= 8192 on either plan, primes <= 13 on a default plan and
    any prime a prime-power list can hold (they are int16: below 2^15) on an opted-in one."""
    assert _plan(lolhip, m, False, q=12289).gaussRoute() == default
    assert _plan(lolhip, m, True, q=12289).gaussRoute() == opted


# ---- statuses ------------------------------------------------------------------------------------------------------------
def _sampler_statuses(lolhip, m, dense):
    """name -> status of every sampler entry over host-only plans of index m (B = 0 or null pointers: the host checks
    answer before either is looked at)"""
    L = lolhip.lib()
    pq = _plan(lolhip, m, dense)
    assert pq.has_crt
    pp = lolhip.Plan.for_index(m, [16], host_only=True, dense_gauss=dense)
    h = pq._h
    return {
        "sample disc": L.lolhip_rlwe_sample_batch(h, None, 0, 4, None, 1.0, KEY, 0, None, None, None, 0),
        "sample cont": L.lolhip_rlwe_sample_batch(h, None, 1, 4, None, 1.0, KEY, 0, None, None, None, 0),
        "encrypt": L.lolhip_encrypt_batch(h, pp._h, None, None, None, None, 1.0, KEY, 0, 0, None, None, 0),
        "errorRounded": L.lolhip_error_rounded_batch(h, None, 1.0, KEY, 0, None, None, 0),
        "ksHint": L.lolhip_kshint_batch(h, None, None, None, 1.0, 0, KEY, 0, None, None, 0),
        "challenge disc": L.lolhip_chall_generate_batch(h, None, 0, 4, 1.0, KEY, 0, 0, 2, 2, None, None, None, None),
        "challenge cont": L.lolhip_chall_generate_batch(h, None, 1, 4, 1.0, KEY, 0, 0, 2, 2, None, None, None, None),
    }


@pytest.mark.parametrize("m", INDICES)
def test_default_plans_refuse_the_index_and_opted_in_plans_only_lack_a_device(lolhip, m):
    got = _sampler_statuses(lolhip, m, False)
    assert set(got.values()) == {ERR_INVALID}, got
    got = _sampler_statuses(lolhip, m, True)
    assert set(got.values()) == {ERR_INVALID if m == 3 * 2 ** 14 else ERR_NO_DEVICE}, got
    # gaussianDec itself asks for the device first, as before; RLWR has no sampler on either plan
    L = lolhip.lib()
    for dense in (False, True):
        pq = _plan(lolhip, m, dense)
        assert L.lolhip_gaussian_dec_batch(pq._h, None, None, 0) == ERR_NO_DEVICE
        assert L.lolhip_rlwe_sample_batch(pq._h, None, 2, 4, None, 1.0, KEY, 0, None, None, None, 0) == ERR_NO_DEVICE
        assert L.lolhip_crtc_batch(pq._h, None, None, 0) == ERR_NO_DEVICE


# ---- the challenge list --------------------------------------------------------------------------------------------------
def _generate_status(lolhip, cache, kind, m, q, arg, dense):
    """the status of the whole-challenge generate entry of the line's route over host-only handles"""
    L = lolhip.lib()
    if (m, q) not in cache:
        pq = lolhip.Plan.for_index(m, [q], host_only=True, dense_gauss=dense)
        cache[(m, q)] = (pq, None if pq.has_crt else lolhip.RingMul(pq))
    pq, ring = cache[(m, q)]
    p, svar = (int(arg), 1.0) if kind == "RLWR" else (0, float(arg))
    if ring is None:
        return L.lolhip_chall_generate_batch(pq._h, None, rg.KINDS[kind], p, svar, KEY, 0, 0, 2, 3, None, None, None, None)
    return L.lolhip_chall_ring_generate_batch(ring._h, pq._h, None, rg.KINDS[kind], p, svar, KEY, 0, 0, 2, 3, None, None, None, None)


def test_the_challenge_list_is_served_in_full_by_opted_in_plans(lolhip):
    lines = rg.challenge_lines()
    assert len(lines) == 516
    for dense, refused in ((True, 0), (False, 136)):
        cache = {}
        status = [_generate_status(lolhip, cache, kind, m, q, arg, dense) for kind, m, q, arg in lines]
        assert set(status) <= {ERR_NO_DEVICE, ERR_INVALID}
        bad = [ln for ln, st in zip(lines, status) if st != ERR_NO_DEVICE]
        assert len(bad) == refused
        # the refused lines are the Cont and Disc lines at a prime above 13 (RLWR has no sampler)
        assert all(kind in ("Cont", "Disc") and max(p for p, _ in lm.factor_pps(m)) > 13 for kind, m, _, _ in bad)
        assert not bad or sorted({m for _, m, _, _ in bad}) == [179, 257, 797]


def test_challenges_module_opts_in_for_cont_and_disc(lolhip):
    from lol_amd import challenges as ch
    recs = {r.challID: r for r in ch.parse_params(open(os.path.join(ROOT, "tests", "golden", "challenge_params.txt")).read())}
    cp = recs[287]
    assert (cp.kind, cp.m, cp.q) == ("Disc", 179, 2048)
    which, plan = ch.route(cp)
    assert which == "ring" and plan.gaussRoute() == 0 and not plan.dense_gauss         # what route returns today
    which, plan = ch.route(cp, dense_gauss=True)
    assert which == "ring" and plan.gaussRoute() == 2 and plan.host_only


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [17, 51, 289, 323, 797, 2 ** 9 * 17])
def test_transposed_table_is_the_transpose(lolhip, m):
    pps = lm.factor_pps(m)
    P, D = _plan(lolhip, m, True, q=12289), _plan(lolhip, m, False, q=12289)
    for k, (p, _) in enumerate(pps):
        M, Mt = P.gaussTable(k), P.gaussTable(k, transposed=True)
        if p == 2:
            assert M.size == Mt.size == 0
            continue
        assert M.shape == (p - 1, p - 1)
        assert np.array_equal(M.view(np.int64), D.gaussTable(k).view(np.int64))      # the flag leaves the matrix as it was
        assert D.gaussTable(k, transposed=True).size == 0                            # a default plan builds no copy
        if p <= 13:
            assert Mt.size == 0                                                      # register stage: no copy either
            continue
        assert np.array_equal(Mt.view(np.int64), np.ascontiguousarray(M.T).view(np.int64))
        # and the matrix is the reference's: 2 cos / 2 sin of 2 pi (row col mod p) / p, col = 1 .. p - 1
        row, col = np.meshgrid(np.arange(p - 1), np.arange(1, p), indexing="ij")
        ang = 2.0 * math.pi * ((row * col) % p) / p
        want = 2.0 * np.where(col <= p // 2, np.cos(ang), np.sin(ang))
        assert np.abs(M - want).max() <= 4 * 2.0 ** -52
    L = lolhip.lib()
    assert L.lolhip_plan_gauss_table(P._h, len(pps), 0, None, 0) == L.lolhip_plan_gauss_table(P._h, -1, 1, None, 0) == 0
    assert L.lolhip_plan_gauss_table(None, 0, 0, None, 0) == 0
    k = len(pps) - 1
    d = pps[k][0] - 1
    short = np.full(d + 3, 7.0)
    assert L.lolhip_plan_gauss_table(P._h, k, 1, short.ctypes.data_as(C.POINTER(C.c_double)), d) == d * d
    assert np.array_equal(short[:d], P.gaussTable(k, transposed=True).ravel()[:d]) and (short[d:] == 7.0).all()
