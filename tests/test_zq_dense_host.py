"""Host side of the dense Z_q stages (LOLHIP_ROUTE_DENSE_ZQ, include/lolhip.h): no GPU.

 - the creator, the two queries and the constant in the ctypes table, with the header's types;
 - routes = 0 is lolhip_plan_create_flags; undefined route bits are refused, and so are the flag bits that were;
 - lolhip_plan_zq_route on host-only plans against the documented rule: opted in, n <= 8192, a prime above 13 in the
   program a lone transform launches, GENERIC_SCALAR off; the matrix cores (2) where every modulus fits W <= 4 balanced
   base-256 limbs and the longest dense vector has at least 48 elements, else the vector ALU (1); ZQ_DENSE_VALU;
 - the limb thresholds 65279 / 16711423 / 4278124287, exactly, at m = 257;
 - the tables: the limb planes recombine to the centred residue of the plan's own matrix, their padding is zero, the
   transposed copy is the transpose, short buffers return the count;
 - rlwe-challenges' parameter list: the plans lol_amd.challenges builds report a dense route at exactly the 144 lines
   whose index has a prime above 13.
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import rlwe_ring_ref as rg
from oracle import lolmath as lm
from saturate import good_below

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_NO_DEVICE = 0, -1, -5
W_TOPS = (65279, 16711423, 4278124287)           # floor(q/2) <= 127 (256^W - 1) / 255 for W = 2, 3, 4
MFMA_MIN_D = 48


def _plan(lolhip, m, qs=None, dense=True, **kw):
    return lolhip.Plan.for_index(m, qs or [lm.first_good_q(m, 1000)], host_only=True, dense_zq=dense, **kw)


def _limbs(q):
    """the documented W: the least count of balanced base-256 limbs holding floor(q/2), at least 2; None above 4"""
    w = 2
    while q // 2 > 127 * (256 ** w - 1) // 255:
        w += 1
    return w if w <= 4 else None


def _rule(m, qs):
    """lolhip_plan_zq_route(what = 0 or 1) of an opted-in plan by the documented rule"""
    pps = lm.factor_pps(m)
    n = lm.totient_pps(pps)
    big = [p for p, _ in pps if p > 13]
    if not big or n > 8192:
        return 0
    dmax = max(p if e > 1 else p - 1 for p, e in pps if p > 13)      # a prime power adds DFT_p stages of length p
    return 2 if all(_limbs(q) for q in qs) and dmax >= MFMA_MIN_D else 1


def _rule_polymul(m, qs):
    """lolhip_plan_zq_route(what = 2): one launch on the transforms' route when the stage programs alone make the transform
    (no 2-power part with kernels of its own, e >= 5), 4 n words fit 152 KiB of LDS, and a 64 KiB tile leaves the inverse
    program a whole register tile of columns (32 on the matrix cores, 8 / 4 on the vector ALU at 4- / 8-byte words); else 0"""
    pps = lm.factor_pps(m)
    n = lm.totient_pps(pps)
    if pps[0][0] == 2 and pps[0][1] >= 5:
        return 0
    word = 4 if max(qs) < 2 ** 32 else 8
    route = _rule(m, qs)
    if not route or 4 * n * word > 152 * 1024:
        return 0
    dmax = max(p if e > 1 else p - 1 for p, e in pps if p > 13)
    cols = max(1, 64 * 1024 // (4 * n * word)) * (n // dmax)
    return route if cols >= (32 if route == 2 else 8 if word == 4 else 4) else 0


# ---- the binding ---------------------------------------------------------------------------------------------------------
def test_abi_rows_and_the_route_constant():
    from lol_amd import _abi
    from test_abi_host import RETURNS, _ctypes_kind, prototypes
    header = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    protos = prototypes()
    for name in ("lolhip_plan_create_routes", "lolhip_plan_zq_route", "lolhip_plan_zq_table"):
        restype, argtypes = _abi.ABI[name]
        assert restype is RETURNS[protos[name][0]], name
        assert [_ctypes_kind(t) for t in argtypes] == protos[name][1], name
    assert protos["lolhip_plan_create_routes"] == ("int", ["ptr", "int", "ptr", "int", "int", "uint32_t", "uint32_t", "ptr"])
    assert protos["lolhip_plan_zq_route"] == ("int", ["ptr", "int"])
    assert protos["lolhip_plan_zq_table"] == ("int64_t", ["ptr", "int", "int", "int", "int", "ptr", "int64_t"])
    (value,) = re.findall(r"#define\s+LOLHIP_ROUTE_DENSE_ZQ\s+(\d+)u?\b", header)
    assert int(value) == _abi.ROUTE_DENSE_ZQ == 1
    import lol_amd.tensor as t
    assert t.ROUTE_DENSE_ZQ == 1
    assert "ZQ_DENSE_VALU" in header and "ZQ_DENSE_MFMA" in header and "LOLHIP_ZQ_DENSE_INFO" in header and "LOLHIP_ZQ_DENSE_GRID" in header


def test_routes_zero_is_create_flags_and_unknown_bits_are_refused(lolhip):
    L = lolhip.lib()
    _, arr, npp = lolhip.tensor._pps(lm.factor_pps(17))
    q = (C.c_int64 * 1)(103)
    for flags, routes, rc, gauss, zq in ((0, 0, OK, 0, 0), (1, 0, OK, 2, 0), (0, 1, OK, 0, 1), (1, 1, OK, 2, 1), (0, 2, ERR_INVALID, 0, 0),
                                         (0, 3, ERR_INVALID, 0, 0), (0, 0x80000000, ERR_INVALID, 0, 0), (1, 0x80000001, ERR_INVALID, 0, 0),
                                         (2, 1, ERR_INVALID, 0, 0), (3, 0, ERR_INVALID, 0, 0)):
        h = C.c_void_p()
        assert L.lolhip_plan_create_routes(arr, npp, q, 1, 1, flags, routes, C.byref(h)) == rc, (flags, routes)
        assert bool(h) == (rc == OK)
        if h:
            assert L.lolhip_plan_gauss_route(h) == gauss
            assert [L.lolhip_plan_zq_route(h, w) for w in (0, 1, 2, 3, -1)] == [zq, zq, zq, 0, 0]
            L.lolhip_plan_destroy(h)
    for flags in (2, 3, 0x80000000):                      # the flag word of the older creator is what it was
        h = C.c_void_p()
        assert L.lolhip_plan_create_flags(arr, npp, q, 1, 1, flags, C.byref(h)) == ERR_INVALID and not h
    assert L.lolhip_plan_zq_route(None, 0) == 0
    assert L.lolhip_plan_zq_table(None, 0, 0, 0, -1, None, 0) == 0
    with pytest.raises(ValueError):
        lolhip.Plan.for_index(17, [103], host_only=True, dense_zq=True, omega_pp=[1])


def test_a_route_changes_no_table_and_no_program(lolhip):
    for m in (17, 51, 289, 153, 544, 45):
        qs = [lm.first_good_q(m, 2 ** 26)]
        P, D = _plan(lolhip, m, qs), _plan(lolhip, m, qs, dense=False)
        assert P.dense_zq and not D.dense_zq
        for inv in (False, True):
            assert np.array_equal(P.program(inv), D.program(inv))
            assert np.array_equal(P.program(inv, polymul=True), D.program(inv, polymul=True))
        assert all(np.array_equal(P._table(w), D._table(w)) for w in (2, 3, 4, 5, 12))
        assert P.gaussRoute() == D.gaussRoute()


# ---- the route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [17, 19, 51, 221, 289, 323, 68, 544, 2 ** 9 * 17, 797, 179, 257, 67, 4913, 7429, 2 ** 10 * 17,
                               45, 2 ** 10, 2 ** 11 * 17, 3 * 2 ** 14])
def test_route_of_host_only_plans(lolhip, m):
    n = lm.totient_pps(lm.factor_pps(m))
    for qs in ([lm.first_good_q(m, 1000)], [lm.first_good_q(m, 2 ** 20)], [good_below(m, 2 ** 32)], [lm.first_good_q(m, 2 ** 58)],
               [lm.first_good_q(m, 2 ** 20), lm.first_good_q(m, 2 ** 40)]):
        P, D = _plan(lolhip, m, qs), _plan(lolhip, m, qs, dense=False)
        want = _rule(m, qs)
        assert [P.zqRoute(w) for w in range(3)] == [want, want, _rule_polymul(m, qs)], (m, qs)
        assert [D.zqRoute(w) for w in range(3)] == [0, 0, 0], (m, qs)
    assert (_rule(m, [lm.first_good_q(m, 1000)]) > 0) == (m not in (45, 2 ** 10, 2 ** 11 * 17, 3 * 2 ** 14))
    assert m != 2 ** 10 * 17 or n == 8192           # the largest n the route takes; 2^11 * 17 (n = 16384) is beyond it


def test_polymul_takes_one_launch_on_either_side_of_the_lds_limit(lolhip):
    """4 n words: two operands, two ping-pong buffers.  4-byte words fit at every n <= 8192; 8-byte words up to n = 4864:
    17^3 (n = 4624) fits, 17^2 19 (n = 4896) does not, nor 17 19 23 (n = 6336).  The split route (2^e, e >= 5) stays composed,
    and so does a tile too small for the inverse program: m = 257 on the matrix cores (16 columns of 32), m = 797 at 8-byte
    words (2 of 4)."""
    q20, q58 = (lambda m: [lm.first_good_q(m, 2 ** 20)]), (lambda m: [lm.first_good_q(m, 2 ** 58)])
    for m, qs, want in ((4913, q58(4913), 1), (5491, q58(5491), 0), (7429, q58(7429), 0), (4913, q20(4913), 1), (5491, q20(5491), 1),
                        (7429, q20(7429), 1), (97, q20(97), 2), (257, q20(257), 0), (257, q58(257), 1), (797, q58(797), 0), (2 ** 4 * 17, q20(272), 1), (544, q20(544), 0),
                        (2 ** 7 * 67, q20(2 ** 7 * 67), 0)):
        P = _plan(lolhip, m, qs)
        assert 4 * P.n * (4 if qs[0] < 2 ** 32 else 8) <= 152 * 1024 or want == 0
        assert P.zqRoute(2) == want == _rule_polymul(m, qs), (m, qs)
        assert P.zqRoute(0) >= 1 and _plan(lolhip, m, qs, dense=False).zqRoute(2) == 0
    P = _plan(lolhip, 4913, q58(4913))
    try:
        lolhip.debug_set("POLYMUL_UNFUSED", True)
        assert P.zqRoute(2) == 0 and P.zqRoute(0) == 1
    finally:
        lolhip.debug_set("POLYMUL_UNFUSED", False)


def test_no_crt_basis_no_route(lolhip):
    P = _plan(lolhip, 17, [2048])
    assert not P.has_crt and [P.zqRoute(w) for w in range(3)] == [0, 0, 0] and P.zqTable(0).size == 0


@pytest.mark.parametrize("m", [17, 257])
def test_limb_thresholds_exactly(lolhip, m):
    """The largest good prime up to each top and the first above it: W = 2 / 3 / 4 limb planes, none above the last top.
    m = 257 (d = 256) takes the matrix cores below the last top and the vector ALU above it; m = 17 (d = 16 < 48) builds
    the same planes and stays on the vector ALU, where it measured faster."""
    dp = (m - 1 + 31) // 32 * 32
    for W, top in zip((2, 3, 4), W_TOPS):
        below, above = good_below(m, top + 1), lm.first_good_q(m, top)
        assert below <= top < above and _limbs(below) == W and _limbs(above) == (W + 1 if W < 4 else None)
        for q, w in ((below, W), (above, W + 1)):
            P = _plan(lolhip, m, [q])
            assert P.zqRoute(0) == P.zqRoute(1) == (2 if w <= 4 and m == 257 else 1), q
            planes = [P.zqTable(0, limb=k).size for k in range(6)]
            assert planes == [dp * dp if (w <= 4 and k < w) else 0 for k in range(6)], (q, planes)
    if m == 17:
        return
    # one wide modulus sends the whole plan to the vector ALU, and no plane is built
    P = _plan(lolhip, m, [good_below(m, 65280), lm.first_good_q(m, W_TOPS[2])])
    assert P.zqRoute(0) == P.zqRoute(1) == 1 and P.zqTable(0, limb=0).size == 0 and P.zqTable(0, t=1).shape == (256, 256)
    # one W for the plan: the largest of its components
    P = _plan(lolhip, m, [good_below(m, 65280), good_below(m, W_TOPS[1] + 1)])
    assert P.zqRoute(0) == 2 and [P.zqTable(0, t=0, limb=k).size > 0 for k in range(4)] == [True, True, True, False]


def test_switches_move_the_answer(lolhip):
    P, S = _plan(lolhip, 257), _plan(lolhip, 17)
    assert (P.zqRoute(0), S.zqRoute(0)) == (2, 1)
    try:
        lolhip.debug_set("ZQ_DENSE_VALU", True)
        assert (P.zqRoute(0), P.zqRoute(1), S.zqRoute(0)) == (1, 1, 1)
        lolhip.debug_set("GENERIC_SCALAR", True)
        assert (P.zqRoute(0), P.zqRoute(1), S.zqRoute(0)) == (0, 0, 0)
        assert P.zqTable(0).size == 0                              # not dense now
        lolhip.debug_set("ZQ_DENSE_VALU", False)
        assert P.zqRoute(0) == 0
        lolhip.debug_set("GENERIC_SCALAR", False)
        lolhip.debug_set("ZQ_DENSE_MFMA", True)                   # lifts the length condition, not the limb condition
        wide = _plan(lolhip, 17, [lm.first_good_q(17, W_TOPS[2])])
        assert (P.zqRoute(0), S.zqRoute(0), S.zqRoute(1), wide.zqRoute(0)) == (2, 2, 2, 1)
        lolhip.debug_set("ZQ_DENSE_VALU", True)                   # wins over it
        assert (P.zqRoute(0), S.zqRoute(0)) == (1, 1)
    finally:
        for name in ("ZQ_DENSE_VALU", "ZQ_DENSE_MFMA", "GENERIC_SCALAR"):
            lolhip.debug_set(name, False)
    assert (P.zqRoute(0), S.zqRoute(0)) == (2, 1)


def test_compute_calls_of_host_only_plans_need_a_device(lolhip):
    L = lolhip.lib()
    for m in (17, 257):
        P = _plan(lolhip, m)
        assert L.lolhip_crt_batch(P._h, None, None, 0) == ERR_NO_DEVICE
        assert L.lolhip_crtinv_batch(P._h, None, None, 0) == ERR_NO_DEVICE
        assert L.lolhip_polymul_batch(P._h, None, None, None, None, 0) == ERR_NO_DEVICE


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [17, 19, 37, 289, 67, 2 ** 4 * 17])
def test_tables_recombine_to_the_plans_matrix(lolhip, cpuref, m):
    """The dense copies of every dense stage of both programs.  The limb planes recombine (sum of 256^w limb_w) to the
    centred residues of the transposed copy's transpose, with zero padding; at a prime index the forward program is the
    one stage, so its matrix is the transform of the unit vectors, which the CPU oracle computes from the same roots,
    and the inverse stage times the forward one is a multiple of the identity."""
    from oracle.oracle import Params
    qs = [lm.first_good_q(m, 1000), lm.first_good_q(m, 2 ** 20)]       # W = 2 and W = 3 components: W = 3 for the plan
    assert [_limbs(q) for q in qs] == [2, 3]
    P = _plan(lolhip, m, qs)
    assert P.zqRoute(0) >= 1
    R = Params(lm.factor_pps(m), qs)
    first = {}
    for inv in (False, True):
        prog = P.program(inv)
        dense = [i for i, st in enumerate(prog) if st[0] in (1, 2, 3) and st[1] > 13]
        assert dense
        for i in range(len(prog)):
            if i not in dense:
                assert P.zqTable(i, inverse=inv).size == 0 and P.zqTable(i, limb=0, inverse=inv).size == 0
        for i in dense:
            d = int(prog[i][2])
            dp = (d + 31) // 32 * 32
            for t, q in enumerate(qs):
                Mt = P.zqTable(i, t=t, inverse=inv)
                assert Mt.shape == (d, d) and Mt.min() >= 0 and Mt.max() < q
                planes = [P.zqTable(i, t=t, limb=w, inverse=inv) for w in range(3)]
                assert all(pl.shape == (dp, dp) and pl.min() >= -128 and pl.max() <= 127 for pl in planes)
                full = sum(256 ** w * planes[w] for w in range(3))
                assert not full[d:].any() and not full[:, d:].any()                           # zero padding
                assert np.array_equal(full[:d, :d], np.where(Mt.T > q // 2, Mt.T - q, Mt.T))  # row-major, centred
                assert P.zqTable(i, t=t, limb=3, inverse=inv).size == 0
                first.setdefault((inv, t), Mt.T)
    if m in (17, 19, 37, 67):
        d = m - 1
        eye = np.zeros((d, d, len(qs)), dtype=np.int64)
        eye[np.arange(d), np.arange(d), :] = 1
        cols = cpuref.crt(R, eye)                                       # row c = transform of e_c = column c of the matrix
        for t, q in enumerate(qs):
            assert np.array_equal(first[(False, t)].T, cols[:, :, t])
            prod = (first[(True, t)] @ first[(False, t)]) % q           # entries < 2^40 * d
            assert prod[0, 0] != 0 and np.array_equal(prod, prod[0, 0] * np.eye(d, dtype=np.int64))
        # short buffers: the count comes back, the tail stays
        L = lolhip.lib()
        short = np.full(d + 3, 7, dtype=np.int64)
        ptr = short.ctypes.data_as(C.POINTER(C.c_int64))
        for limb, count in ((-1, d * d), (0, ((d + 31) // 32 * 32) ** 2)):
            short[:] = 7
            assert L.lolhip_plan_zq_table(P._h, 0, 0, 0, limb, ptr, d) == count
            assert np.array_equal(short[:d], P.zqTable(0, limb=limb).ravel()[:d]) and (short[d:] == 7).all()
            short[:] = 7
            assert L.lolhip_plan_zq_table(P._h, 0, 0, 0, limb, ptr, 1) == count and short[0] == P.zqTable(0, limb=limb).ravel()[0]
            assert L.lolhip_plan_zq_table(P._h, 0, 0, 0, limb, None, 0) == L.lolhip_plan_zq_table(P._h, 0, 0, 0, limb, ptr, 0) == count
            assert (short[1:] == 7).all()
        assert L.lolhip_plan_zq_table(P._h, 0, 1, 0, -1, None, 0) == L.lolhip_plan_zq_table(P._h, 0, 0, 2, -1, None, 0) == 0
        assert L.lolhip_plan_zq_table(P._h, 0, -1, 0, -1, None, 0) == L.lolhip_plan_zq_table(P._h, 0, 0, -1, -1, None, 0) == 0
        assert L.lolhip_plan_zq_table(P._h, 0, 0, 0, -2, None, 0) == 0


def test_default_plans_build_no_copy(lolhip):
    D = _plan(lolhip, 257, dense=False)
    assert D.zqTable(0).size == 0 and D.zqTable(0, limb=0).size == 0


# ---- the challenge list --------------------------------------------------------------------------------------------------
def test_challenge_plans_take_the_dense_route_at_the_large_prime_lines(lolhip):
    from lol_amd import challenges as ch
    lines = rg.challenge_lines()
    assert len(lines) == 516
    cache, dense = {}, []
    for kind, m, q, _ in lines:
        if (m, q) not in cache:
            which, plan = ch.route(SimpleNamespace(m=m, q=q))
            # a modulus without a CRT basis: a s runs over the NTT primes of the RingMul made from the plan
            zq = plan if which == "plan" else lolhip.RingMul(plan).plan_Q
            assert plan.dense_zq == zq.dense_zq == ch.large_prime(m)
            cache[(m, q)] = (which, min(zq.zqRoute(0), zq.zqRoute(1)))
        dense.append(cache[(m, q)])
    large = [max(p for p, _ in lm.factor_pps(m)) > 13 for _, m, _, _ in lines]
    assert sum(large) == 144 and [r >= 1 for _, r in dense] == large
    assert sorted({m for (_, m, _, _), lp in zip(lines, large) if lp}) == [23, 29, 179, 257, 797]
    with_crt = sum(1 for (w, _), lp in zip(dense, large) if lp and w == "plan")
    assert (with_crt, 144 - with_crt) == (56, 88)
