"""Host side of the dense complex CRT stages (LOLHIP_PLAN_DENSE_CPLX, lolhip_plan_create_opts; include/lolhip.h): no GPU.

 - the new creator, the route accessor and the table read-back in the ctypes table, with the header's types, struct and
   constant;
 - lolhip_plan_create_opts checks `size`, refuses unknown flag and route bits and honours the new bit; the two older
   creators still refuse it;
 - cplxRoute() at a table of indices on default and opted-in host-only plans, and the statuses of crtc / crtinvc there;
 - the matrix forms the device reads against the closed forms of the matrices: the transposed copy, the planes M_re,
   M_im, -M_im, their padding;
 - by enumeration over the GPU tests' case tables: every path of the kernel is reached by some case.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cplx_dense_cases import DENSE_INDICES, LARGE_PARITY, PARITY_INDICES, dense_routes
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_NO_DEVICE = 0, -1, -5
ST_DIAG, ST_DFTP, ST_CRTP, ST_CRTPINV, ST_SCALE = 0, 1, 2, 3, 10
LDS_BUDGET = 152 * 1024


def _plan(lolhip, m, dense, **kw):
    return lolhip.Plan.for_index(m, [12289], host_only=True, dense_cplx=dense, **kw)


def _switched(lolhip, m, forced=False, valu=False):
    """an opted-in host-only plan built under the debug switches, which are released again"""
    L = lolhip.lib()
    L.lolhip_debug_set(b"CPLX_DENSE", int(forced))
    L.lolhip_debug_set(b"CPLX_DENSE_VALU", int(valu))
    try:
        return _plan(lolhip, m, True)
    finally:
        L.lolhip_debug_set(b"CPLX_DENSE", 0)
        L.lolhip_debug_set(b"CPLX_DENSE_VALU", 0)


# ---- the binding ---------------------------------------------------------------------------------------------------------
def test_abi_rows_struct_and_constant():
    from lol_amd import _abi
    from test_abi_host import RETURNS, _ctypes_kind, prototypes
    header = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    protos = prototypes()
    for name in ("lolhip_plan_create_opts", "lolhip_plan_cplx_route", "lolhip_plan_cplx_table"):
        restype, argtypes = _abi.ABI[name]
        assert restype is RETURNS[protos[name][0]], name
        assert [_ctypes_kind(t) for t in argtypes] == protos[name][1], name
    assert protos["lolhip_plan_create_opts"] == ("int", ["ptr", "int", "ptr", "int", "int", "ptr", "ptr"])
    assert protos["lolhip_plan_cplx_route"] == ("int", ["ptr"])
    assert protos["lolhip_plan_cplx_table"] == ("int64_t", ["ptr", "int", "int", "int", "ptr", "int64_t"])
    (fields,) = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*lolhip_plan_opts\s*;", header)
    assert [tuple(f.split()) for f in fields.split(";") if f.strip()] == [("uint32_t", "size"), ("uint32_t", "flags"), ("uint32_t", "routes")]
    assert [(n, t) for n, t in _abi._PlanOpts._fields_] == [("size", C.c_uint32), ("flags", C.c_uint32), ("routes", C.c_uint32)]
    assert C.sizeof(_abi._PlanOpts) == 12
    assert _abi.ABI["lolhip_plan_create_opts"][1][5]._type_ is _abi._PlanOpts
    (value,) = re.findall(r"#define\s+LOLHIP_PLAN_DENSE_CPLX\s+(\d+)u?\b", header)
    assert int(value) == _abi.PLAN_DENSE_CPLX == 2
    import lol_amd.tensor as t
    assert t.PLAN_DENSE_CPLX == 2


# ---- the creators --------------------------------------------------------------------------------------------------------
def test_creators_and_their_bits(lolhip):
    from lol_amd._abi import _PlanOpts
    L = lolhip.lib()
    _, arr, npp = lolhip.tensor._pps(lm.factor_pps(17))
    q = (C.c_int64 * 1)(103)

    def opts(size, flags, routes):
        h = C.c_void_p()
        o = _PlanOpts(size, flags, routes)
        rc = L.lolhip_plan_create_opts(arr, npp, q, 1, 1, C.byref(o), C.byref(h))
        assert bool(h) == (rc == OK), (size, flags, routes)
        got = (rc, L.lolhip_plan_cplx_route(h), L.lolhip_plan_gauss_route(h)) if h else (rc, None, None)
        if h:
            L.lolhip_plan_destroy(h)
        return got

    # flags, routes -> status, cplx route, gauss route at m = 17
    for flags, routes, want in ((0, 0, (OK, 0, 0)), (1, 0, (OK, 0, 2)), (2, 0, (OK, 2, 0)), (3, 0, (OK, 2, 2)), (2, 1, (OK, 2, 0)),
                                (3, 1, (OK, 2, 2)), (0, 1, (OK, 0, 0)), (4, 0, (ERR_INVALID, None, None)), (6, 0, (ERR_INVALID, None, None)),
                                (0x80000002, 0, (ERR_INVALID, None, None)), (2, 2, (ERR_INVALID, None, None)), (2, 3, (ERR_INVALID, None, None)),
                                (0, 0x80000000, (ERR_INVALID, None, None))):
        assert opts(12, flags, routes) == want, (flags, routes)
    # size is checked: anything but sizeof(lolhip_plan_opts), and a null block
    for size in (0, 4, 8, 11, 13, 16, 24):
        assert opts(size, 2, 0) == (ERR_INVALID, None, None), size
    h = C.c_void_p()
    assert L.lolhip_plan_create_opts(arr, npp, q, 1, 1, None, C.byref(h)) == ERR_INVALID and not h
    # the older creators refuse the new bit, as flag and as route
    for flags in (2, 3):
        h = C.c_void_p()
        assert L.lolhip_plan_create_flags(arr, npp, q, 1, 1, flags, C.byref(h)) == ERR_INVALID and not h
        assert L.lolhip_plan_create_routes(arr, npp, q, 1, 1, flags, 0, C.byref(h)) == ERR_INVALID and not h
        assert L.lolhip_plan_create_routes(arr, npp, q, 1, 1, 0, flags, C.byref(h)) == ERR_INVALID and not h
    assert L.lolhip_plan_cplx_route(None) == 0
    with pytest.raises(ValueError):
        lolhip.Plan.for_index(17, [103], host_only=True, dense_cplx=True, omega_pp=[1])
    # the three options compose
    P = lolhip.Plan.for_index(17, [103], host_only=True, dense_cplx=True, dense_gauss=True, dense_zq=True)
    assert (P.cplxRoute(), P.gaussRoute(), P.zqRoute(0)) == (2, 2, 1)


def test_a_plan_without_the_flag_is_the_plan_of_the_older_creators(lolhip):
    """same tables, same programs, same routes: flags / routes without the new bit behave as lolhip_plan_create_routes"""
    from lol_amd._abi import _PlanOpts
    L = lolhip.lib()
    for m in (17, 45, 323):
        pps, arr, npp = lolhip.tensor._pps(lm.factor_pps(m))
        q = (C.c_int64 * 1)(lm.first_good_q(m, 1000))
        a, b = C.c_void_p(), C.c_void_p()
        o = _PlanOpts(12, 1, 1)
        assert L.lolhip_plan_create_opts(arr, npp, q, 1, 1, C.byref(o), C.byref(a)) == OK
        assert L.lolhip_plan_create_routes(arr, npp, q, 1, 1, 1, 1, C.byref(b)) == OK
        for h in (a, b):
            assert L.lolhip_plan_cplx_table(h, 0, 0, 0, None, 0) == 0
        for which in (0, 1, 2, 3, 10, 11, 20, 21):
            na = L.lolhip_plan_table(a, which, 0, None, 0)
            assert na == L.lolhip_plan_table(b, which, 0, None, 0)
            ta, tb = np.zeros(na, dtype=np.int64), np.zeros(na, dtype=np.int64)
            L.lolhip_plan_table(a, which, 0, ta.ctypes.data_as(C.POINTER(C.c_int64)), na)
            L.lolhip_plan_table(b, which, 0, tb.ctypes.data_as(C.POINTER(C.c_int64)), na)
            assert np.array_equal(ta, tb), (m, which)
        assert [L.lolhip_plan_cplx_route(h) for h in (a, b)] == [L.lolhip_plan_cplx_route(b)] * 2
        assert [L.lolhip_plan_gauss_route(h) for h in (a, b)] == [L.lolhip_plan_gauss_route(b)] * 2
        assert [L.lolhip_plan_zq_route(h, 0) for h in (a, b)] == [L.lolhip_plan_zq_route(b, 0)] * 2
        L.lolhip_plan_destroy(a); L.lolhip_plan_destroy(b)


# ---- the route -----------------------------------------------------------------------------------------------------------
ROUTES = [  # m, default plan, opted-in plan
    (16, 1, 1), (45, 1, 1),                                   # no prime above 13: the register kernel on either plan
    (17, 0, 2), (19, 0, 2), (51, 0, 2), (68, 0, 2), (289, 0, 2), (323, 0, 2), (797, 0, 2),
    (2 ** 9 * 17, 0, 2),                                      # n = 4096
    (2 ** 10 * 17, 0, 2),                                     # n = 8192: one buffer, the dense stage is the last
    (32 * 17 * 19, 0, 2),                                     # n = 4608: 144 KiB of ping-pong, within the 152 KiB budget
    (3 * 2 ** 14, 0, 0),                                      # n = 16384
    (2 ** 11 * 17, 0, 0),                                     # n = 16384
    (1031, 0, 0),                                             # the first prime above the cap of 1021
    (1021, 0, 2),                                             # the cap itself
]


def _lds_rule(pps):
    """the accepted set restated from the arithmetic: stage kinds in program order (forward and inverse hold the same
    dense stages at the same places counted from the front), 16 n bytes when the only dense stage is the last stage of
    the program, 32 n otherwise"""
    n = lm.totient_pps(pps)
    if n > 8192 or max(p for p, _ in pps) > 1021:
        return False
    dense_at, count = [], 0
    for p, e in pps:
        stages = (1 if p != 2 else 0) + (e - 1)                # CRT_p and e - 1 DFT_p; diagonals fold into them ...
        if p == 2 and e > 1:
            stages += 1                                        # ... but the crtTwiddle of 2^e, the first operation, stands alone
        if p > 13:
            dense_at += list(range(count, count + stages))
        count += stages
    if not dense_at:
        return None
    nbuf = 1 if dense_at == [count - 1] else 2
    return count <= 12 and nbuf * 16 * n <= LDS_BUDGET


@pytest.mark.parametrize("m,default,opted", ROUTES)
def test_route_is_a_function_of_the_index_and_the_flag(lolhip, m, default, opted):
    D, P = _plan(lolhip, m, False), _plan(lolhip, m, True)
    assert D.cplxRoute() == default
    assert P.cplxRoute() == opted
    pps = lm.factor_pps(m)
    rule = _lds_rule(pps)
    assert opted == (default if rule is None else (2 if rule else 0))
    # the programs agree with the route: no rows when refused, a dense stage exactly at the primes above 13
    for inv in (False, True):
        assert (D.cplxProgram(inv).shape[0] == 0) == (default == 0)
        prog = P.cplxProgram(inv)
        assert (prog.shape[0] == 0) == (opted == 0)
        for kind, p, d, rts, route in prog.tolist():
            assert (route != 0) == (kind in (ST_DFTP, ST_CRTP, ST_CRTPINV) and p > 13), (m, kind, p)
        assert prog[:, 4].tolist() == dense_routes(prog.tolist(), P.n), m
        assert all(r == 0 for r in D.cplxProgram(inv)[:, 4].tolist())


@pytest.mark.parametrize("m", [2 ** 5 * 17 * 19, 2 ** 6 * 3 * 5 * 17, 2 ** 3 * 3 * 5 * 7 * 17, 2 ** 5 * 11 * 17, 2 ** 4 * 17 * 23, 17 * 31, 9 * 17 * 19,
                               3 * 1021, 2 ** 3 * 1021, 2 ** 4 * 1021, 5 * 7 * 257, 2 ** 5 * 17 * 23, 17 * 19 * 23, 2 ** 4 * 17 * 41, 2 ** 6 * 17 * 19])
def test_route_follows_the_lds_arithmetic(lolhip, m):
    """n up to 8192 with the dense stages in the middle, at the end, and several of them: served exactly when the
    program fits its one or two buffers"""
    pps = lm.factor_pps(m)
    rule = _lds_rule(pps)
    assert rule is not None
    assert _plan(lolhip, m, True).cplxRoute() == (2 if rule else 0), (m, lm.totient_pps(pps))
    assert _plan(lolhip, m, False).cplxRoute() == 0


def test_the_required_set_is_served(lolhip):
    """every index with n <= 4096 whose primes are at most 1021 (sampled: all products of a 2-power, at most two odd
    primes below 14 and one or two primes above 13 from a spread list), and 2^e p up to n = 8192"""
    big = [17, 19, 97, 257, 1021]
    seen = 0
    for e in (0, 1, 3, 6, 9, 10):
        for small in (1, 3, 5, 15, 7 * 13):
            for p1 in big:
                for p2 in [1] + [b for b in big if b > p1]:
                    m = 2 ** e * small * p1 * p2
                    n = lm.totient_pps(lm.factor_pps(m))
                    if n <= 4096 or (small == 1 and p2 == 1 and n <= 8192):
                        assert _plan(lolhip, m, True).cplxRoute() == 2, (m, n)
                        seen += 1
    assert seen > 60


@pytest.mark.parametrize("m,routes", [(17, [2]), (257, [2]), (331, [1]), (797, [1]), (1021, [1]), (2 * 257, [2]), (3 * 257, [0, 2]), (289, [2, 2]),
                                      (17 * 257, [2, 2]), (2 ** 10 * 17, [0] * 10 + [2]), (32 * 17 * 19, [0] * 5 + [2, 2])])
def test_matrix_route_needs_sixteen_rows_and_sixteen_columns(lolhip, m, routes):
    """m = 257: 16 items of 4 KiB fill 64 KiB, 16 columns; m = 331: 12 items; m = 797: 5; 3 257: 8 items of two columns"""
    P = _plan(lolhip, m, True)
    assert P.cplxProgram()[:, 4].tolist() == routes == dense_routes(P.cplxProgram().tolist(), P.n)


def test_statuses_on_host_only_plans(lolhip):
    """both entries ask for the device first, as every compute entry does; the route is checked after it (on the GPU:
    tests/test_cplx_dense.py)"""
    L = lolhip.lib()
    for m in (17, 45, 3 * 2 ** 14):
        for dense in (False, True):
            P = _plan(lolhip, m, dense)
            assert L.lolhip_crtc_batch(P._h, None, None, 0) == ERR_NO_DEVICE
            assert L.lolhip_crtinvc_batch(P._h, None, None, 0) == ERR_NO_DEVICE
    assert L.lolhip_crtc_batch(None, None, None, 0) == ERR_INVALID


def test_debug_switches_are_read_when_the_plan_is_built(lolhip):
    P = _switched(lolhip, 45, forced=True)
    assert P.cplxRoute() == 2 and P.cplxProgram()[:, 4].tolist() == [2, 2, 2]        # CPLX_DENSE lifts the length condition
    assert _switched(lolhip, 45, forced=True, valu=True).cplxProgram()[:, 4].tolist() == [1, 1, 1]
    assert _switched(lolhip, 289, valu=True).cplxProgram()[:, 4].tolist() == [1, 1]
    assert _plan(lolhip, 45, True).cplxRoute() == 1                                   # released: register stages again
    assert P.cplxRoute() == 2                                                         # and the built plan keeps its route
    assert _switched(lolhip, 16, forced=True).cplxRoute() == 1                        # no odd prime: nothing to force
    assert lolhip.Plan.for_index(45, [12289], host_only=True).cplxRoute() == 1
    # a forced index whose two buffers do not fit keeps the register route: 13 2^10, n = 6144, 2-power stages first
    assert _switched(lolhip, 2 ** 10 * 13, forced=True).cplxRoute() == 2              # the dense stage is the last: one buffer
    assert _switched(lolhip, 2 ** 9 * 5 * 7, forced=True).cplxRoute() == 1            # n = 6144, two dense stages: 192 KiB


# ---- the tables ----------------------------------------------------------------------------------------------------------
def _closed_form(kind, p, inverse):
    """DFT_p[i][c] = w^(c i), CRT_p[i][c] = w^(c (i + 1)), CRT_p^-1[i][c] = w^(i (c + 1)) - w^(p - c - 1) with w the
    inverse root (plan.cpp build_crt_programs), in long double"""
    w = np.exp((-2j if inverse else 2j) * np.pi * np.arange(p).astype(np.longdouble) / np.longdouble(p))
    d = p if kind == ST_DFTP else p - 1
    i, c = np.meshgrid(np.arange(d), np.arange(d), indexing="ij")
    if kind == ST_DFTP:
        return w[(c * i) % p]
    if kind == ST_CRTP:
        return w[(c * (i + 1)) % p]
    return w[(i * (c + 1)) % p] - w[(p - c - 1) % p]


@pytest.mark.parametrize("m", [17, 19, 51, 289, 323, 797, 2 ** 9 * 17])
def test_matrix_forms(lolhip, m):
    P, D = _plan(lolhip, m, True), _plan(lolhip, m, False)
    L = lolhip.lib()
    dense = 0
    for inv in (False, True):
        for s, (kind, p, d, rts, route) in enumerate(P.cplxProgram(inv).tolist()):
            Mt = P.cplxTable(s, 0, inverse=inv)
            assert D.cplxTable(s, 0, inverse=inv).size == 0                  # a default plan builds no form
            if not route:
                assert Mt.size == 0 and all(P.cplxTable(s, f, inverse=inv).size == 0 for f in (1, 2, 3))
                continue
            dense += 1
            assert Mt.shape == (d, d)
            M = Mt.T
            want = _closed_form(kind, p, inv)
            assert float(np.abs(M - want).max()) <= 8 * 2.0 ** -52, (m, s)
            dpr, dpc = (d + 15) // 16 * 16, (d + 3) // 4 * 4
            re, im, ni = (P.cplxTable(s, f, inverse=inv).reshape(dpr, dpc) for f in (1, 2, 3))
            assert np.array_equal(re[:d, :d].view(np.int64), np.ascontiguousarray(M.real).view(np.int64))
            assert np.array_equal(im[:d, :d].view(np.int64), np.ascontiguousarray(M.imag).view(np.int64))
            assert np.array_equal(ni[:d, :d], -im[:d, :d])
            for pl in (re, im, ni):
                assert not pl[d:, :].any() and not pl[:, d:].any()
            assert L.lolhip_plan_cplx_table(P._h, int(inv), s, 4, None, 0) == 0
            short = np.full(9, 7.0)
            assert L.lolhip_plan_cplx_table(P._h, int(inv), s, 1, short.ctypes.data_as(C.POINTER(C.c_double)), 5) == dpr * dpc
            assert np.array_equal(short[:5], re.ravel()[:5]) and (short[5:] == 7.0).all()
    assert dense == 2 * sum(e for p, e in lm.factor_pps(m) if p > 13)
    assert L.lolhip_plan_cplx_table(P._h, 0, len(P.cplxProgram()), 0, None, 0) == L.lolhip_plan_cplx_table(P._h, 0, -1, 0, None, 0) == 0
    assert L.lolhip_plan_cplx_table(None, 0, 0, 0, None, 0) == 0


# ---- the kernel's paths, by enumeration ------------------------------------------------------------------------------------
def _paths(prog):
    """the paths of k_cplx_dense a program takes (floatpath.hip), from its rows (kind, p, d, stride, route)"""
    out = set()
    rows = prog.tolist()
    for s, (kind, p, d, rts, route) in enumerate(rows):
        last = s == len(rows) - 1
        if kind in (ST_DIAG, ST_SCALE):
            out.add("diag")
        elif route == 0:
            out.add("reg")
        else:
            out.add({1: "valu-rows" if rts < 64 else "valu-cols", 2: "mfma-vt" if rts < 16 else "mfma-mv"}[route])
            out.add("to-slab" if last else "ping-pong")
            if d % 16:
                out.add("row-tail")
            if d % 4:
                out.add("depth-tail")
    if rows and rows[-1][4] == 0:
        out.add("copy-out")
    return out


def test_the_gpu_cases_reach_every_path_of_the_kernel(lolhip):
    """the plans tests/test_cplx_dense.py builds: DENSE_INDICES as they are, DENSE_INDICES and LARGE_PARITY under
    CPLX_DENSE_VALU, PARITY_INDICES under CPLX_DENSE with and without CPLX_DENSE_VALU"""
    seen = set()
    for m in DENSE_INDICES:
        P = _plan(lolhip, m, True)
        assert P.cplxRoute() == 2
        for inv in (False, True):
            seen |= _paths(P.cplxProgram(inv))
    mfma_only = set(seen)
    for m in LARGE_PARITY + [2 ** 9 * 17]:
        for inv in (False, True):
            seen |= _paths(_switched(lolhip, m, valu=True).cplxProgram(inv))
    for m in PARITY_INDICES:
        for valu in (False, True):
            P = _switched(lolhip, m, forced=True, valu=valu)
            assert P.cplxRoute() == 2
            for inv in (False, True):
                seen |= _paths(P.cplxProgram(inv))
    # (the last stage of a program with a dense stage is the largest prime's and so dense itself: the kernel's copy-out
    # of an LDS-resident result is there for completeness and no index reaches it)
    assert seen == {"diag", "reg", "valu-rows", "valu-cols", "mfma-vt", "mfma-mv", "to-slab", "ping-pong", "row-tail", "depth-tail"}
    assert {"mfma-vt", "mfma-mv", "to-slab", "ping-pong", "row-tail", "depth-tail", "reg", "diag"} <= mfma_only
    # the register kernel itself: a default plan at every parity index
    assert all(_plan(lolhip, m, False).cplxRoute() == 1 for m in PARITY_INDICES)
