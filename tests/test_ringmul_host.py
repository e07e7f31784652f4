"""Host side of the exact ring product over moduli without a CRT basis (lolhip_ringmul_*, lol_amd.RingMul): the
declared symbols, the rule for the default NTT primes against its Python restatement (tests/ringmul_ref.py), the
certification exactly at the bound 2 C_m H^2 < prod Q, every status code and the work length.  No GPU: host-only plans."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ringmul_ref as rr
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, MODULUS, NO_CRT, NO_DEVICE = 0, -1, -2, -3, -5
SYMBOLS = ("moduli", "create", "destroy", "work_len", "batch", "prepare", "prepared_batch")

# (m, moduli): K = 1, 2 and 3, two-power and mixed indices, one tuple
MODULI_TABLE = [
    (16, [2 ** 8]), (8, [2]), (34, [15]), (45, [2 ** 20]), (21, [9]),                          # one prime
    (16384, [2 ** 32]), (16, [2 ** 32]), (45, [2 ** 40]), (64, [2 ** 16, 12289, 3 ** 20]),  # two
    (16384, [2 ** 62 - 1]), (16, [2 ** 61 + 1]), (34, [2 ** 62 - 1]), (45, [2 ** 55, 2 ** 60 + 1]),                 # three
]


def _plan(lolhip, m, qs):
    return lolhip.Plan(lm.factor_pps(m), qs, host_only=True)


def _create(lolhip, pq, pQ):
    h = C.c_void_p()
    rc = lolhip.lib().lolhip_ringmul_create(pq._h if pq else None, pQ._h if pQ else None, C.byref(h))
    if h:
        lolhip.lib().lolhip_ringmul_destroy(h)
    return rc


def test_symbols_are_declared_exported_and_bound(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in SYMBOLS:
        assert f"lolhip_ringmul_{nm}" in names
        assert hasattr(raw, f"lolhip_ringmul_{nm}")
    assert lolhip.RingMul is lolhip.tensor.RingMul and "RingMul" in lolhip.__all__


@pytest.mark.parametrize("m", [1, 2, 3, 4, 8, 9, 15, 16, 21, 25, 34, 45])
def test_growth_restatement_matches_its_definition(m):
    assert rr.growth(m) == rr.growth_by_definition(m)


def test_default_moduli_follow_the_rule(lolhip):
    seen = set()
    for m, qs in MODULI_TABLE:
        want = rr.moduli(m, qs)
        got = lolhip.RingMul.moduli(lm.factor_pps(m), qs)
        assert got == want, (m, qs)
        assert rr.accepts(m, qs, got) and all(lm.is_prime(Q) and Q % m == 1 % m and Q < 2 ** 61 for Q in got)
        assert _create(lolhip, _plan(lolhip, m, qs), _plan(lolhip, m, got)) == OK
        seen.add(len(got))
    assert seen == {1, 2, 3}
    assert lolhip.RingMul.moduli(16, [2 ** 8]) == rr.moduli(16, [2 ** 8])           # an index in place of its factors


def test_moduli_statuses(lolhip):
    L = lolhip.lib()
    pp, Qs = (lolhip.tensor._PP * 2)(), (C.c_int64 * 3)()
    pp[0].prime, pp[0].exponent, pp[1].prime, pp[1].exponent = 2, 4, 3, 1
    q = lambda *v: (C.c_int64 * len(v))(*v)
    assert L.lolhip_ringmul_moduli(pp, 2, q(256), 1, Qs) == 1 and Qs[0] == rr.moduli(48, [256])[0]
    assert L.lolhip_ringmul_moduli(pp, 2, None, 1, Qs) == INVALID
    assert L.lolhip_ringmul_moduli(pp, 2, q(256), 0, Qs) == INVALID
    assert L.lolhip_ringmul_moduli(pp, 2, q(256), 1, None) == INVALID
    assert L.lolhip_ringmul_moduli(None, 2, q(256), 1, Qs) == INVALID
    assert L.lolhip_ringmul_moduli(pp, -1, q(256), 1, Qs) == INVALID
    pp[1].prime = 2                                                                  # not ascending
    assert L.lolhip_ringmul_moduli(pp, 2, q(256), 1, Qs) == INVALID
    pp[1].prime, pp[1].exponent = 9, 1                                               # not a prime
    assert L.lolhip_ringmul_moduli(pp, 2, q(256), 1, Qs) == INVALID
    pp[1].prime, pp[1].exponent = 3, 0
    assert L.lolhip_ringmul_moduli(pp, 2, q(256), 1, Qs) == INVALID
    pp[1].exponent = 1
    assert L.lolhip_ringmul_moduli(pp, 2, q(1), 1, Qs) == MODULUS
    assert L.lolhip_ringmul_moduli(pp, 2, q(256, 2 ** 62), 2, Qs) == MODULUS
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.RingMul.moduli([(2, 4), (3, 1)], [2 ** 62])
    assert e.value.code == MODULUS
    with pytest.raises(lolhip.LolHipError) as e:                                     # an index beyond 2^30
        lolhip.RingMul.moduli([(2, 31)], [256])
    assert e.value.code == INVALID


@pytest.mark.parametrize("m,Qs", rr.BOUNDARY)
@pytest.mark.parametrize("odd", [False, True])
def test_create_accepts_and_rejects_exactly_at_the_bound(lolhip, m, Qs, odd):
    assert all(lm.is_prime(Q) and Q % m == 1 for Q in Qs)
    q_ok, q_bad, ratio = rr.boundary_pair(m, Qs, odd)
    print(f"m={m} Qs={Qs} q={q_ok}: 2 C H^2 / prod Q = {ratio:.4f}")
    assert 0.95 <= ratio < 1 and rr.accepts(m, [q_ok], Qs) and not rr.accepts(m, [q_bad], Qs)
    pQ = _plan(lolhip, m, list(Qs))
    assert _create(lolhip, _plan(lolhip, m, [q_ok]), pQ) == OK
    assert _create(lolhip, _plan(lolhip, m, [q_bad]), pQ) == MODULUS
    # in a tuple the largest H decides
    assert _create(lolhip, _plan(lolhip, m, [3, q_ok, 4]), pQ) == OK
    assert _create(lolhip, _plan(lolhip, m, [3, q_bad, 4]), pQ) == MODULUS


def test_create_statuses(lolhip):
    L = lolhip.lib()
    pq, pQ = _plan(lolhip, 16, [256]), _plan(lolhip, 16, rr.moduli(16, [256]))
    assert _create(lolhip, pq, pQ) == OK
    assert L.lolhip_ringmul_create(pq._h, pQ._h, None) == INVALID
    assert _create(lolhip, None, pQ) == INVALID and _create(lolhip, pq, None) == INVALID
    assert _create(lolhip, pq, _plan(lolhip, 32, [12289])) == INVALID                # another index
    assert _create(lolhip, _plan(lolhip, 8, [256]), pQ) == INVALID
    g = lm.good_qs(16, 2 ** 20)
    four = [next(g) for _ in range(4)]
    assert _create(lolhip, pq, _plan(lolhip, 16, four)) == INVALID                   # K > 3
    assert _create(lolhip, pq, _plan(lolhip, 16, four[:3])) == OK
    assert _create(lolhip, _plan(lolhip, 16, [256] * 17), pQ) == INVALID             # T > 16
    assert _create(lolhip, _plan(lolhip, 16, [256] * 16), pQ) == OK
    assert _create(lolhip, pq, _plan(lolhip, 16, [four[0], four[0]])) == MODULUS     # not distinct
    assert _create(lolhip, pq, _plan(lolhip, 16, [2 ** 20])) == NO_CRT
    assert _create(lolhip, pq, _plan(lolhip, 16, [four[0], 2 ** 20 + 7])) == NO_CRT
    assert _create(lolhip, pq, _plan(lolhip, 16, [97])) == MODULUS                   # 2 * 8 * 128^2 > 97
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.RingMul(pq, _plan(lolhip, 16, [97]))
    assert e.value.code == MODULUS


def test_work_len_and_compute_statuses_on_host_only_plans(lolhip):
    L = lolhip.lib()
    for m, qs in ((16, [256]), (45, [2 ** 40]), (64, [2 ** 16, 12289, 15]), (16, [2 ** 61 + 1])):
        rm = lolhip.RingMul(_plan(lolhip, m, qs))                                    # plan_Q by the default rule
        n, T, K = math.prod(lm.totient_pp(pe) for pe in lm.factor_pps(m)), len(qs), len(rr.moduli(m, qs))
        assert (rm.n, rm.T, rm.K) == (n, T, K) and rm.plan_Q.qs == rr.moduli(m, qs)
        for B in (0, 1, 2, 3, 7):
            words = B * T * n * K
            assert rm.workLen(B) == 2 * (words + (words & 1))
        assert L.lolhip_ringmul_work_len(rm._h, -1) == INVALID
        assert L.lolhip_ringmul_work_len(None, 1) == INVALID
        assert L.lolhip_ringmul_work_len(rm._h, 2 ** 31) == INVALID
        x = 1 << 12                                                                  # any non-null address: nothing is launched
        assert L.lolhip_ringmul_batch(None, None, x, x, x, x, 1) == INVALID
        assert L.lolhip_ringmul_batch(rm._h, None, x, x, x, x, -1) == INVALID
        assert L.lolhip_ringmul_prepare(rm._h, None, x, x, x, -1) == INVALID
        assert L.lolhip_ringmul_prepared_batch(rm._h, None, x, x, x, 2, x, 3) == INVALID     # Bb not in {1, B}
        assert L.lolhip_ringmul_prepared_batch(rm._h, None, x, x, x, 1, x, -3) == INVALID
        assert L.lolhip_ringmul_batch(rm._h, None, x, x, x, x, 1) == NO_DEVICE
        assert L.lolhip_ringmul_batch(rm._h, None, None, None, None, None, 0) == NO_DEVICE
        assert L.lolhip_ringmul_prepare(rm._h, None, x, x, None, 1) == NO_DEVICE
        assert L.lolhip_ringmul_prepared_batch(rm._h, None, x, x, x, 1, x, 3) == NO_DEVICE
        assert L.lolhip_ringmul_prepared_batch(rm._h, None, x, x, x, 3, x, 3) == NO_DEVICE
        a = np.zeros((2, n, T), dtype=np.int64)
        for call in (lambda: rm(a, a), lambda: rm.prepare(a), lambda: rm.mulPrepared(a, np.zeros((2 * T, n, K), dtype=np.int64))):
            with pytest.raises(lolhip.NoDeviceError):
                call()


# ---------------------------------------------------------------------------------------------
# prime-power lists at every entry that validates one (valid_pps / to_pps, hostmath.h)
# ---------------------------------------------------------------------------------------------
_BELOW_2_30 = [(3, 2), (7, 1), (11, 1), (31, 1), (151, 1), (331, 1)]                  # 2^30 - 1
_ABOVE_2_30 = [(5, 2), (13, 1), (41, 1), (61, 1), (1321, 1)]                          # 2^30 + 1
# list -> the statuses of lolhip_plan_create (host_only, q = 257), lolhip_ringmul_moduli (q = 2),
# lolhip_crtset_modulus (p = 2, e = 1) and lolhip_pt_tunnel_modulus (p = 2, e = 1) with the list as S (R empty, first
# hop) and as R (S = [(7, 1)]).  The index caps: none for a plan (its own rule is n <= 2^24), m <= 2^30 for ringmul,
# m < 2^31 for crtSet; the tunnel bound converts its lists without validating them.
PPS_STATUSES = [
    ("descending primes", [(3, 1), (2, 2)], (INVALID, INVALID, INVALID, 24, 264)),
    ("a repeated prime", [(2, 1), (2, 1)], (INVALID, INVALID, INVALID, 2, 132)),
    ("exponent 0", [(2, 2), (3, 0)], (INVALID, INVALID, INVALID, 8, 264)),
    ("a composite prime", [(2, 1), (9, 1)], (INVALID, INVALID, INVALID, 240, 264)),
    ("empty", [], (OK, 1, 3, 2, 132)),
    ("valid", [(2, 2), (3, 1)], (OK, 1, 7, 24, 264)),
    ("2^30 - 1", _BELOW_2_30, (INVALID, 1, 53687091151, MODULUS, 8448)),
    ("2^30 + 1", _ABOVE_2_30, (INVALID, INVALID, 45097156651, MODULUS, 4224)),
    ("2^31 - 2", [(2, 1)] + _BELOW_2_30, (INVALID, INVALID, 53687091151, MODULUS, 8448)),
    ("2^31 + 2", [(2, 1)] + _ABOVE_2_30, (INVALID, INVALID, INVALID, MODULUS, 4224)),
]


@pytest.mark.parametrize("name,pps,want", PPS_STATUSES, ids=[c[0] for c in PPS_STATUSES])
def test_prime_power_list_validation_at_every_entry(lolhip, name, pps, want):
    L = lolhip.lib()
    from lol_amd.tensor import _pps as arr
    _, a, n = arr(pps)
    q = lambda *v: (C.c_int64 * len(v))(*v)
    assert math.prod(p ** e for p, e in _BELOW_2_30) == 2 ** 30 - 1 and math.prod(p ** e for p, e in _ABOVE_2_30) == 2 ** 30 + 1
    h = C.c_void_p()
    got = [L.lolhip_plan_create(a, n, q(257), 1, 1, C.byref(h))]
    if h:
        L.lolhip_plan_destroy(h)
    got.append(L.lolhip_ringmul_moduli(a, n, q(2), 1, (C.c_int64 * 3)()))
    got.append(L.lolhip_crtset_modulus(a, n, 2, 1))
    (_, none, n0), (_, seven, n7) = arr([]), arr([(7, 1)])
    got.append(L.lolhip_pt_tunnel_modulus(none, n0, a, n, 1, 1, 2, 1))
    got.append(L.lolhip_pt_tunnel_modulus(a, n, seven, n7, 1, 0, 2, 1))
    assert tuple(got) == want
    # the conversion's own rules: a negative count, and no array behind a positive one
    assert L.lolhip_plan_create(a, -1, q(257), 1, 1, C.byref(h)) == INVALID
    assert L.lolhip_plan_create(None, 1, q(257), 1, 1, C.byref(h)) == INVALID
    assert L.lolhip_ringmul_moduli(a, -1, q(2), 1, (C.c_int64 * 3)()) == INVALID
    assert L.lolhip_crtset_modulus(a, -1, 2, 1) == INVALID and L.lolhip_crtset_modulus(None, 1, 2, 1) == INVALID
    assert L.lolhip_pt_tunnel_modulus(a, -1, seven, n7, 1, 0, 2, 1) == INVALID
    assert L.lolhip_pt_tunnel_modulus(none, n0, None, 1, 1, 1, 2, 1) == INVALID
