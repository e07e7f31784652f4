"""Host side of gSqNormDec and the RLWE / RLWR entries (include/lolhip.h): no GPU needed.

 - tests/rlwe_ref.py's gSqNorm against the reference's own tensorNormSqR / tensorNormSqD (tests/golden/golden_norm.npz):
   exact for int64, relative 1e-12 for doubles (the project's float contract);
 - lolhip_rlwe_error_bound against the restatement and its status codes;
 - a host-only plan refuses every device entry (no CPU fallback), and the argument checks come first.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import rlwe_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_M = [8, 12, 23, 45, 81, 1456, 11648, 14400, 2 ** 14, 2 ** 15]
ERR_INVALID, ERR_NO_CRT, ERR_NO_DEVICE = -1, -3, -5
# the distinct (m = 256, svar) pairs of rlwe-challenges params.txt rows 0-19
CHALLENGE_SVARS = [7.8125e-3, 3.125e-2, 0.28125, 0.6328125, 0.9367973043891067]
EPS = 2.0 ** -25


@pytest.fixture(scope="module")
def golden_norm():
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_norm.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("m", GOLDEN_M)
def test_restated_gsqnorm_matches_the_reference(golden_norm, m):
    pps = rr.factor_pps(m)
    ei = golden_norm[f"e_i_{m}"].astype(np.int64)
    assert np.abs(ei).max() < 2 ** 20 and ei.shape[1] == rr.totient(pps)
    assert np.array_equal(rr.gsqnorm_sat(pps, ei), golden_norm[f"n_i_{m}"])
    ed = golden_norm[f"e_d_{m}"].astype(np.float64)
    want = golden_norm[f"n_d_{m}"]
    assert (np.abs(rr.gsqnorm_f64(pps, ed) - want) <= 1e-12 * np.abs(want)).all()


def test_restated_gsqnorm_saturates_and_is_the_sum_of_squares_for_two_powers():
    e = np.array([[3, -4, 0, 1], [2 ** 31 - 1] * 4, [2 ** 32, 0, 0, 0], [rr.INT64_MIN, 0, 0, 0]], dtype=np.int64)
    got = rr.gsqnorm_sat([(2, 3)], e)
    assert 4 * (2 ** 31 - 1) ** 2 > rr.INT64_MAX
    assert list(got) == [26, rr.INT64_MAX, rr.INT64_MAX, rr.INT64_MAX]
    # the largest all-equal sample that still fits: n = 2 coefficients of 2^31 - 1 (m = 4)
    assert list(rr.gsqnorm_sat([(2, 2)], e[1:2, :2])) == [2 * (2 ** 31 - 1) ** 2] and 2 * (2 ** 31 - 1) ** 2 < 2 ** 63
    # m = 3: <e, (I+J) e> = sum e^2 + (sum e)^2
    assert rr.gsqnorm_int([(3, 1)], np.array([[5, -2]], dtype=np.int64)) == [25 + 4 + 9]


def _bound(lolhip, m, svar, eps, kind):
    pps = rr.factor_pps(m)
    arr = (lolhip.tensor._PP * max(1, len(pps)))()
    for i, (p, e) in enumerate(pps):
        arr[i].prime, arr[i].exponent = p, e
    out = C.c_double(-7.0)
    rc = lolhip.lib().lolhip_rlwe_error_bound(arr, len(pps), svar, eps, kind, C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("m,svar", [(256, v) for v in CHALLENGE_SVARS] + [(4 * 3 * 5 * 7, 0.28125), (45, 4.0)])
def test_error_bound_matches_restatement(lolhip, m, svar):
    rc, cont = _bound(lolhip, m, svar, EPS, 1)
    want = rr.error_bound_cont(m, svar, EPS)
    assert rc == 0 and abs(cont - want) <= 1e-12 * want, (cont, want)
    assert lolhip.RLWE.errorBound(m, svar, kind="cont") == cont
    rc, disc = _bound(lolhip, m, svar, EPS, 0)
    assert rc == 0 and disc == math.floor(disc) and int(disc) == rr.error_bound_disc(m, svar, EPS), disc
    got = lolhip.RLWE.errorBound(m, svar, EPS, kind="disc")
    assert isinstance(got, int) and got == int(disc) and got > cont


def test_error_bound_counts_the_odd_primes():
    """the 2^#odd primes term: m = 4*3*5*7 has three"""
    m, svar = 420, 0.28125
    n = 96
    plain = math.ceil(n * rr._stabilize(math.log(EPS)) + rr.error_bound_cont(m, svar, EPS))
    assert rr.error_bound_disc(m, svar, EPS) > plain + 6 * n


def test_error_bound_status_codes(lolhip):
    for svar, eps in ((0.0, EPS), (-1.0, EPS), (float("nan"), EPS), (float("inf"), EPS), (1.0, 0.0), (1.0, 1.0),
                      (1.0, -0.5), (1.0, 1.5), (1.0, float("nan"))):
        for kind in (0, 1):
            assert _bound(lolhip, 256, svar, eps, kind) == (ERR_INVALID, -7.0), (svar, eps)
    assert _bound(lolhip, 256, 1.0, EPS, 2)[0] == ERR_INVALID
    with pytest.raises(lolhip.LolHipError):
        lolhip.RLWE.errorBound(256, -1.0)


def test_work_len(lolhip):
    L = lolhip.lib()
    p = lolhip.Plan([(3, 2), (5, 1)], [181, 271, 541], host_only=True)
    assert L.lolhip_rlwe_work_len(p._h, 0, 5) == 5 * p.n * 4
    assert L.lolhip_rlwe_work_len(p._h, 1, 5) == 2 * 5 * p.n
    assert L.lolhip_rlwe_work_len(p._h, 2, 5) == 5 * p.n
    assert L.lolhip_rlwe_work_len(p._h, 3, 5) == ERR_INVALID
    assert L.lolhip_rlwe_work_len(p._h, 0, -1) == ERR_INVALID


def _calls(L, pl, kind, p=4, svar=1.0, B=0):
    """every device entry at B (null pointers): name -> status"""
    h, key = pl._h, bytes(32)
    return {
        "sample": L.lolhip_rlwe_sample_batch(h, None, kind, p, None, svar, key, 0, None, None, None, B),
        "error": L.lolhip_rlwe_error_batch(h, None, min(kind, 1), None, None, None, None, None, None, B),
        "rounded_prod": L.lolhip_rlwr_rounded_prod_batch(h, p, None, None, None, None, None, B),
        "check": L.lolhip_rlwr_check_batch(h, p, None, None, None, None, None, None, B),
        "secret": L.lolhip_rlwe_secret(h, None, key, 0, None),
        "gsqnorm": L.lolhip_gsqnorm_batch(h, None, None, None, B),
        "gsqnorm_f64": L.lolhip_gsqnorm_f64_batch(h, None, None, None, B),
    }


def test_host_only_plan_refuses_every_device_entry(lolhip):
    L = lolhip.lib()
    p1 = lolhip.Plan([(2, 4)], [97], host_only=True)
    for kind in (0, 1, 2):
        assert set(_calls(L, p1, kind).values()) == {ERR_NO_DEVICE}, kind
    p2 = lolhip.Plan([(2, 4)], [17, 97], host_only=True)
    assert _calls(L, p2, 0)["sample"] == ERR_NO_DEVICE and _calls(L, p2, 0)["error"] == ERR_NO_DEVICE
    # the Python layer raises before it stages anything
    r = lolhip.RLWE(p1)
    z = np.zeros((1, p1.n, 1), dtype=np.int64)
    s = np.zeros((p1.n, 1), dtype=np.int64)
    for call in (lambda: r.secret(key=bytes(32)), lambda: r.sampleDisc(s, 1, 1.0), lambda: r.sampleCont(s, 1, 1.0),
                 lambda: r.sampleRLWR(s, 1, 4), lambda: r.errorTermDisc(s, z, z), lambda: r.errorGSqNormDisc(s, z, z),
                 lambda: r.errorTermCont(s, z, np.zeros((1, p1.n))), lambda: r.roundedProd(s, z, 4),
                 lambda: r.validRLWR(s, z, z[..., 0], 4), lambda: r.gSqNorm(z[..., 0]), lambda: r.gSqNorm(np.zeros((1, p1.n)))):
        with pytest.raises(lolhip.NoDeviceError):
            call()


def test_argument_checks_come_before_the_device_check(lolhip):
    L = lolhip.lib()
    p1 = lolhip.Plan([(2, 4)], [97], host_only=True)
    p2 = lolhip.Plan([(2, 4)], [17, 97], host_only=True)
    # T != 1 for Cont / RLWR
    for kind in (1, 2):
        assert _calls(L, p2, kind)["sample"] == ERR_INVALID
    c = _calls(L, p2, 1)
    assert c["error"] == c["rounded_prod"] == c["check"] == ERR_INVALID
    # p >= q, p < 2
    for p in (97, 98, 1, 0, -3):
        c = _calls(L, p1, 2, p=p)
        assert c["sample"] == c["rounded_prod"] == c["check"] == ERR_INVALID, p
    assert _calls(L, p1, 2, p=96)["sample"] == ERR_NO_DEVICE
    # svar <= 0, not finite (ignored by RLWR)
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        for kind in (0, 1):
            assert _calls(L, p1, kind, svar=sv)["sample"] == ERR_INVALID, sv
        assert _calls(L, p1, 2, svar=sv)["sample"] == ERR_NO_DEVICE
    # B < 0, an unknown kind
    c = _calls(L, p1, 0, B=-1)
    assert {c[k] for k in ("sample", "error", "rounded_prod", "check", "gsqnorm", "gsqnorm_f64")} == {ERR_INVALID}
    assert L.lolhip_rlwe_sample_batch(p1._h, None, 3, 4, None, 1.0, bytes(32), 0, None, None, None, 0) == ERR_INVALID
    assert L.lolhip_rlwe_error_batch(p1._h, None, 2, None, None, None, None, None, None, 0) == ERR_INVALID
    # a plan without a CRT basis (16 does not divide 23 - 1)
    pn = lolhip.Plan([(2, 4)], [23], host_only=True)
    assert not pn.has_crt
    c = _calls(L, pn, 2)
    assert {c[k] for k in ("sample", "error", "rounded_prod", "check", "secret")} == {ERR_NO_CRT}
    assert c["gsqnorm"] == ERR_NO_DEVICE                                  # the norm needs the index only
    # the sampler's index limits (a prime above 13), and the norm's (n > 16384)
    p17 = lolhip.Plan([(17, 1)], [103], host_only=True)
    assert _calls(L, p17, 0)["sample"] == ERR_INVALID and _calls(L, p17, 2)["sample"] == ERR_NO_DEVICE
    assert _calls(L, p17, 0)["gsqnorm"] == ERR_NO_DEVICE
    big = lolhip.Plan([(2, 16)], [65537], host_only=True)
    assert _calls(L, big, 0)["gsqnorm"] == _calls(L, big, 0)["gsqnorm_f64"] == ERR_INVALID
