"""The scalar stage interpreter (kernels.hip k_generic) at every kind of plan only it can run (-m gpu).

The vector interpreter refuses a plan (mixed.hip mixed_ok) with a prime factor >= 17, with n > 8192 and an index that is
not a power of two, with m = 2^e beyond e = 15, or with a modulus <= 16; GENERIC_SCALAR forces the same kernel on any
plan.  test_scalar_interp_host.py pins which stage list each of these plans launches.  Here every list is executed:

    a  prime factors >= 17: primes (dense lengths 16 .. 96: every fold count and tail of the 8-term accumulator),
       composites (strided 16-vectors), prime powers (DFT_17 / DFT_19 plus the twiddle diagonal), the merged
       6-, 8-, 18- and 20-vector stages that class-2 plans hand to this kernel, ragged packed batches
    b  2^e * 17 whole (e < 5) and split between the m = 2^k kernels and the scalar odd part (e >= 5)
    c  moduli <= 16 (multipliers of the G maps above q)
    d  GENERIC_SCALAR on indices the vector interpreter takes: both kernels, one answer
    e  n > 8192: the largest LDS-resident polynomials, the HBM scratch ring and its grid stride, DFT_2 programs of
       m = 2^16 and 2^17
    f  the ends of the magic division: the largest n that takes it and the one shape that does not
    g  what is composed around the kernel: ring extensions, the unfused key switch, the SHE properties

Bit-exact everywhere: `np.array_equal` against the CPU oracle, no tolerance in this file.
"""
import time

import numpy as np
import pytest

from oracle import lolmath as lm
from oracle.oracle import Params
from params import PLAN_NAME, PRIME_OPS
from saturate import good_below, neg_rep
from test_gpu_parity import test_twace_embed_vs_oracle as _check_ext          # the assertions, under names pytest does not collect
from test_pipelines import test_gpu_keyswitch as _check_keyswitch
from test_she_properties import _run_properties

pytestmark = pytest.mark.gpu

TRANSFORMS = ("crt", "crtinv")


def _params(m, qs, crt=True):
    if crt:
        return Params(lm.factor_pps(m), qs)
    R = Params.__new__(Params)                    # no CRT basis: what the prime ops need
    R.pps = lm.factor_pps(m)
    R.qs, R.T, R.m, R.n = list(qs), len(qs), m, lm.totient_pps(R.pps)
    return R


def _inputs(R, rng, B=4):
    """rows: random residues, q - 1 everywhere, alternating 0 / q - 1, representatives in (-q, 0]; further rows random"""
    qv = np.array(R.qs, dtype=np.int64)
    y, z = R.random(rng, max(B, 4)), R.random(rng, max(B, 4))
    y[1] = qv - 1
    y[2, ::2] = 0; y[2, 1::2] = qv - 1
    y[3] = neg_rep(y[3], R.qs)
    z[1] = qv - 1
    z[2] = neg_rep(z[2], R.qs)
    return np.ascontiguousarray(y), np.ascontiguousarray(z)


def _gpu_ops(P, y, z, ops=None):
    """every op of test_generic_indices on the device: name -> array (None where the op refuses)"""
    import torch
    out = {}
    for op in (TRANSFORMS if P.has_crt else ()) + PRIME_OPS:
        if ops is None or op in ops:
            out[op] = getattr(P, PLAN_NAME[op])(y)
    if not P.has_crt or ops is not None:
        return out
    out["mul"] = P.mul(y, z)
    da, db = torch.from_numpy(y).cuda(), torch.from_numpy(z).cuda()
    dc = torch.empty_like(da)
    P.polymul(da, db, out=dc)
    out["polymul"] = dc.cpu().numpy()
    assert np.array_equal(da.cpu().numpy(), y) and np.array_equal(db.cpu().numpy(), z), "poly-mul wrote its inputs"
    x = da.clone(); P.polymul(x, db, out=x); out["polymul c=a"] = x.cpu().numpy()
    x = db.clone(); P.polymul(da, x, out=x); out["polymul c=b"] = x.cpu().numpy()
    x = da.clone(); P.polymul(x, x, out=x); out["square"] = x.cpu().numpy()
    out["mulGCRT"] = P.mulGCRT(y)
    out["divGCRT"] = P.divGCRT(out["mulGCRT"])
    return out


def _oracle_ops(cpuref, R, y, z, crt=True, ops=None):
    out = {}
    for op in (TRANSFORMS if crt else ()) + PRIME_OPS:
        if ops is None or op in ops:
            out[op] = getattr(cpuref, op)(R, y)
    if not crt or ops is not None:
        return out
    out["mul"] = cpuref.mul(R, y, z)
    out["polymul"] = out["polymul c=a"] = out["polymul c=b"] = cpuref.polymul(R, y, z)
    out["square"] = cpuref.polymul(R, y, y)
    # mulGCRT = crt . mulGPow . crtInv ; divGCRT its inverse (TensorTests.hs:107-112)
    out["mulGCRT"] = cpuref.crt(R, cpuref.gpow(R, cpuref.crtinv(R, y)))
    out["divGCRT"] = np.mod(y, np.array(R.qs, dtype=np.int64))
    return out


def _same(got, want, tag):
    assert got.keys() == want.keys(), tag
    for op in want:
        assert (got[op] is None) == (want[op] is None), (op, tag)
        if want[op] is not None:
            assert np.array_equal(got[op], want[op]), (op, tag)


def _check(gpu, cpuref, m, qs, seed, B=4, crt=True, ops=None):
    """one plan, every op, the four kinds of input, against the oracle; returns the device results"""
    P, R = gpu.Plan(lm.factor_pps(m), qs), _params(m, qs, crt)
    assert P.has_crt == crt
    y, z = _inputs(R, np.random.default_rng(seed), B)
    got = _gpu_ops(P, y, z, ops)
    _same(got, _oracle_ops(cpuref, R, y, z, crt, ops), (m, qs))
    return got


def _moduli_sets(m):
    """one modulus below 2^27 (the lazy 32-bit class), the top of the Q32 instantiation, the first 64-bit modulus, the tops
    of both 64-bit classes, a pair that must clear q32 for the whole plan, and three moduli at about 2^30"""
    q27 = good_below(m, 2 ** 27)
    g = lm.good_qs(m, 2 ** 30)
    return [[q27], [good_below(m, 2 ** 32)], [lm.first_good_q(m, 2 ** 32)], [good_below(m, 2 ** 61)], [good_below(m, 2 ** 62)],
            [q27, lm.first_good_q(m, 2 ** 32)], [next(g), next(g), next(g)]]


# ---------------------------------------------------------------------------------------------------------------------
# a. prime factors >= 17
# ---------------------------------------------------------------------------------------------------------------------
# primes: d = 16, 18, 22, 30, 96 terms per dot product = 2, 2, 2, 3, 12 folds of 8 and a tail of 0, 2, 6, 6, 0 terms;
# composites: strided 16-vectors (221: behind a 12-vector stage; 7429: n = 6336, the 1024-thread launch);
# prime powers: DFT_17 / DFT_19 (d = 17, 19: tails of 1 and 3 terms) behind the twiddle diagonal; 17^3: two of them
LARGE_PRIME_INDICES = [17, 19, 23, 31, 97, 51, 85, 119, 221, 323, 7429, 289, 361, 4913]


@pytest.mark.parametrize("m", LARGE_PRIME_INDICES)
def test_indices_with_a_prime_factor_of_17_or_more(gpu, cpuref, m):
    for k, qs in enumerate(_moduli_sets(m)):
        _check(gpu, cpuref, m, qs, seed=m * 8 + k)


@pytest.mark.parametrize("m", [153, 459, 425, 255])
def test_merged_programs_on_the_scalar_path(gpu, cpuref, m):
    """Class-2 plans replace 3^2, 3^3, 5^2 and 3 (x) 5 by one dense 6-, 18-, 20- and 8-vector stage (plan.cpp
    merge_stages) and, with a factor 17 beside them, launch that list on the scalar interpreter.  At a class-2 modulus
    (merged), at a 64-bit modulus (staged) and with NO_MERGE (staged, 32-bit operands): one answer, the oracle's."""
    q26, q58 = lm.first_good_q(m, 2 ** 26), lm.first_good_q(m, 2 ** 58)
    merged = _check(gpu, cpuref, m, [q26], seed=m)
    _check(gpu, cpuref, m, [q58], seed=m + 1)
    _check(gpu, cpuref, m, [lm.first_good_q(m, 2 ** 30)], seed=m + 3)          # the 13-term class: 459 runs 3^3 as CRT_3 and a DFT_9 stage
    gpu.debug_set("NO_MERGE", True)
    try:
        staged = _check(gpu, cpuref, m, [q26], seed=m)
    finally:
        gpu.debug_set("NO_MERGE", False)
    _same(staged, merged, (m, "NO_MERGE against merged"))
    # two moduli of one class: the merged matrices are per component
    _check(gpu, cpuref, m, [q26, lm.first_good_q(m, q26)], seed=m + 2)


@pytest.mark.parametrize("B", [1, 2, 3, 7, 13, 33, 65, 130])
def test_ragged_packed_batches(gpu, cpuref, B):
    """m = 51 (n = 32): up to 64 polynomials share a workgroup; batches that leave the last group short or alone"""
    m = 51
    for qs in ([lm.first_good_q(m, 2 ** 30)], [lm.first_good_q(m, 2 ** 40), lm.first_good_q(m, 2 ** 20)]):
        P, R = gpu.Plan(lm.factor_pps(m), qs), _params(m, qs)
        rng = np.random.default_rng(B)
        y, z = R.random(rng, B), R.random(rng, B)
        y[B - 1] = neg_rep(y[B - 1], qs)
        assert np.array_equal(P.crt(y), cpuref.crt(R, y)), (B, qs)
        assert np.array_equal(P.crtInv(y), cpuref.crtinv(R, y)), (B, qs)
        assert np.array_equal(P.divGDec(y), cpuref.ginvdec(R, y)), (B, qs)
        assert np.array_equal(P.polymul(y, z), cpuref.polymul(R, y, z)), (B, qs)


# ---------------------------------------------------------------------------------------------------------------------
# b. 2^e * 17
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [1, 2, 4, 5, 6, 9, 10])
def test_two_power_times_17(gpu, cpuref, e):
    """e < 5: the whole stage program (DFT_2 stages and their diagonals) on the scalar interpreter.  e >= 5: the 2-power
    factor through the m = 2^k kernels and prog_crt_odd through the scalar interpreter (the default), or the whole
    program with NO_POW2_PART.  n = 8 .. 8192."""
    m = 2 ** e * 17
    for k, qs in enumerate(([good_below(m, 2 ** 31)], [good_below(m, 2 ** 61)], [lm.first_good_q(m, 2 ** 20), lm.first_good_q(m, 2 ** 40)])):
        split = _check(gpu, cpuref, m, qs, seed=m + k)
        if e >= 5:
            gpu.debug_set("NO_POW2_PART", True)
            try:
                whole = _check(gpu, cpuref, m, qs, seed=m + k)
            finally:
                gpu.debug_set("NO_POW2_PART", False)
            _same(whole, split, (m, qs, "NO_POW2_PART against the split route"))


# ---------------------------------------------------------------------------------------------------------------------
# c. moduli <= 16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,qs", [(3, [7]), (3, [13]), (4, [5]), (4, [13]), (12, [13]), (5, [11]), (6, [7, 13]),
                                  (12, [13, lm.first_good_q(12, 2 ** 30)])])
def test_moduli_up_to_16_with_a_crt_basis(gpu, cpuref, m, qs):
    """the vector interpreter keeps its small multipliers as they stand, so one modulus <= 16 sends the whole tuple here"""
    assert all(lm.is_prime(q) and (q - 1) % m == 0 for q in qs) and min(qs) <= 16
    for B in (4, 9):
        _check(gpu, cpuref, m, qs, seed=m * 100 + qs[0] + B, B=B)


@pytest.mark.parametrize("m,q", [(51, 16), (289, 8)])
def test_g_multipliers_above_the_modulus(gpu, cpuref, m, q):
    """divGPow / divGDec multiply by p - 1 - i, i + 1, c + 1 and p: at p = 17 over q = 16 or 8 they exceed q (smallmod's
    k % q branch).  No CRT basis: the six prime ops."""
    got = _check(gpu, cpuref, m, [q], seed=m + q, B=5, crt=False)
    assert set(got) == set(PRIME_OPS) and all(v is not None for v in got.values())


# ---------------------------------------------------------------------------------------------------------------------
# d. GENERIC_SCALAR on plans the vector interpreter takes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [45, 225, 1575, 1728, 11648, 14400])
def test_forced_scalar_interpreter_equals_the_default_route(gpu, cpuref, m):
    for k, lower in enumerate((2 ** 26, 2 ** 30, 2 ** 58)):
        qs = [lm.first_good_q(m, lower)]
        default = _check(gpu, cpuref, m, qs, seed=m + k)
        gpu.debug_set("GENERIC_SCALAR", True)
        try:
            forced = _check(gpu, cpuref, m, qs, seed=m + k)
        finally:
            gpu.debug_set("GENERIC_SCALAR", False)
        _same(forced, default, (m, qs, "GENERIC_SCALAR against the default route"))


# ---------------------------------------------------------------------------------------------------------------------
# e. n > 8192
# ---------------------------------------------------------------------------------------------------------------------
# 27648, 19456: n = 9216, 147,456 of the 155,648 bytes of LDS, the split route with an LDS-resident scalar odd part;
# 22528: n = 10240, the smallest index on the scratch ring; 2^11 * 17: n = 16384; 9 * 2^13: n = 24576, a merged 3^2 stage on
# the scratch path at the class-2 modulus; 2^16, 2^17: programs of 15 and 16 DFT_2 stages (the m = 2^k kernels end at 2^15)
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("m", [27648, 19456, 22528, 2 ** 11 * 17, 9 * 2 ** 13, 2 ** 16, 2 ** 17])
def test_polynomials_beyond_the_vector_interpreter(gpu, cpuref, m, T):
    n = lm.totient_pps(lm.factor_pps(m))
    assert n > 8192 and (2 * n * 8 > 152 * 1024) == (n > 9728)
    # every op; the poly-mul is composed of lone transforms around a stream-ordered temporary
    qs = [lm.first_good_q(m, 2 ** 26)] if T == 1 else [lm.first_good_q(m, 2 ** 30), lm.first_good_q(m, 2 ** 58)]
    _check(gpu, cpuref, m, qs, seed=m + T)


def test_scratch_ring_grid_stride(gpu, cpuref):
    """B T = 514 items over the ring's 512 slots at n = 10240: two workgroups take a second item.  Every row."""
    m, B = 22528, 257
    qs = [lm.first_good_q(m, 2 ** 30), lm.first_good_q(m, 2 ** 45)]
    P, R = gpu.Plan(lm.factor_pps(m), qs), _params(m, qs)
    assert R.n == 10240 and B * R.T > 512
    y = R.random(np.random.default_rng(514), B)
    y[B - 1] = neg_rep(y[B - 1], qs)
    assert np.array_equal(P.crt(y), cpuref.crt(R, y))
    assert np.array_equal(P.crtInv(y), cpuref.crtinv(R, y))


# ---------------------------------------------------------------------------------------------------------------------
# f. the ends of the magic division
# ---------------------------------------------------------------------------------------------------------------------
# fdiv<true> computes x / v as (x M) >> 40 with M = floor(2^40 / v) + 1, exact while x v < 2^40.  Every divisor of a
# stage (stride, length, diagonal period, n itself) is at most n and x < n, so n < 2^20 is the launch's condition;
# m = 2^18 * 9 (n = 786,432) is the largest n the reference's index range reaches below it and m = 2^21 (n = 2^20) the
# only shape above.  One polynomial, one modulus, crt and crtInv; the wall times are printed (pytest -s).
@pytest.mark.parametrize("m", [2 ** 18 * 9, 2 ** 21])
def test_division_limits(gpu, cpuref, m):
    qs = [lm.first_good_q(m, 2 ** 58)]
    P, R = gpu.Plan(lm.factor_pps(m), qs), _params(m, qs)
    assert (R.n < 2 ** 20) == (m != 2 ** 21) and R.n >= 786432
    y = R.random(np.random.default_rng(m % 1000), 1)
    y[0, ::3] = qs[0] - 1
    y[0, 1::7] = neg_rep(y[0, 1::7], qs)
    t0 = time.perf_counter()
    f, i = P.crt(y), P.crtInv(y)
    t1 = time.perf_counter()
    wf, wi = cpuref.crt(R, y), cpuref.crtinv(R, y)
    t2 = time.perf_counter()
    print(f"\nm = {m}, n = {R.n}: crt + crtInv on the device {t1 - t0:.3f} s (host copies included), oracle {t2 - t1:.3f} s")
    assert np.array_equal(f, wf)
    assert np.array_equal(i, wi)


# ---------------------------------------------------------------------------------------------------------------------
# g. around the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,m2", [(17, 51), (51, 255), (17, 289), (68, 544), (19, 323)])
def test_ring_extensions_over_scalar_plans(gpu, cpuref, m, m2):
    _check_ext(gpu, cpuref, m, m2, lm.first_good_q(m2, 2 ** 20))


@pytest.mark.parametrize("m", [51, 153, 544])
@pytest.mark.parametrize("base", [0, 2, 256])
def test_unfused_keyswitch_over_scalar_plans(gpu, cpuref, m, base):
    """decompose -> scalar crt -> knapsack: no fused key switch exists for these plans"""
    g = lm.good_qs(m, 2 ** 29)
    _check_keyswitch(gpu, cpuref, lm.factor_pps(m), [next(g), next(g)], base)


def test_she_properties_over_a_scalar_plan(gpu, cpuref):
    """the reference's SHE properties (test_she_properties.py) at m = 51, plaintext modulus 103 = 2 m + 1"""
    _run_properties(lambda pps, qs: gpu.Plan(pps, qs), cpuref, 51, 103, 2 ** 29, 256, seed=51)
