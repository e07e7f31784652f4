"""Host side of tests/test_scalar_interp.py (no GPU): which stage list the plans of the scalar stage interpreter
launch, on host-only plans, and the oracle those GPU tests compare with against the reference's own C++ at indices with
a prime factor >= 17.

Rows of Plan.program(): (kind, prime, vector length, stride); kinds (plan.h): 0 = a lone diagonal, 1 = DFT_p, 2 = CRT_p
(or a merged dense stage of the forward transform), 3 = CRT_p^-1, 12 / 13 = 2-power tile forward / inverse."""
import os

import numpy as np
import pytest

from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params
from params import PRIME_OPS
from test_she_properties import _run_properties


def _prog(lolhip, m, qs, inverse=False, polymul=False):
    P = lolhip.Plan(lm.factor_pps(m), qs, host_only=True)
    return [tuple(int(v) for v in r) for r in P.program(inverse, polymul)]


def _q(m):
    return tuple(lm.first_good_q(m, 2 ** b) for b in (26, 30, 45))


# what a lone crt launches at q ~ 2^26 (class 4: everything that merges is merged), 2^30 (class 2, 13-term
# accumulator: 3^2 and 3 (x) 5 merge, 5^2 and 3^3 do not) and 2^45 (64-bit residues: the staged list)
PROGRAMS = {
    51: 3 * [[(2, 3, 2, 1), (2, 17, 16, 2)]],
    153: 2 * [[(2, 3, 6, 1), (2, 17, 16, 6)]] + [[(2, 3, 2, 1), (1, 3, 3, 2), (2, 17, 16, 6)]],
    459: [[(2, 3, 18, 1), (2, 17, 16, 18)],                                    # 3^3 as one 18-vector
          [(2, 3, 2, 1), (2, 3, 9, 2), (2, 17, 16, 18)],                       # its two radix-3 stages as DFT_9
          [(2, 3, 2, 1), (1, 3, 3, 2), (1, 3, 3, 6), (2, 17, 16, 18)]],
    425: [[(2, 5, 20, 1), (2, 17, 16, 20)]] + 2 * [[(2, 5, 4, 1), (1, 5, 5, 4), (2, 17, 16, 20)]],
    255: 2 * [[(2, 3, 8, 1), (2, 17, 16, 8)]] + [[(2, 3, 2, 1), (2, 5, 4, 2), (2, 17, 16, 8)]],     # 3 (x) 5 as one 8-vector
    289: 3 * [[(2, 17, 16, 1), (1, 17, 17, 16)]],
    68: 3 * [[(0, 1, 1, 1), (1, 2, 2, 1), (2, 17, 16, 2)]],                    # no 2-power tile: the staged CRT_4
    544: 3 * [[(2, 17, 16, 16)]],                                              # the split route's odd part
    27648: 3 * [[(2, 3, 2, 512), (1, 3, 3, 1024), (1, 3, 3, 3072)]],           # the same at n = 9216, never merged
}
PROGRAMS_INV = {
    51: 3 * [[(3, 3, 2, 1), (3, 17, 16, 2)]],
    153: 2 * [[(3, 3, 6, 1), (3, 17, 16, 6)]] + [[(1, 3, 3, 2), (3, 3, 2, 1), (3, 17, 16, 6)]],
    459: [[(3, 3, 18, 1), (3, 17, 16, 18)],
          [(2, 3, 9, 2), (3, 3, 2, 1), (3, 17, 16, 18)],
          [(1, 3, 3, 6), (1, 3, 3, 2), (3, 3, 2, 1), (3, 17, 16, 18)]],
    425: [[(3, 5, 20, 1), (3, 17, 16, 20)]] + 2 * [[(1, 5, 5, 4), (3, 5, 4, 1), (3, 17, 16, 20)]],
    255: 2 * [[(3, 3, 8, 1), (3, 17, 16, 8)]] + [[(3, 3, 2, 1), (3, 5, 4, 2), (3, 17, 16, 8)]],
    289: 3 * [[(1, 17, 17, 16), (3, 17, 16, 1)]],
    68: 3 * [[(1, 2, 2, 1), (3, 17, 16, 2)]],
    544: 3 * [[(3, 17, 16, 16)]],
    27648: 3 * [[(1, 3, 3, 3072), (1, 3, 3, 1024), (3, 3, 2, 512)]],
}


@pytest.mark.parametrize("m", sorted(PROGRAMS))
def test_programs_of_scalar_plans(lolhip, m):
    """The lists tests/test_scalar_interp.py executes.  153, 459, 425, 255: the merged stages do reach the scalar
    interpreter.  None of these plans has a one-launch poly-mul: it is composed of these transforms."""
    for q, want, want_inv in zip(_q(m), PROGRAMS[m], PROGRAMS_INV[m]):
        assert _prog(lolhip, m, [q]) == want, (m, q)
        assert _prog(lolhip, m, [q], True) == want_inv, (m, q)
        assert _prog(lolhip, m, [q], polymul=True) == [] == _prog(lolhip, m, [q], True, polymul=True), (m, q)
    lolhip.debug_set("NO_MERGE", True)
    try:
        assert _prog(lolhip, m, [_q(m)[0]]) == PROGRAMS[m][2], m
        assert _prog(lolhip, m, [_q(m)[0]], True) == PROGRAMS_INV[m][2], m
    finally:
        lolhip.debug_set("NO_MERGE", False)


def test_program_table_reports_what_a_lone_transform_launches(lolhip):
    """lolhip_plan_table 10 / 11 and do_crt share one choice (capi.cpp crt_route).  The 2-power tiles exist in the
    vector interpreter only, so a plan it refuses must not report them: the scalar interpreter would take a tile for
    the identity."""
    tiles = lambda prog: [r for r in prog if r[0] in (12, 13)]
    for m, qs in ((68, [_q(68)[0]]), (544, [_q(544)[1]]), (22528, [_q(22528)[0]]), (27648, [_q(27648)[2]]), (12, [13]),
                  (12, [13, lm.first_good_q(12, 2 ** 30)])):
        for inverse in (False, True):
            assert _prog(lolhip, m, qs, inverse) and not tiles(_prog(lolhip, m, qs, inverse)), (m, qs)
    assert _prog(lolhip, 12, [13]) == [(0, 1, 1, 1), (1, 2, 2, 1), (2, 3, 2, 2)]
    assert _prog(lolhip, 22528, [_q(22528)[0]]) == [(2, 11, 10, 1024)]
    # the vector interpreter's plans: tiles where the lone transform is one launch ...
    q26, q30, q45 = _q(14400)
    assert _prog(lolhip, 12, [37]) == [(12, 1, 1, 1), (2, 3, 2, 2)]
    assert _prog(lolhip, 14400, [q26]) == [(12, 1, 4, 1), (12, 5, 1, 16), (2, 3, 6, 32), (2, 5, 20, 192)]
    # ... and, with 64-bit residues and e >= 5, the odd part of the split route; the poly-mul stays one launch with tiles
    odd = [(2, 3, 2, 32), (1, 3, 3, 64), (2, 5, 4, 192), (1, 5, 5, 768)]
    assert _prog(lolhip, 14400, [q45]) == odd
    assert _prog(lolhip, 14400, [q45], polymul=True) == [(12, 1, 4, 1), (12, 5, 1, 16)] + odd
    # the switches of the launch are the switches of the table
    for name, want in (("NO_POW2_PART", [(12, 1, 4, 1), (12, 5, 1, 16), (2, 3, 6, 32), (2, 5, 20, 192)]),      # fused all the same
                       ("NO_FUSED2", [(2, 3, 2, 32), (1, 3, 3, 64), (2, 5, 4, 192), (1, 5, 5, 768)]),          # split: the unmerged odd part
                       ("GENERIC_SCALAR", odd)):
        lolhip.debug_set(name, True)
        try:
            assert _prog(lolhip, 14400, [q26]) == want, name
        finally:
            lolhip.debug_set(name, False)
    lolhip.debug_set("NO_FUSED2", True); lolhip.debug_set("NO_POW2_PART", True)
    try:
        assert [r[0] for r in _prog(lolhip, 14400, [q45])] == [0] + 5 * [1] + [2, 1, 2, 1]       # CRT_64 staged: its twiddle diagonal, five DFT_2 stages
    finally:
        lolhip.debug_set("NO_FUSED2", False); lolhip.debug_set("NO_POW2_PART", False)


def test_a_prime_19_is_not_taken_for_a_merged_3_cubed(lolhip):
    """CRT_19 has 18-element vectors, the length of the merged 3^3 stage, which is all the vector interpreter's
    18-vector code knows (a dense matrix, no diagonal, classes 2 / 4): an index with a factor 19 must go to the scalar
    interpreter like every prime >= 17.  Seen from the host: its poly-mul is not one launch of the vector interpreter."""
    for m in (19, 38, 57, 19 * 64):
        for q in _q(m):
            assert _prog(lolhip, m, [q], polymul=True) == [], (m, q)
    assert _prog(lolhip, 19, [_q(19)[0]]) == [(2, 19, 18, 1)]
    assert _prog(lolhip, 19 * 64, [_q(19 * 64)[0]]) == [(2, 19, 18, 32)]          # no 2-power tiles either: the split route
    assert _prog(lolhip, 27, [_q(27)[0]], polymul=True) == [(2, 3, 18, 1)]        # the merged 3^3 stays where it was


@pytest.fixture(scope="module")
def golden_scalar():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_scalar.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("m", [51, 153, 221, 289, 323, 544])
def test_restatement_matches_the_reference_at_large_primes(cpuref, golden_scalar, m):
    """tests/golden/make_golden_scalar.py: the reference's own C++ on seeded inputs"""
    q = int(golden_scalar[f"{m}/q"][0])
    assert lm.is_prime(q) and (q - 1) % m == 0 and 2 ** 30 < q < 2 ** 31
    P = Params(lm.factor_pps(m), [q])
    y = golden_scalar[f"{m}/y"]
    assert y.shape == (2, P.n, 1) and y.min() >= 0 and y.max() == q - 1
    for op in ("crt", "crtinv") + PRIME_OPS:
        want = golden_scalar[f"{m}/{op}"]
        got = getattr(cpuref, op)(P, y)
        assert got is not None and np.array_equal(got.reshape(want.shape), want), (op, m)


def test_she_model_holds_at_m_51_on_the_cpu_oracle(cpuref):
    """the parameters of test_scalar_interp.py's SHE run, with the CPU oracle as the engine: this proves the model there"""
    _run_properties(lambda pps, qs: sm.CpuEngine(cpuref, Params(pps, qs)), cpuref, 51, 103, 2 ** 29, 256, seed=51)
