"""Index set, inputs and error bound of the float stage tests (tests/test_float_stages.py on the GPU,
tests/test_float_oracle.py on the host, tests/golden/make_golden_float_stages.py for the fixture).

The floating-point programs reuse the Z_q stage lists (plan.cpp build_crt_programs): per prime power p^e,
crtC runs CRT_p (d = p - 1, odd p only) and e - 1 radix-p DFT stages (d = p), crtInvC the same list backwards,
and gaussianDec one (p - 1)-vector stage per odd prime.  STAGE_INDICES is chosen so that every vector length
k_cplx and k_gauss dispatch on runs, each from a prime power with e >= 2, and so that n reaches 8192.
"""
import numpy as np

from oracle import lolmath as lm

STAGE_INDICES = [25, 49, 121, 169, 125, 343, 1331, 2197, 2401, 3125, 6561, 11025, 4225, 1573, 5600, 1936,
                 2 ** 13, 2 ** 14, 2 ** 13 * 3]
CPLX_SIZES = {2, 3, 4, 5, 6, 7, 10, 11, 12, 13}       # the cases of k_cplx's switch
GAUSS_SIZES = {2, 4, 6, 10, 12}                       # the cases of k_gauss's switch
SEED = 20261015
U = 2.0 ** -53
FIXTURE_COLS = 384                                    # output columns per row the fixture keeps (n > FIXTURE_COLS)


def batch(n):
    return 2 if n <= 2500 else 1


def stage_inputs(m):
    """(z complex128 [B][n], g float64 [B][n]): the fixture's inputs, regenerated from SEED and m."""
    n = lm.totient_pps(lm.factor_pps(m))
    rng = np.random.default_rng([SEED, m])
    B = batch(n)
    z = rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))
    g = rng.standard_normal((B, n)) * 3.0
    return z, g


def fixture_columns(m):
    """The output columns golden_float_stages.npz keeps at index m: all of them when n <= FIXTURE_COLS, else the
    first, the last and a seeded sample in between, ascending.  (Every output of a stage program depends on every
    input of its vector; the full outputs are checked against the long-double oracle, not against the fixture.)"""
    n = lm.totient_pps(lm.factor_pps(m))
    if n <= FIXTURE_COLS:
        return np.arange(n)
    mid = np.random.default_rng([SEED, m, 1]).choice(np.arange(1, n - 1), FIXTURE_COLS - 2, replace=False)
    return np.sort(np.concatenate([[0, n - 1], mid]))


def cplx_stages(pps):
    """[(d, e)] of the dense stages crtC / crtInvC run, with the exponent of the prime power they come from."""
    out = []
    for p, e in pps:
        if p != 2:
            out.append((p - 1, e))
        out += [(p, e)] * (e - 1)
    return out


def gauss_stages(pps):
    return [(p - 1, e) for p, e in pps if p != 2]


def bound_cplx(pps):
    """16 u sum_s d_s over the stages of crtC (the same list serves crtInvC)."""
    return 16 * U * sum(d for d, _ in cplx_stages(pps))


def bound_gauss(pps):
    return 16 * U * max(1, sum(d for d, _ in gauss_stages(pps)))
