"""The extended-precision float oracle (oracle/floatref.py *_ext) and the stage fixture, on the host.

  mpmath pin          crt_c_ext and gaussian_dec_ext agree with a 40-digit mpmath evaluation of the closed
                      forms to 1e-17 (float64 alone cannot: its unit roundoff is 1.1e-16)
  float64 pin         they agree with crt_matrix_c / gaussian_dec (n <= 600) and with golden_float.npz
                      within the 1e-12 contract; the float64 matrix inverse passes the backward-error check
  stage fixture       golden_float_stages.npz (lol-cpp's own outputs at tests/float_stages.py's indices, at
                      the columns fixture_columns names) is within the contract of the oracle, and lol-cpp itself meets the normwise bound the GPU
                      tests assert (16 u sum_s d_s)
  coverage            the GPU index set runs every vector length of k_cplx and k_gauss, each from a prime power
                      with e >= 2, and n = 8192
"""
import os

import numpy as np
import pytest

from float_stages import (CPLX_SIZES, FIXTURE_COLS, GAUSS_SIZES, STAGE_INDICES, bound_cplx, bound_gauss,
                          cplx_stages, fixture_columns, gauss_stages, stage_inputs)
from oracle import floatref as fr
from oracle import lolmath as lm

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-12


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.max(np.abs(got - want)) <= RTOL * max(1.0, np.max(np.abs(want)))


# ---- 40-digit restatement (small n only: dense n x n over mpmath) ----------------------------------
def _mp_crt_c(pps, z):
    import mpmath as mp
    m, n = lm.value_pps(pps), lm.totient_pps(pps)
    w = [mp.expjpi(mp.mpf(2 * k) / m) for k in range(m)]               # omega_m^k
    ex = np.zeros((n, n), dtype=np.int64)
    _, _, digs = fr._digits(pps)
    for (p, e), dig in zip(pps, digs):
        pp = p ** e
        zms = p * (dig // (p - 1)) + dig % (p - 1) + 1
        pw = np.array([lm.index_to_pow((p, e), int(j)) for j in dig])
        ex = (ex + ((zms[:, None] * pw[None, :]) % pp) * (m // pp)) % m   # prod_k omega_pp^a_k = omega_m^(sum a_k m/pp)
    return [[mp.fsum(w[ex[i, j]] * mp.mpc(z[b, j].real, z[b, j].imag) for j in range(n)) for i in range(n)]
            for b in range(z.shape[0])]


def _mp_gaussian_dec(pps, g):
    import mpmath as mp
    n = lm.totient_pps(pps)
    _, _, digs = fr._digits(pps)
    M = [[mp.mpf(1)] * n for _ in range(n)]
    for (p, e), dig in zip(pps, digs):
        if p == 2:
            for i in range(n):
                for j in range(n):
                    if dig[i] != dig[j]:
                        M[i][j] = mp.mpf(0)
            continue
        D = [[2 * (mp.cospi(mp.mpf(2 * ((r * c) % p)) / p) if c <= p // 2 else mp.sinpi(mp.mpf(2 * ((r * c) % p)) / p))
              / mp.sqrt(2) for c in range(1, p)] for r in range(p - 1)]
        for i in range(n):
            for j in range(n):
                a, b = int(dig[i]), int(dig[j])
                M[i][j] *= D[a % (p - 1)][b % (p - 1)] if a // (p - 1) == b // (p - 1) else 0
    return [[mp.fsum(M[i][j] * mp.mpf(float(g[b, j])) for j in range(n)) for i in range(n)] for b in range(g.shape[0])]


def _mp_of(x):
    """a long double (or complex long double) as an exact mpmath number: hi + lo in float64"""
    import mpmath as mp

    def r(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))
    if np.iscomplexobj(x):
        return mp.mpc(r(x.real), r(x.imag))
    return r(x)


def _mp_rel(got, want):
    import mpmath as mp
    num = mp.fsum(abs(_mp_of(got[b, i]) - want[b][i]) ** 2 for b in range(got.shape[0]) for i in range(got.shape[1]))
    den = mp.fsum(abs(want[b][i]) ** 2 for b in range(got.shape[0]) for i in range(got.shape[1]))
    return mp.sqrt(num / den)


@pytest.mark.parametrize("m", [25, 49, 121, 169, 2 ** 4 * 3 ** 2])
def test_ext_oracle_matches_mpmath(m):
    import mpmath as mp
    mp.mp.dps = 40
    pps = lm.factor_pps(m)
    n = lm.totient_pps(pps)
    rng = np.random.default_rng(m)
    z = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    g = rng.standard_normal((2, n))
    want_c, want_g = _mp_crt_c(pps, z), _mp_gaussian_dec(pps, g)
    e_c = _mp_rel(fr.crt_c_ext(pps, z), want_c)
    e_g = _mp_rel(fr.gaussian_dec_ext(pps, g), want_g)
    assert e_c <= 1e-17 and e_g <= 1e-17, (m, float(e_c), float(e_g))
    # and float64 is measurably worse, so the pin above is not vacuous
    assert _mp_rel(fr.crt_c(pps, z).astype(np.clongdouble), want_c) > 1e-17, m


def test_ext_oracle_matches_float64_restatement():
    rng = np.random.default_rng(7)
    for m in (8, 9, 15, 21, 45, 63, 64, 25, 49, 121, 169, 125, 2 * 11 ** 2, 3 * 5 * 7 * 4):
        pps = lm.factor_pps(m)
        n = lm.totient_pps(pps)
        assert n <= 600, m
        z = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        g = rng.standard_normal((3, n))
        assert close(fr.crt_c_ext(pps, z).astype(np.complex128), fr.crt_c(pps, z)), m
        assert close(fr.gaussian_dec_ext(pps, g).astype(np.float64), fr.gaussian_dec(pps, g)), m
        assert np.all(fr.crtinv_c_residual(pps, fr.crtinv_c(pps, z), z) <= 1e-13), m


def test_ext_oracle_matches_golden_float():
    gold = np.load(os.path.join(HERE, "golden", "golden_float.npz"))
    for m in (int(x) for x in gold["indices"]):
        pps = lm.factor_pps(m)
        z, g = gold[f"m{m}_cin"], gold[f"m{m}_gin"]
        assert close(gold[f"m{m}_crtc"], fr.crt_c_ext(pps, z).astype(np.complex128)), m
        assert close(gold[f"m{m}_gauss"], fr.gaussian_dec_ext(pps, g).astype(np.float64)), m
        assert np.all(fr.crtinv_c_residual(pps, gold[f"m{m}_crtinvc"], z) <= bound_cplx(pps)), m


def test_lolcpp_stage_fixture_within_oracle_and_bound():
    """lol-cpp's own outputs (the fixture, at the columns it keeps) against the long-double oracle: within the
    1e-12 contract, and within the normwise bound tests/test_float_stages.py asserts for the GPU, so that bound is
    attainable.  The fixture keeps no whole crtInvC rows past n = 384, so its backward error cannot be taken here:
    where n <= 384 it is, and elsewhere its crtInvC columns are checked against the dense float64 inverse (n <= 600)
    or, on the GPU, against the kernel whose backward error is bounded."""
    gold = np.load(os.path.join(HERE, "golden", "golden_float_stages.npz"))
    assert [int(x) for x in gold["indices"]] == STAGE_INDICES
    for m in STAGE_INDICES:
        pps = lm.factor_pps(m)
        n = lm.totient_pps(pps)
        z, g = stage_inputs(m)
        cols = fixture_columns(m)
        want_c, want_g = fr.crt_c_ext(pps, z)[:, cols], fr.gaussian_dec_ext(pps, g)[:, cols]
        for op in ("crtc", "crtinvc", "gauss"):
            assert gold[f"m{m}_{op}"].shape == (z.shape[0], len(cols)), (m, op)
        assert close(gold[f"m{m}_crtc"], want_c.astype(np.complex128)), m
        assert close(gold[f"m{m}_gauss"], want_g.astype(np.float64)), m
        assert np.all(fr.rel_err(gold[f"m{m}_crtc"], want_c) <= bound_cplx(pps)), m
        assert np.all(fr.rel_err(gold[f"m{m}_gauss"], want_g) <= bound_gauss(pps)), m
        if n <= FIXTURE_COLS:
            assert np.all(fr.crtinv_c_residual(pps, gold[f"m{m}_crtinvc"], z) <= bound_cplx(pps)), m
        if n <= 600:
            want_i = fr.crtinv_c(pps, z)[:, cols]
            assert np.max(np.abs(gold[f"m{m}_crtinvc"] - want_i)) <= 1e-10 * np.max(np.abs(want_i)), m


def test_stage_fixture_columns():
    for m in STAGE_INDICES:
        n = lm.totient_pps(lm.factor_pps(m))
        cols = fixture_columns(m)
        assert len(cols) == min(n, FIXTURE_COLS) and cols[0] == 0 and cols[-1] == n - 1, m
        assert np.all(np.diff(cols) > 0), m
        assert np.array_equal(cols, fixture_columns(m)), m


def test_stage_index_set_covers_every_kernel_size():
    ns = [lm.totient_pps(lm.factor_pps(m)) for m in STAGE_INDICES]
    assert ns == [20, 42, 110, 156, 100, 294, 1210, 2028, 2058, 2500, 4374, 5040, 3120, 1320, 1920, 880, 4096, 8192, 8192]
    cplx = {d for m in STAGE_INDICES for d, e in cplx_stages(lm.factor_pps(m)) if e >= 2}
    gauss = {d for m in STAGE_INDICES for d, e in gauss_stages(lm.factor_pps(m)) if e >= 2}
    assert cplx == CPLX_SIZES, sorted(CPLX_SIZES - cplx)
    assert gauss == GAUSS_SIZES, sorted(GAUSS_SIZES - gauss)
    # and the stage lists really are what the plan runs: every prime <= 13, so Plan::float_ok admits them all
    assert all(p <= 13 for m in STAGE_INDICES for p, _ in lm.factor_pps(m))
