"""The float kernels (k_cplx: crtC / crtInvC, k_gauss: gaussianDec; floatpath.hip) at every stage size they
dispatch on, on the GPU (-m gpu).

  accuracy        at every index of tests/float_stages.py (every dense vector length of both kernels, each from a
                  prime power with e >= 2; n up to 8192): within the 1e-12 contract of lol-cpp's own outputs
                  (golden_float_stages.npz, at the columns it keeps) and of the long-double oracle, and the
                  normwise relative error against that oracle (the backward error ||M_ext got - z|| / ||z|| for
                  crtInvC) at most 16 u sum_s d_s
  moduli          the plan's moduli play no role: bit-identical outputs for a modulus below 2^30, one near 2^61,
                  T = 16 of mixed widths, a modulus without a CRT basis and the debug switches that reshape the
                  Z_q programs the float path shares
  grid stride     batches past the 4096-workgroup sweep: every row equals the small-batch run bit for bit
  in place        a row-offset view under a side stream, its neighbours untouched
  limits          n = 8192 accepted; n > 8192 and p >= 17 refused with the input untouched; B = 0
"""
import os

import numpy as np
import pytest

from float_stages import STAGE_INDICES, bound_cplx, bound_gauss, fixture_columns, stage_inputs
from oracle import floatref as fr
from oracle import lolmath as lm
from test_rns_width_host import mixed16

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-12
GRID = 4096                                  # workgroups of k_cplx / k_gauss


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.max(np.abs(got - want)) <= RTOL * max(1.0, np.max(np.abs(want)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "golden_float_stages.npz"))


def _plan(gpu, m, qs=None):
    pps = lm.factor_pps(m)
    return gpu.Plan(pps, qs or [lm.first_good_q(m, 1000)]), pps


def _no_crt_q(m):
    """a prime q > 1000 with m not dividing q - 1: no CRT basis mod q"""
    q = 1001
    while not (lm.is_prime(q) and (q - 1) % m):
        q += 1
    return q


@pytest.mark.parametrize("m", STAGE_INDICES)
def test_float_ops_at_every_stage_size(gpu, gold, m):
    """Bound asserted: 16 u sum_s d_s over the index's stages, u = 2^-53 (1.6e-14 .. 6.8e-14 for crtC / crtInvC,
    1.8e-15 .. 3.9e-14 for gaussianDec).  Observed on an MI355X, max over the index set: crtC 1.15e-15 (m = 11025),
    crtInvC backward error 1.27e-15 (11025), gaussianDec 4.8e-16 (1573); lol-cpp's own outputs on the same inputs:
    1.15e-15, 1.23e-15, 5.7e-16.  Roots built as a running product of omega instead exceed the bound (9e-14 at
    m = 1331) while passing the 1e-12 contract."""
    P, pps = _plan(gpu, m)
    z, g = stage_inputs(m)
    c, ci, gd = P.crtC(z), P.crtInvC(z), P.gaussianDec(g)
    cols = fixture_columns(m)                                           # the columns the fixture keeps
    assert close(c[:, cols], gold[f"m{m}_crtc"]), ("crtC vs lol-cpp", m)
    assert close(ci[:, cols], gold[f"m{m}_crtinvc"]), ("crtInvC vs lol-cpp", m)
    assert close(gd[:, cols], gold[f"m{m}_gauss"]), ("gaussianDec vs lol-cpp", m)
    want_c, want_g = fr.crt_c_ext(pps, z), fr.gaussian_dec_ext(pps, g)
    assert close(c, want_c.astype(np.complex128)), ("crtC vs oracle", m)
    assert close(gd, want_g.astype(np.float64)), ("gaussianDec vs oracle", m)
    e_c = float(fr.rel_err(c, want_c).max())
    e_i = float(fr.crtinv_c_residual(pps, ci, z).max())
    e_g = float(fr.rel_err(gd, want_g).max())
    print(f"float-stage-error m={m} crtC={e_c:.3e} crtInvC={e_i:.3e} gaussianDec={e_g:.3e} "
          f"bound={bound_cplx(pps):.3e}/{bound_gauss(pps):.3e}")
    assert e_c <= bound_cplx(pps), ("crtC", m, e_c)
    assert e_i <= bound_cplx(pps), ("crtInvC", m, e_i)
    assert e_g <= bound_gauss(pps), ("gaussianDec", m, e_g)


# ---- the moduli play no role ------------------------------------------------------------------------
def _configs(m):
    base = [lm.first_good_q(m, 2 ** 20)]
    return [("q < 2^30", base, None), ("q ~ 2^61", [lm.first_good_q(m, 2 ** 61)], None), ("T = 16 mixed", mixed16(m), None),
            ("no CRT basis", [_no_crt_q(m)], None)] + [(sw, base, sw) for sw in ("NO_MERGE", "NO_OWN_DIAG", "NO_KRON", "GENERIC_SCALAR")]


@pytest.mark.parametrize("m", [121, 11025, 2 ** 14, 5600])
def test_float_ops_independent_of_moduli(gpu, m):
    import torch
    pps = lm.factor_pps(m)
    z, g = stage_inputs(m)
    dz, dg = torch.from_numpy(z).cuda(), torch.from_numpy(g).cuda()
    ref = None
    for name, qs, sw in _configs(m):
        if sw:
            gpu.debug_set(sw, True)
        try:
            P = gpu.Plan(pps, qs)
            assert P.has_crt == (name != "no CRT basis"), name
            out = (P.crtC(dz.clone()), P.crtInvC(dz.clone()), P.gaussianDec(dg.clone()))
            torch.cuda.synchronize()
        finally:
            if sw:
                gpu.debug_set(sw, False)
        if ref is None:
            ref = out
            assert close(out[0].cpu().numpy(), fr.crt_c_ext(pps, z).astype(np.complex128)), m
        for op, a, b in zip(("crtC", "crtInvC", "gaussianDec"), out, ref):
            assert torch.equal(a, b), (m, name, op)


# ---- batches past one grid sweep ------------------------------------------------------------------
@pytest.mark.parametrize("m", [25, 169, 32])
def test_float_grid_stride_small(gpu, m):
    """B = 2 * 4096 + 5 rows tiled from K distinct polynomials: copies sit at rows 4095, 4096, 8191 and 8192."""
    import torch
    P, pps = _plan(gpu, m)
    n, K, B = P.n, 7, 2 * GRID + 5
    rng = np.random.default_rng(m)
    z = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    g = rng.standard_normal((K, n))
    small = (P.crtC(z), P.crtInvC(z), P.gaussianDec(g))
    assert fr.rel_err(small[0], fr.crt_c_ext(pps, z)).max() <= bound_cplx(pps)
    assert fr.rel_err(small[2], fr.gaussian_dec_ext(pps, g)).max() <= bound_gauss(pps)
    rows = np.arange(B) % K
    assert B > 8192
    dz, dg = torch.from_numpy(z).cuda()[rows], torch.from_numpy(g).cuda()[rows]
    big = (P.crtC(dz.clone()), P.crtInvC(dz.clone()), P.gaussianDec(dg.clone()))
    for op, s, b in zip(("crtC", "crtInvC", "gaussianDec"), small, big):
        assert torch.equal(b, torch.from_numpy(s).cuda()[rows]), (m, op)
    rt = P.crtInvC(big[0])                                            # round trip over the whole batch
    err = torch.linalg.vector_norm(rt - dz, dim=1) / torch.linalg.vector_norm(dz, dim=1)
    assert float(err.max()) <= bound_cplx(pps), (m, float(err.max()))


@pytest.mark.parametrize("m", [2 ** 14, 2 ** 13 * 3])
def test_float_grid_stride_n8192(gpu, m):
    """B = 4097 polynomials of n = 8192 (0.5 GB complex): rows 0, 4095 and 4096 equal the B = 1 output bit for bit.
    (gaussianDec is the identity at 2^14 and launches nothing: 2^13 * 3 runs k_gauss at n = 8192.)"""
    import torch
    P, pps = _plan(gpu, m)
    n, B, hot = P.n, GRID + 1, [0, GRID - 1, GRID]
    z, g = stage_inputs(m)
    z, g = z[:1], g[:1]
    one = (P.crtC(z), P.crtInvC(z), P.gaussianDec(g))
    gen = torch.Generator(device="cuda").manual_seed(m)
    dz = torch.randn((B, n), dtype=torch.complex128, device="cuda", generator=gen)
    dg = torch.randn((B, n), dtype=torch.float64, device="cuda", generator=gen)
    dz[hot], dg[hot] = torch.from_numpy(z).cuda(), torch.from_numpy(g).cuda()
    for op, fn, x, want in (("crtC", P.crtC, dz, one[0]), ("crtInvC", P.crtInvC, dz, one[1]), ("gaussianDec", P.gaussianDec, dg, one[2])):
        y = fn(x.clone())
        assert torch.equal(y[hot], torch.from_numpy(want).cuda().expand(len(hot), n)), (m, op)
        del y
    y = P.crtInvC(P.crtC(dz.clone()))
    err = torch.linalg.vector_norm(y - dz, dim=1) / torch.linalg.vector_norm(dz, dim=1)
    assert float(err.max()) <= bound_cplx(pps), (m, float(err.max()))
    del y, dz, dg
    torch.cuda.empty_cache()


# ---- in place on a view, on a side stream ------------------------------------------------------------
@pytest.mark.parametrize("m", [169, 2 ** 13 * 3])
def test_float_ops_on_offset_view_and_side_stream(gpu, m):
    import torch
    P, pps = _plan(gpu, m)
    n, K, pre, post = P.n, 3, 2, 3
    rng = np.random.default_rng(m + 1)
    z = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    g = rng.standard_normal((K, n))
    want = (P.crtC(z), P.crtInvC(z), P.gaussianDec(g))
    side = torch.cuda.Stream()
    for op, fn, x, w in (("crtC", P.crtC, z, want[0]), ("crtInvC", P.crtInvC, z, want[1]), ("gaussianDec", P.gaussianDec, g, want[2])):
        sent = torch.from_numpy(rng.standard_normal((pre + K + post, n)) * (1 + 1j if np.iscomplexobj(x) else 1)).cuda()
        sent[pre:pre + K] = torch.from_numpy(x).cuda()
        before = sent.clone()
        view = sent[pre:pre + K]
        assert view.is_contiguous() and view.data_ptr() % 16 == 0 and view.data_ptr() != sent.data_ptr()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = fn(view)
        torch.cuda.synchronize()
        assert out.data_ptr() == view.data_ptr(), op
        assert torch.equal(sent[:pre], before[:pre]) and torch.equal(sent[pre + K:], before[pre + K:]), (m, op)
        assert torch.equal(view, torch.from_numpy(w).cuda()), (m, op)


# ---- limits ----------------------------------------------------------------------------------------
def test_float_ops_accept_n8192_and_refuse_beyond(gpu):
    import torch
    P, _ = _plan(gpu, 2 ** 14)
    g = torch.from_numpy(stage_inputs(2 ** 14)[1]).cuda()
    assert torch.equal(P.gaussianDec(g.clone()), g)                   # no odd prime: the identity, bit for bit
    z = torch.from_numpy(stage_inputs(2 ** 14)[0]).cuda()
    assert not torch.equal(P.crtC(z.clone()), z)
    for m in (2 ** 13 * 5, 3 ** 9, 17, 2 ** 4 * 17):                    # n = 16384, n = 13122, p = 17
        Q, _ = _plan(gpu, m)
        rng = np.random.default_rng(m)
        dz = torch.from_numpy(rng.standard_normal((2, Q.n)) + 1j * rng.standard_normal((2, Q.n))).cuda()
        dg = torch.from_numpy(rng.standard_normal((2, Q.n))).cuda()
        for fn, x in ((Q.crtC, dz), (Q.crtInvC, dz), (Q.gaussianDec, dg)):
            keep = x.clone()
            with pytest.raises(gpu.LolHipError):
                fn(x)
            torch.cuda.synchronize()
            assert torch.equal(x, keep), (m, fn.__name__)
    for m in (169, 2 ** 14):                                           # B = 0
        Q, _ = _plan(gpu, m)
        assert Q.crtC(np.zeros((0, Q.n), dtype=np.complex128)).shape == (0, Q.n)
        assert Q.crtInvC(np.zeros((0, Q.n), dtype=np.complex128)).shape == (0, Q.n)
        assert Q.gaussianDec(np.zeros((0, Q.n))).shape == (0, Q.n)
