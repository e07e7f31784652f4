"""The dense stage of the Gaussian map (k_gauss_dense, floatpath.hip) on the GPU (-m gpu): plans created with
dense_gauss=True (LOLHIP_PLAN_DENSE_GAUSS) at indices with a prime above 13.

  1 accuracy     every index of gauss_dense_cases.DENSE_INDICES within 16 u sum_s d_s of the long-double oracle (normwise
                 relative error), and the launcher's info line names a dense stage
  2 reference    lol-cpp's own tensorGaussianDec on the same inputs (golden_gauss_dense.npz), the 1e-12 contract
  3 parity       under the GAUSS_DENSE switch (a fresh child process) indices both routes take give the same bits
  4 batches      B = 5 = 2 + 3; B beyond one sweep of tiles; B = 0; in place on a view under a side stream, guard rows intact
  5 consumers    sampleDisc / sampleCont, encrypt -> decrypt, a tunnel hint into index 17, RingRLWE on a challenge line,
                 challenges.generate -> verify at m = 257 and m = 797
  6 default      the same calls on a default plan at m = 17: LOLHIP_ERR_INVALID, outputs untouched
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import enc_ref as er
import rlwe_ref as rr
from float_stages import batch, bound_gauss, fixture_columns, stage_inputs
from gauss_dense_cases import DENSE_INDICES, PARITY_INDICES
from oracle import floatref as fr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle import she_ref as sr
from oracle.oracle import Params
from test_float_stages import close

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_INVALID = -1
KEY = bytes(range(32))


def _plan(gpu, m, qs=None, dense=True):
    return gpu.Plan.for_index(m, qs or [lm.first_good_q(m, 1000)], dense_gauss=dense)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "golden_gauss_dense.npz"))


@pytest.fixture
def info(monkeypatch, capfd):
    """the launcher's lines since the last read: [[route of every stage]] of the k_gauss_dense launches, and how many
    launches of the register kernel"""
    monkeypatch.setenv("LOLHIP_GAUSS_INFO", "1")

    def read():
        dense, reg = [], 0
        for ln in capfd.readouterr().err.splitlines():
            if ln.startswith("k_gauss_dense: "):
                dense.append(ln.split(" stages ")[1].split())
            elif ln.startswith("k_gauss: "):
                reg += 1
        return dense, reg
    return read


# ---------------------------------------------------------------------------------------------
# 1 + 2. accuracy against the oracle and against lol-cpp's own outputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", DENSE_INDICES)
def test_gaussian_dec_at_large_primes(gpu, gold, info, m):
    """Bound asserted: 16 u sum_s d_s over the odd primes of the index, u = 2^-53 (2.8e-14 at m = 17, 1.4e-12 at
    m = 797).  The float64 restatement of the reference sits at 3e-16 .. 8e-16 on m = 17 .. 289."""
    pps = lm.factor_pps(m)
    P = _plan(gpu, m)
    assert P.gaussRoute() == 2 and P.n <= 8192
    g = stage_inputs(m)[1]
    assert g.shape == (batch(P.n), P.n)
    info()
    gd = P.gaussianDec(g)
    dense, reg = info()
    want_routes = ["reg" if p <= 13 else ("dense-cols" if rts >= 64 else "dense-rows") for p, rts in _odd_strides(pps)]
    assert dense == [want_routes] and reg == 0, (m, dense, reg)
    assert any(r != "reg" for r in want_routes)
    want = fr.gaussian_dec_ext(pps, g)
    assert close(gd, want.astype(np.float64)), ("gaussianDec vs oracle", m)
    e_g = float(fr.rel_err(gd, want).max())
    print(f"gauss-dense-error m={m} gaussianDec={e_g:.3e} bound={bound_gauss(pps):.3e}")
    assert e_g <= bound_gauss(pps), (m, e_g)
    assert close(gd[:, fixture_columns(m)], gold[f"m{m}_gauss"]), ("gaussianDec vs lol-cpp", m)


def _odd_strides(pps):
    """(p, rts) of every odd prime, rts the product of the totients of the prime powers before it"""
    out, rts = [], 1
    for p, e in pps:
        if p != 2:
            out.append((p, rts))
        rts *= (p - 1) * p ** (e - 1)
    return out


# ---------------------------------------------------------------------------------------------
# 3. both routes give the same bits
# ---------------------------------------------------------------------------------------------
def test_forced_dense_route_gives_the_register_route_bits(gpu, info, tmp_path):
    out = str(tmp_path / "forced.npz")
    env = dict(os.environ, LOLHIP_GAUSS_DENSE="1", LOLHIP_GAUSS_INFO="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gauss_dense_child.py"), out, *map(str, PARITY_INDICES)], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split(" stages ")[1].split() for ln in r.stderr.splitlines() if ln.startswith("k_gauss_dense: ")]
    forced = np.load(out)
    for i, m in enumerate(PARITY_INDICES):
        pps = lm.factor_pps(m)
        assert int(forced[f"route{m}"]) == 2
        assert lines[i] == [("dense-cols" if rts >= 64 else "dense-rows") for _, rts in _odd_strides(pps)], (m, lines[i])
        P = _plan(gpu, m)
        assert P.gaussRoute() == 1                                   # no switch here: register stages only
        info()
        got = P.gaussianDec(stage_inputs(m)[1])
        assert info() == ([], 1)
        assert np.array_equal(_bits(got), _bits(forced[f"m{m}"])), m
        assert np.array_equal(_bits(got), _bits(_plan(gpu, m, dense=False).gaussianDec(stage_inputs(m)[1]))), m
    assert {r_ for ln in lines for r_ in ln} == {"dense-rows", "dense-cols"}


# ---------------------------------------------------------------------------------------------
# 4. batch shapes and calling conventions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [23, 257])
def test_batch_shapes(gpu, m):
    import torch
    P = _plan(gpu, m)
    n = P.n
    rng = np.random.default_rng(m)
    x = rng.standard_normal((5, n)) * 2.0
    whole = P.gaussianDec(x)
    assert np.array_equal(_bits(whole), _bits(np.concatenate([P.gaussianDec(x[:2]), P.gaussianDec(x[2:])])))
    assert fr.rel_err(whole, fr.gaussian_dec_ext(lm.factor_pps(m), x)).max() <= bound_gauss(lm.factor_pps(m))
    assert P.gaussianDec(np.zeros((0, n))).shape == (0, n)
    # in place on a row-offset view under a side stream; the guard rows around the slab stay as they were
    pre, post, K = 2, 3, 5
    sent = torch.from_numpy(rng.standard_normal((pre + K + post, n))).cuda()
    sent[pre:pre + K] = torch.from_numpy(x).cuda()
    before = sent.clone()
    view = sent[pre:pre + K]
    assert view.is_contiguous() and view.data_ptr() != sent.data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = P.gaussianDec(view)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    assert torch.equal(sent[:pre], before[:pre]) and torch.equal(sent[pre + K:], before[pre + K:])
    assert np.array_equal(_bits(view), _bits(whole))


def test_batch_beyond_one_sweep_of_tiles(gpu, info):
    """m = 23, B = 5000: tiles of 16 items (313 tiles, the last with 8 live items); 64 sampled rows, the first and the
    last among them, equal their single-row runs bit for bit"""
    import torch
    P = _plan(gpu, 23)
    n, B = P.n, 5000
    rng = np.random.default_rng(5000)
    x = rng.standard_normal((B, n))
    info()
    big = P.gaussianDec(torch.from_numpy(x).cuda()).cpu().numpy()
    assert info() == ([["dense-rows"]], 0)
    rows = np.unique(np.concatenate([[0, B - 1, B - 8, B - 9], rng.choice(B, 60, replace=False)]))[:64]
    for i in rows:
        assert np.array_equal(_bits(big[i]), _bits(P.gaussianDec(x[i:i + 1])[0])), i
    assert fr.rel_err(big[rows], fr.gaussian_dec_ext([(23, 1)], x[rows])).max() <= bound_gauss([(23, 1)])


# ---------------------------------------------------------------------------------------------
# 5. the consumers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,svar", [(17, 0.28125), (23, 4.0), (257, 4.0)])
def test_sample_disc_matches_restatement(gpu, cpuref, m, svar):
    """the condition of test_rlwe.py's Disc test; the restatement has no coefficient near a tie on these three inputs"""
    from test_rlwe import _crt_of_dec
    qs = [next(lm.good_qs(m, 2 ** 27))]
    pps = rr.factor_pps(m)
    r = gpu.RLWE(_plan(gpu, m, qs))
    n, B, ctr = r.plan.n, 3, 2 ** 32 - 2
    s = r.secret(key=KEY, ctr=77)
    assert np.array_equal(s.cpu().numpy(), rr.uniform(KEY, rr.DOM_RLWE_SECRET, 77, 1, n, qs)[0])
    a, b = r.sampleDisc(s, B, svar, key=KEY, ctr=ctr)
    a_h, b_h, s_h = a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(a_h, rr.uniform(KEY, rr.DOM_RLWE_UNIFORM, ctr, B, n, qs))
    e = r.errorTermDisc(s, a, b).cpu().numpy()
    want, near = er.round_coset(rr.gaussian_dec(pps, KEY, ctr, B, svar), np.zeros((B, n), dtype=np.int64), 1)
    bad = e != want
    assert bad.sum() <= 4 and near[bad].all(), (int(bad.sum()), int(near.sum()))
    qv = np.array(qs, dtype=object)
    b_want = (a_h.astype(object) * s_h.astype(object)[None] + _crt_of_dec(cpuref, m, qs, e).astype(object)) % qv
    assert np.array_equal(b_h, b_want.astype(np.int64))


def test_sample_cont_matches_restatement(gpu, cpuref):
    from test_rlwe import _as_dec
    m, svar = 23, 4.0
    q = next(lm.good_qs(m, 2 ** 27))
    pps = rr.factor_pps(m)
    r = gpu.RLWE(_plan(gpu, m, [q]))
    n, B, ctr = r.plan.n, 3, 1000 + m
    s = r.secret(key=KEY, ctr=3)
    a, b = r.sampleCont(s, B, svar, key=KEY, ctr=ctr)
    a_h, b_h = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a_h, rr.uniform(KEY, rr.DOM_RLWE_UNIFORM, ctr, B, n, [q]))
    assert (b_h >= 0).all() and (b_h < float(q)).all()
    g = rr.gaussian_dec(pps, KEY, ctr, B, svar)
    e = r.errorTermCont(s, a, b).cpu().numpy()
    assert (np.abs(e - g) <= 1e-12 * np.abs(g) + float(q) * 2.0 ** -52).all(), float(np.abs(e - g).max())
    x = _as_dec(cpuref, m, [q], a_h, s.cpu().numpy())[..., 0]
    d = np.abs(b_h - rr.cont_sample(x, g, q))
    d = np.minimum(d, float(q) - d)
    assert (d <= 1e-12 * np.abs(g) + float(q) * 2.0 ** -52).all()


def test_encrypt_then_decrypt_at_index_136(gpu, cpuref):
    from test_encrypt import _moduli, _rep, _restated_e, _small_key
    m, m2, p = 8, 136, 16
    qs = _moduli(m2, 30, 2)
    pq, pp = _plan(gpu, m2, qs), _plan(gpu, m2, [p])
    x_p = gpu.Ext(gpu.Plan.for_index(m, [p]), pp)
    rng = np.random.default_rng(m2 + p)
    B, svar, ctr = 3, 1.5, 1000 + m2
    key = rng.bytes(32)
    pt = rng.integers(-p + 1, p, size=(B, x_p.lo.n), dtype=np.int64)
    s_crt = _small_key(cpuref, m2, qs, rng)
    out_crt = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, ext=x_p, out_crt=True)
    out_pow = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, ext=x_p)
    rep = _rep(cpuref, m, m2, p, pt)
    e_want, near = _restated_e(m2, p, svar, key, ctr, B, rep)
    e_pow = pq.errorTerm(out_pow, s_crt, p)
    assert np.array_equal(e_pow, pq.errorTerm(out_crt, s_crt, p, cs_crt=True))
    bad = e_pow != e_want
    assert bad.sum() <= 4 and near[bad].all(), (int(bad.sum()), int(near.sum()))
    assert ((e_pow - rep) % p == 0).all()
    want = pt % p
    assert np.array_equal(pq.decrypt(out_pow, s_crt, pp, ext=x_p), want)
    assert np.array_equal(pq.decrypt(out_crt, s_crt, pp, ext=x_p, cs_crt=True), want)
    # genSK's sampler at the same index
    z = pq.errorRounded(3.0, B=4, key=KEY, ctr=7).cpu().numpy()
    x = fr.gaussian_dec(pq.pps, er.gaussians(KEY, er.DOM_ERR_ROUNDED, 7, 4, pq.n, er.sigma(pq.pps, 3.0))).reshape(4, pq.n)
    zw, near = er.round_coset(x, np.zeros_like(z), 1)
    assert (z != zw).sum() <= 4 and near[z != zw].all()


def test_tunnel_hint_into_index_17(gpu, cpuref):
    """e = 1, r = 8, s = 17: the shape test_kshint.py's error test sees refused on a default plan"""
    from test_kshint import _bmul, _check_rows, sm_engine
    e, r, s, base = 1, 8, 17, 0
    p = lm.first_good_q(136, 40)
    g = lm.good_qs(136, 2 ** 29)
    qs = [next(g), next(g)]
    pe, pr, ps = (lm.factor_pps(m) for m in (e, r, s))
    rng = np.random.default_rng(3000 + e + r + s + base)
    GE, GR, GS = gpu.Plan(pe, qs), gpu.Plan(pr, qs), gpu.Plan(ps, qs, dense_gauss=True)
    she_in = sm.SHE(GR, gpu.Plan(pr, [p]), qs, p, rng)
    she_out = sm.SHE(GS, gpu.Plan(ps, [p], dense_gauss=True), qs, p, rng)
    she_in.keygen(); she_out.keygen()
    XR, XS = gpu.Ext(GE, GR), gpu.Ext(GE, GS)
    rel_index = [row[0] for row in lm.ext_indices_coeffs(pe, pr)]
    rel = len(rel_index)
    f_vals = rng.integers(0, p, size=(rel, she_out.n), dtype=np.int64)
    v = f_vals.astype(object) % p
    ys_crt = GS.crt(she_out.reduce(np.where(2 * v < p, v, v - p)))
    key, ctr, svar = rng.bytes(32), 17, 0.5
    hints = XR.tunnelHint(XS, ys_crt, she_in.s_crt[0], she_out.s_crt[0], svar, base, key=key, ctr=ctr)
    assert hints.shape == (rel, GS.decomposeLen(base), 2, she_out.n, 2)
    PE, PR, PS = Params(pe, qs), Params(pr, qs), Params(ps, qs)
    comps = []
    for idx in rel_index:
        pi = np.zeros((1, she_in.n, 2), dtype=np.int64)
        pi[0, idx, :] = 1
        sp = cpuref.crtinv(PR, _bmul(cpuref, PR, cpuref.crt(PR, pi), she_in.s_crt[0]))
        comps.append(sr.evallin(cpuref, PE, PR, PS, cpuref.linv(PR, sp).reshape(1, she_in.n, 2), ys_crt).reshape(she_out.n, 2))
    _check_rows(cpuref, PS, GS, hints, np.stack(comps), she_out.s_crt[0], svar, base, key, ctr)
    B = 2
    x = rng.integers(0, p, size=(B, she_in.n), dtype=np.int64)
    out = sm.tunnel(she_in, sm_engine(XR, XS), ys_crt, hints, base, she_in.encrypt(x))
    out["c"] = [GS.crtInv(np.ascontiguousarray(c)) for c in out["c"]]
    got = she_out.decrypt(out)
    PEp, PRp, PSp = (Params(q_, [p]) for q_ in (pe, pr, ps))
    x_dec = cpuref.linv(PRp, x[..., None]).reshape(B, she_in.n, 1)
    f_crt = cpuref.crt(PSp, f_vals[..., None]).reshape(rel, she_out.n, 1)
    want = cpuref.crtinv(PSp, sr.evallin(cpuref, PEp, PRp, PSp, x_dec, f_crt)).reshape(B, she_out.n)
    assert np.array_equal(got, want) and want.any()


def test_ring_rlwe_disc_on_line_287(gpu):
    import rlwe_ring_ref as rg
    import torch
    m, q, svar = 179, 2048, 5.6179775280898875e-3
    assert rg.challenge_lines()[287] == ("Disc", m, q, svar)
    r = gpu.RingRLWE(_plan(gpu, m, [q]))
    _, shat = r.secret(key=KEY, ctr=0)
    _, other = r.secret(key=KEY, ctr=1)
    assert not torch.equal(other, shat)
    bound = r.errorBound(m, svar, eps=2.0 ** -25, kind="disc")
    assert bound == rr.error_bound_disc(m, svar, 2.0 ** -25)
    a, b = r.sampleDisc(shat, 3, svar, key=KEY, ctr=10)
    assert r.validDisc(bound, shat, a, b).all() and not r.validDisc(bound, other, a, b).any()


@pytest.mark.parametrize("ids", [(344, 347), (400, 401)])
def test_challenges_generate_then_verify(gpu, tmp_path, ids):
    """one Cont and one Disc line each of m = 257 (plan and ring route) and m = 797, cut to 2 instances of 3 samples"""
    from lol_amd import challenges as ch
    text = open(os.path.join(HERE, "golden", "challenge_params.txt")).read()
    recs = {r.challID: r for r in ch.parse_params(text, num_instances=2)}
    root = str(tmp_path)
    kinds = set()
    for i in ids:
        cp = dataclasses.replace(recs[i], numSamples=3)
        assert cp.m in (257, 797) and cp.kind in ("Cont", "Disc")
        kinds.add(cp.kind)
        name = ch.generate(cp, root, KEY, beacon=(1478822400, 63), ctr_s=5, ctr=100)
        res = ch.verify(root, name)
        assert sorted(res) == [0, 1] and all(ok and f == 0 for ok, f, _ in res.values()), (i, res)
        _, _, s, a, b, _ = ch.read_tree(root, name)
        ok, (fails, _) = ch.verify_arrays(cp, np.roll(s, 1, axis=0), a, b)
        assert not np.asarray(ok).any(), (i, fails)
    assert kinds == {"Cont", "Disc"}


# ---------------------------------------------------------------------------------------------
# 6. default plans refuse as before
# ---------------------------------------------------------------------------------------------
def test_default_plan_at_17_refuses_with_outputs_untouched(gpu):
    import torch
    L = gpu.lib()
    SENT = 0x5A5A5A5A
    qs = [next(lm.good_qs(17, 2 ** 27))]
    D = _plan(gpu, 17, qs, dense=False)
    assert D.gaussRoute() == 0
    n, B = D.n, 2
    g = torch.from_numpy(np.random.default_rng(17).standard_normal((B, n))).cuda()
    keep = g.clone()
    assert L.lolhip_gaussian_dec_batch(D._h, None, g.data_ptr(), B) == ERR_INVALID
    with pytest.raises(gpu.LolHipError) as ei:
        D.gaussianDec(g)
    assert ei.value.code == ERR_INVALID

    def sent(*shape):
        return torch.full(shape, SENT, dtype=torch.int64, device="cuda")
    z = sent(B, n)
    assert L.lolhip_error_rounded_batch(D._h, None, 1.0, KEY, 0, z.data_ptr(), None, B) == ERR_INVALID
    s = torch.zeros((n, 1), dtype=torch.int64, device="cuda")
    a, b, w = sent(B, n, 1), sent(B, n, 1), sent(max(L.lolhip_rlwe_work_len(D._h, 0, B), 1))
    for kind in (0, 1):
        assert L.lolhip_rlwe_sample_batch(D._h, None, kind, 0, s.data_ptr(), 1.0, KEY, 0, a.data_ptr(), b.data_ptr(), w.data_ptr(),
                                          B) == ERR_INVALID
    nL = D.decomposeLen(0)
    vals, hints = torch.zeros((B, n, 1), dtype=torch.int64, device="cuda"), sent(B, nL, 2, n, 1)
    hw = sent(max(L.lolhip_kshint_work_len(D._h, 0, B), 1))
    assert L.lolhip_kshint_batch(D._h, None, s.data_ptr(), vals.data_ptr(), 1.0, 0, KEY, 0, hints.data_ptr(), hw.data_ptr(),
                                 B) == ERR_INVALID
    pp = _plan(gpu, 17, [16], dense=False)
    cs, ew = sent(2, B, n, 1), sent(max(L.lolhip_encrypt_work_len(D._h, B), 1))
    pt = torch.zeros((B, n), dtype=torch.int64, device="cuda")
    assert L.lolhip_encrypt_batch(D._h, pp._h, None, None, pt.data_ptr(), s.data_ptr(), 1.0, KEY, 0, 0, cs.data_ptr(),
                                  ew.data_ptr(), B) == ERR_INVALID
    so, ao, bo = sent(2, n, 1), sent(6, n, 1), sent(6, n, 1)
    cw = sent(max(L.lolhip_chall_work_len(D._h, 0, 2, 3), 1))
    assert L.lolhip_chall_generate_batch(D._h, None, 0, 0, 1.0, KEY, 0, 0, 2, 3, so.data_ptr(), ao.data_ptr(), bo.data_ptr(),
                                         cw.data_ptr()) == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(g, keep)
    for t in (z, a, b, w, hints, hw, cs, ew, so, ao, bo, cw):
        assert bool((t == SENT).all())
    # the opted-in plan of the same index and modulus takes them
    assert _plan(gpu, 17, qs).errorRounded(1.0, B=B, key=KEY).shape == (B, n)
