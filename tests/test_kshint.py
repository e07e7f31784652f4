"""Key-switch and tunnel hints on the GPU (lolhip_kshint_batch, lolhip_tunnel_hint_batch; lol-apps SymmSHE.hs:262-296,
330-355, 531-545).

The reference is the numpy restatement of tests/kshint_ref.py over tests/enc_ref.py (ChaCha20, the stream layout,
Box-Muller), with oracle.floatref.gaussian_dec for the decoding-basis map and the CPU oracle for crt, crtInv, l, lInv
and evalLin.

    restatement     c1 exactly; h0 + c1 s - g_j val taken to the decoding basis = the restated errorRounded (domain 3),
                    except within 1e-9 of a rounding tie
    key switching   device key, device ciphertexts, device hints: KSQuad (then modSwitch) and KSLinear decrypt
    tunnel          device tunnelHint + tunnel decrypts to evalLin f x; each row's value term is g_j comps_i
    determinism     a batch split in two at ctr, ctr + 2L is the same batch; a side stream; another key
    errors          every status, decided before any launch: the output stays untouched
    wire            a device hint through kshint_write -> kshint_read comes back identical
"""
import numpy as np
import pytest

import enc_ref as er
import kshint_ref as kr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle import she_ref as sr
from oracle.oracle import Params


def _moduli(m, bits, T):
    g = lm.good_qs(m, 2 ** (bits - 1))
    return [next(g) for _ in range(T)]


def _small_key(cpuref, P, rng):
    """a secret key with decoding-basis coefficients in {-1, 0, 1}, CRT basis [n][T] (the CPU oracle)"""
    z = rng.integers(-1, 2, size=(1, P.n)).astype(object)
    res = np.stack([(z % q).astype(np.int64) for q in P.qs], axis=-1)
    return np.ascontiguousarray(cpuref.crt(P, cpuref.l(P, res)).reshape(P.n, P.T))


def _uniform(rng, B, n, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=(B, n), dtype=np.int64) for q in qs], axis=-1))


def _bmul(cpuref, P, a, b):
    """pointwise a * b mod q_t, b broadcast to a's shape"""
    a = np.ascontiguousarray(a, dtype=np.int64)
    return cpuref.mul(P, a, np.ascontiguousarray(np.broadcast_to(b, a.shape))).reshape(a.shape)


def _noise_rows(cpuref, P, hints, vals_crt, s_crt, g):
    """e_j in the decoding basis, centred, [B*L][n]: crtInv, lInv of h0 + c1 s - g_j val"""
    B, L = hints.shape[:2]
    qv = np.array(P.qs, dtype=np.int64)
    h0, c1 = hints[:, :, 0], hints[:, :, 1]
    c1s = _bmul(cpuref, P, c1.reshape(B * L, P.n, P.T), s_crt).reshape(B, L, P.n, P.T)
    gv = np.stack([_bmul(cpuref, P, vals_crt, g[j]) for j in range(L)], axis=1)        # [B][L][n][T]
    x = (h0 + c1s) % qv
    x = (x - gv) % qv
    x = cpuref.linv(P, cpuref.crtinv(P, x.reshape(B * L, P.n, P.T))).reshape(B * L, P.n, P.T)
    x = np.where(2 * x < qv, x, x - qv)
    assert (x == x[..., :1]).all()                                     # small: the same integer in every component
    return x[..., 0]


def _check_rows(cpuref, P, pq, hints, vals_crt, s_crt, svar, base, key, ctr):
    B, L = hints.shape[:2]
    g = pq.gadget(base)
    assert L == g.shape[0]
    assert np.array_equal(hints[:, :, 1].reshape(B * L, P.n, P.T), kr.uniform_crt(key, kr.DOM_HINT_UNIFORM, ctr, B * L, P.n, P.qs))
    e = _noise_rows(cpuref, P, hints, vals_crt, s_crt, g)
    want, near = kr.rounded_gaussians(key, ctr, B * L, P.pps, P.n, svar)
    bad = e != want
    assert bad.sum() <= 4 and near[bad].all() and (np.abs(e - want) <= 1).all(), (int(bad.sum()), int(near.sum()))
    assert np.abs(e).max() > 0


# ---------------------------------------------------------------------------------------------
# 1. restatement
# ---------------------------------------------------------------------------------------------
# (m', (bits, T), bases, B)
SHAPES = [(2048, (30, 1), (0, 2, 256), 2), (2048, (30, 2), (0, 256), 2), (64, (30, 2), (2,), 3), (45, (30, 3), (0, 256), 2),
          (14400, (30, 2), (0, 256), 1), (2 ** 15, (59, 4), (0, 256), 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,mods,bases,B", SHAPES)
def test_kshint_matches_restatement(gpu, cpuref, m, mods, bases, B):
    qs = _moduli(m, *mods)
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(m + len(qs))
    s_crt = _small_key(cpuref, P, rng)
    vals = _uniform(rng, B, P.n, qs)
    for base in bases:
        key, ctr, svar = rng.bytes(32), 2 ** 32 - 3 + base, 2.5
        hints = pq.ksHint(s_crt, vals, svar, base, key=key, ctr=ctr)
        assert hints.shape == (B, pq.decomposeLen(base), 2, P.n, len(qs))
        _check_rows(cpuref, P, pq, hints, vals, s_crt, svar, base, key, ctr)


# ---------------------------------------------------------------------------------------------
# 2. key switching with device key, ciphertexts and hints
# ---------------------------------------------------------------------------------------------
def _device_she(gpu, pq, pp, qs, p, rng, key, ctr):
    she = sm.SHE(pq, pp, qs, p, rng)
    z = pq.errorRounded(0.5, B=1, key=key, ctr=ctr).cpu().numpy()     # genSK
    she.s = np.ascontiguousarray(pq.l(she.reduce(z)))
    she.s_crt = np.ascontiguousarray(pq.crt(she.s))
    return she


@pytest.mark.gpu
@pytest.mark.parametrize("m,p,lower", [(64, 257, 2 ** 29), (45, 181, 2 ** 30)])
def test_key_switching_with_device_hints(gpu, cpuref, m, p, lower):
    pps = lm.factor_pps(m)
    g = lm.good_qs(m, lower)
    qs = [next(g), next(g)]
    rng = np.random.default_rng(m + p)
    pq, pp = gpu.Plan(pps, qs), gpu.Plan(pps, [p])
    kk = bytes(range(32, 64))
    she = _device_she(gpu, pq, pp, qs, p, rng, kk, 0)
    B = 3
    a = rng.integers(0, p, size=(B, pq.n), dtype=np.int64)
    b = rng.integers(0, p, size=(B, pq.n), dtype=np.int64)
    ca = pq.encrypt(a, she.s_crt[0], pp, 0.5, key=kk, ctr=0)
    cb = pq.encrypt(b, she.s_crt[0], pp, 0.5, key=kk, ctr=B)
    cta = {"enc": "LSD", "k": 0, "l": 1, "c": [ca[0], ca[1]]}
    ctb = {"enc": "LSD", "k": 0, "l": 1, "c": [cb[0], cb[1]]}
    prod_ = she.mul(cta, ctb)
    want = cpuref.polymul(Params(pps, [p]), a[..., None], b[..., None]).reshape(a.shape)
    ctr = 0
    for base in (0, 256):
        hint = pq.ksQuadCircHint(she.s_crt[0], 0.5, base, key=kk, ctr=ctr)
        ctr += pq.decomposeLen(base)
        assert hint.shape == (pq.decomposeLen(base), 2, pq.n, 2)
        lin = she.key_switch_quad(hint, base, prod_)
        assert np.array_equal(she.decrypt(lin), want), ("KSQuad", base)
        lin_small, she2 = she.mod_switch_drop_first(lin, gpu.Plan(pps, qs[1:]))
        assert np.array_equal(she2.decrypt(lin_small), want), ("KSQuad . modSwitch", base)
    # KSLinear: Enc under s_in, keySwitchLinear with ksLinearHint s_out s_in, Dec under s_out
    she_out = _device_she(gpu, pq, pp, qs, p, rng, kk, 1)
    ct = she.toMSD(cta)
    for base in (0, 256):
        hint = pq.ksLinearHint(she_out.s_crt[0], she.s_crt[0], 0.5, base, key=kk, ctr=ctr)
        ctr += pq.decomposeLen(base)
        add = np.ascontiguousarray(np.stack([pq.crt(ct["c"][0]), np.zeros_like(ct["c"][0])]))
        out = pq.keySwitch(ct["c"][1], base, hint, addend=add)
        lin = {"enc": "MSD", "k": 0, "l": ct["l"], "c": [pq.crtInv(np.ascontiguousarray(out[0])),
                                                        pq.crtInv(np.ascontiguousarray(out[1]))]}
        assert np.array_equal(she_out.decrypt(lin), a), ("KSLinear", base)


# ---------------------------------------------------------------------------------------------
# 3. tunnel hints
# ---------------------------------------------------------------------------------------------
TUNNEL_CASES = [(4, 12, 20), (8, 16, 40), (1, 8, 8), (128, 128 * 7, 128 * 13)]   # test_she_properties' cases and chain hop


@pytest.mark.gpu
@pytest.mark.parametrize("e,r,s", TUNNEL_CASES)
@pytest.mark.parametrize("base", [0, 16])
def test_tunnel_with_device_hints(gpu, cpuref, e, r, s, base):
    import math
    lcm = r * s // math.gcd(r, s)
    p = lm.first_good_q(lcm, 40)
    g = lm.good_qs(lcm, 2 ** 29)
    qs = [next(g), next(g)]
    pe, pr, ps = (lm.factor_pps(m) for m in (e, r, s))
    rng = np.random.default_rng(3000 + e + r + s + base)
    GE, GR, GS = gpu.Plan(pe, qs), gpu.Plan(pr, qs), gpu.Plan(ps, qs)
    she_in = sm.SHE(GR, gpu.Plan(pr, [p]), qs, p, rng)
    she_out = sm.SHE(GS, gpu.Plan(ps, [p]), qs, p, rng)
    she_in.keygen(); she_out.keygen()
    XR, XS = gpu.Ext(GE, GR), gpu.Ext(GE, GS)
    rel_index = [row[0] for row in lm.ext_indices_coeffs(pe, pr)]
    assert list(XR.table(5).reshape(len(rel_index), -1)[:, 0]) == rel_index
    rel = len(rel_index)
    f_vals = rng.integers(0, p, size=(rel, she_out.n), dtype=np.int64)
    v = f_vals.astype(object) % p
    ys_crt = GS.crt(she_out.reduce(np.where(2 * v < p, v, v - p)))                  # f'q on the relative decoding basis
    key, ctr, svar = rng.bytes(32), 17, 0.5
    hints = XR.tunnelHint(XS, ys_crt, she_in.s_crt[0], she_out.s_crt[0], svar, base, key=key, ctr=ctr)
    nL = GS.decomposeLen(base)
    assert hints.shape == (rel, nL, 2, she_out.n, 2)
    # the value term of every row is g_j comps_i, comps_i = evalLin f' (s_in p_i) by the CPU oracle
    PE, PR, PS = Params(pe, qs), Params(pr, qs), Params(ps, qs)
    comps = []
    for idx in rel_index:
        pi = np.zeros((1, she_in.n, 2), dtype=np.int64)
        pi[0, idx, :] = 1
        sp = cpuref.crtinv(PR, _bmul(cpuref, PR, cpuref.crt(PR, pi), she_in.s_crt[0]))
        comps.append(sr.evallin(cpuref, PE, PR, PS, cpuref.linv(PR, sp).reshape(1, she_in.n, 2), ys_crt).reshape(she_out.n, 2))
    _check_rows(cpuref, PS, GS, hints, np.stack(comps), she_out.s_crt[0], svar, base, key, ctr)
    # ... and the hints tunnel: Dec_skout (tunnel (Enc_skin x)) = evalLin f x over Z_p
    B = 2
    x = rng.integers(0, p, size=(B, she_in.n), dtype=np.int64)
    ct = she_in.encrypt(x)
    out = sm.tunnel(she_in, sm_engine(XR, XS), ys_crt, hints, base, ct)
    out["c"] = [GS.crtInv(np.ascontiguousarray(c)) for c in out["c"]]
    got = she_out.decrypt(out)
    PEp, PRp, PSp = (Params(q_, [p]) for q_ in (pe, pr, ps))
    x_dec = cpuref.linv(PRp, x[..., None]).reshape(B, she_in.n, 1)
    f_crt = cpuref.crt(PSp, f_vals[..., None]).reshape(rel, she_out.n, 1)
    want = cpuref.crtinv(PSp, sr.evallin(cpuref, PEp, PRp, PSp, x_dec, f_crt)).reshape(B, she_out.n)
    assert np.array_equal(got, want), (e, r, s, base)
    assert want.any()


class sm_engine:
    """lol_amd.Ext pairs as the tunnel engine of oracle/she_model.py"""

    def __init__(self, XR, XS):
        self.XR, self.XS = XR, XS

    def tunnel(self, c0_dec, c1_pow, ys_crt, hints, base): return self.XR.tunnel(self.XS, c0_dec, c1_pow, ys_crt, hints, base)


# ---------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,base", [(2048, 256), (45, 0)])
def test_kshint_is_a_function_of_key_and_position(gpu, cpuref, m, base):
    import torch
    qs = _moduli(m, 30, 2)
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(m)
    s_crt = torch.from_numpy(_small_key(cpuref, P, rng)).cuda()
    vals = torch.from_numpy(_uniform(rng, 5, P.n, qs)).cuda()
    nL = pq.decomposeLen(base)
    key, c = bytes(range(5, 37)), 2 ** 32 - 7
    whole = pq.ksHint(s_crt, vals, 1.0, base, key=key, ctr=c)
    parts = torch.cat([pq.ksHint(s_crt, vals[:2].contiguous(), 1.0, base, key=key, ctr=c),
                       pq.ksHint(s_crt, vals[2:].contiguous(), 1.0, base, key=key, ctr=c + 2 * nL)])
    assert torch.equal(whole, parts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = pq.ksHint(s_crt, vals, 1.0, base, key=key, ctr=c, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(whole, on_side)
    other = pq.ksHint(s_crt, vals, 1.0, base, key=bytes(range(6, 38)), ctr=c)
    assert (other[:, :, 1] == whole[:, :, 1]).double().mean().item() < 1e-4


# ---------------------------------------------------------------------------------------------
# 5. errors: decided on the host, before any launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kshint_errors_leave_output_untouched(gpu):
    import torch
    L = gpu.lib()
    SENT = 0x5A5A5A5A
    key = bytes(32)
    ERR_INVALID, ERR_NO_CRT = -1, -3

    def run(pq, svar=1.0, base=0, b=2):
        nL = max(L.lolhip_decompose_len(pq._h, base), 1)
        bb = max(b, 1)
        s_crt = torch.zeros((pq.n, pq.T), dtype=torch.int64, device="cuda")
        vals = torch.zeros((bb, pq.n, pq.T), dtype=torch.int64, device="cuda")
        wl = L.lolhip_kshint_work_len(pq._h, base if base == 0 or base >= 2 else 0, bb)
        work = torch.zeros((max(wl, 1),), dtype=torch.int64, device="cuda")
        out = torch.full((bb, nL, 2, pq.n, pq.T), SENT, dtype=torch.int64, device="cuda")
        rc = L.lolhip_kshint_batch(pq._h, None, s_crt.data_ptr(), vals.data_ptr(), svar, base, key, 3, out.data_ptr(),
                                   work.data_ptr(), b)
        torch.cuda.synchronize()
        return rc, bool((out == SENT).all())

    qs = [1017857, 1032193]
    pq = gpu.Plan.for_index(2048, qs)
    assert run(pq) == (0, False)
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        assert run(pq, svar=sv) == (ERR_INVALID, True), sv
    assert run(pq, b=-1) == (ERR_INVALID, True)
    for base in (1, -1, -256):
        assert run(pq, base=base) == (ERR_INVALID, True), base
    g = lm.good_qs(16, 2 ** 20)
    assert run(gpu.Plan.for_index(16, [next(g) for _ in range(17)])) == (ERR_INVALID, True)      # T > 16
    for mm in (17, 3 * 2 ** 14, 2 ** 16):                                                       # sampler limits
        assert run(gpu.Plan.for_index(mm, [next(lm.good_qs(mm, 2 ** 29))])) == (ERR_INVALID, True), mm
    no_crt = [q for q in range(1000003, 1001000, 2) if lm.is_prime(q) and (q - 1) % 2048][:2]
    assert run(gpu.Plan.for_index(2048, no_crt)) == (ERR_NO_CRT, True)
    with pytest.raises(gpu.LolHipError) as ei:
        pq.ksHint(np.zeros((pq.n, 2), dtype=np.int64), np.zeros((1, pq.n, 2), dtype=np.int64), -1.0, 0)
    assert ei.value.code == ERR_INVALID

    # tunnelHint
    qs2 = [next(lm.good_qs(60, 2 ** 29))]
    qs2.append(next(q for q in lm.good_qs(60, qs2[0] + 1)))

    def run_t(xr, xs, svar=1.0, base=0, n_in=None, n_out=None):
        R, S = xr.hi, xs.hi
        rel = R.n // xr.lo.n
        nL = max(L.lolhip_decompose_len(S._h, base), 1)
        ys = torch.zeros((rel, S.n, S.T), dtype=torch.int64, device="cuda")
        s_in = torch.zeros((R.n, R.T), dtype=torch.int64, device="cuda")
        s_out = torch.zeros((S.n, S.T), dtype=torch.int64, device="cuda")
        wl = L.lolhip_tunnel_hint_work_len(xr._h, xs._h, base if base == 0 or base >= 2 else 0)
        work = torch.zeros((max(wl, 1),), dtype=torch.int64, device="cuda")
        out = torch.full((rel, nL, 2, S.n, S.T), SENT, dtype=torch.int64, device="cuda")
        rc = L.lolhip_tunnel_hint_batch(xr._h, xs._h, None, ys.data_ptr(), s_in.data_ptr(), s_out.data_ptr(), svar, base,
                                        key, 0, out.data_ptr(), work.data_ptr())
        torch.cuda.synchronize()
        return rc, bool((out == SENT).all())

    PE, PR, PS = (gpu.Plan.for_index(m, qs2) for m in (4, 12, 20))
    XR, XS = gpu.Ext(PE, PR), gpu.Ext(PE, PS)
    assert run_t(XR, XS) == (0, False)
    for sv in (0.0, float("nan")):
        assert run_t(XR, XS, svar=sv) == (ERR_INVALID, True)
    assert run_t(XR, XS, base=1) == (ERR_INVALID, True)
    # extensions that do not share E' (or the moduli)
    assert run_t(XR, gpu.Ext(gpu.Plan.for_index(2, qs2), gpu.Plan.for_index(20, qs2))) == (ERR_INVALID, True)
    qs3 = [qs2[1], qs2[0]]
    assert run_t(XR, gpu.Ext(gpu.Plan.for_index(4, qs3), gpu.Plan.for_index(20, qs3))) == (ERR_INVALID, True)
    # an S' beyond the sampler's limits (prime 17); no CRT basis
    g136 = lm.good_qs(136, 2 ** 29)
    q17 = [next(g136), next(g136)]
    P1 = gpu.Plan.for_index(1, q17)
    assert run_t(gpu.Ext(P1, gpu.Plan.for_index(8, q17)), gpu.Ext(P1, gpu.Plan.for_index(17, q17))) == (ERR_INVALID, True)
    nc = [q for q in range(1000003, 1002000, 2) if lm.is_prime(q) and (q - 1) % 20 and (q - 1) % 12][:2]
    PEn, PRn, PSn = (gpu.Plan.for_index(m, nc) for m in (4, 12, 20))
    assert run_t(gpu.Ext(PEn, PRn), gpu.Ext(PEn, PSn)) == (ERR_NO_CRT, True)
    # the Python layer: keys of the wrong plans
    rel = PR.n // PE.n
    ys = np.zeros((rel, PS.n, 2), dtype=np.int64)
    with pytest.raises(gpu.LolHipError) as ei:
        XR.tunnelHint(XS, ys, np.zeros((PS.n, 2), dtype=np.int64), np.zeros((PS.n, 2), dtype=np.int64), 1.0, 0)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(gpu.LolHipError) as ei:
        XR.tunnelHint(XS, ys, np.zeros((PR.n, 2), dtype=np.int64), np.zeros((PR.n, 2), dtype=np.int64), 1.0, 0)
    assert ei.value.code == ERR_INVALID


# ---------------------------------------------------------------------------------------------
# 6. wire
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_hint_through_the_wire(gpu, cpuref):
    m, qs = 2048, [1017857, 1032193]
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(5)
    s_crt = _small_key(cpuref, P, rng)
    hint = pq.ksQuadCircHint(s_crt, 1.0, 256, key=bytes(range(32)), ctr=0)
    nL = hint.shape[0]
    dec = pq.lInv(pq.crtInv(hint.reshape(nL * 2, P.n, 2))).reshape(hint.shape)
    m2, qs2, xs = gpu.kshint_read(gpu.kshint_write(m, qs, dec))
    assert (m2, qs2) == (m, qs)
    assert np.array_equal(xs.reshape(hint.shape), dec)
    assert np.array_equal(pq.crt(pq.l(xs.reshape(nL * 2, P.n, 2))).reshape(hint.shape), hint)
