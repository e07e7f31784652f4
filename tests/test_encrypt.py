"""SymmSHE encrypt and errorRounded on the GPU (lolhip_encrypt_batch, lolhip_error_rounded_batch).

The reference is the numpy restatement of tests/enc_ref.py (ChaCha20, the stream layout, Box-Muller, the uniform
residues, coset rounding), with oracle.floatref.gaussian_dec for the decoding-basis map and the CPU oracle for L, lInv,
embedPow and the transforms.

    bit-exact              c1 exactly; errorTerm (ct) = the restated e except within 1e-9 of a rounding tie (libm
                           ulps, the map's 1e-12 contract); e = rep (mod p); out_pow = crtInv (out_crt)
    round trip             decrypt (encrypt pt) = pt, both output bases, m != m' included
    SymmSHE properties     device-made key (errorRounded) and ciphertexts through oracle/she_model.py on the GPU plan:
                           Dec (Enc a * Enc b) = a b, Dec (keySwitchQuadCirc) = Dec
    determinism            a batch split in two at ctr, ctr + 5 is the same batch; on a side stream; another key
    distribution           errorRounded mean / variance; chi-square of c1 at q ~ 2^20 and 2^61
    errors                 every reachable status, decided before any launch: the output stays untouched
"""
import numpy as np
import pytest

import enc_ref as er
from oracle import floatref as fr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params


def _params(m, qs):
    """oracle Params, also for a modulus without a CRT basis (prime ops only)"""
    try:
        return Params(lm.factor_pps(m), qs)
    except ValueError:
        P = Params.__new__(Params)
        P.pps = lm.factor_pps(m)
        P.qs, P.T, P.m, P.n = list(qs), len(qs), m, lm.totient_pps(P.pps)
        return P


def _moduli(m, bits, T):
    g = lm.good_qs(m, 2 ** (bits - 1))
    return [next(g) for _ in range(T)]


def _two_power(m):
    return all(p == 2 for p, _ in lm.factor_pps(m))


def _small_key(cpuref, m, qs, rng):
    """a secret key with decoding-basis coefficients in {-1, 0, 1}, CRT basis [n][T] (the CPU oracle)"""
    P = Params(lm.factor_pps(m), qs)
    z = rng.integers(-1, 2, size=(1, P.n)).astype(object)
    res = np.stack([(z % q).astype(np.int64) for q in qs], axis=-1)
    return np.ascontiguousarray(cpuref.crt(P, cpuref.l(P, res)).reshape(P.n, len(qs)))


def _rep(cpuref, m, m2, p, pt):
    """centred decoding-basis coefficients of embed pt over p, [B][n']"""
    Pm2 = _params(m2, [p])
    x = (pt % p)[..., None]
    if m != m2:
        x = cpuref.embed_pow(_params(m, [p]), Pm2, x)
    return er.centred(cpuref.linv(Pm2, x).reshape(pt.shape[0], Pm2.n), p)


def _restated_e(m2, p, svar, key, ctr, B, rep):
    pps2 = lm.factor_pps(m2)
    n = lm.totient_pps(pps2)
    g = er.gaussians(key, er.DOM_ENC_GAUSS, ctr, B, n, er.sigma(pps2, svar * (float(p) * float(p))))
    if not _two_power(m2):
        g = fr.gaussian_dec(pps2, g).reshape(B, n)
    return er.round_coset(g, rep, p)


# (m, m', p, moduli): 2^11; the sheBenches shapes; config 3's ring; 45; the key-switch index 14400; 15015
SHAPES = [(2048, 2048, 16, ("bits", 30, 1)), (16, 1024, 8, [1017857]), (16, 2048, 16, [1017857]),
          (2 ** 15, 2 ** 15, 65537, ("bits", 59, 4)), (45, 45, 7, ("bits", 30, 3)), (14400, 14400, 11, ("bits", 30, 2)),
          (15015, 15015, 4, ("bits", 30, 4))]


def _setup(gpu, m, m2, p, mods):
    qs = _moduli(m2, mods[1], mods[2]) if isinstance(mods, tuple) else list(mods)
    pq, pp = gpu.Plan.for_index(m2, qs), gpu.Plan.for_index(m2, [p])
    x_p = None if m == m2 else gpu.Ext(gpu.Plan.for_index(m, [p]), pp)
    n_m = pp.n if x_p is None else x_p.lo.n
    return qs, pq, pp, x_p, n_m


# ---------------------------------------------------------------------------------------------
# 1 + 2. bit-exact against the restatement, and the round trip
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,m2,p,mods", SHAPES)
def test_encrypt_matches_restatement_and_decrypts(gpu, cpuref, m, m2, p, mods):
    qs, pq, pp, x_p, n_m = _setup(gpu, m, m2, p, mods)
    n, T = pq.n, len(qs)
    rng = np.random.default_rng(m2 + p)
    B, svar, ctr = 3, 1.5, 1000 + m2
    key = rng.bytes(32)
    pt = rng.integers(-p + 1, p, size=(B, n_m), dtype=np.int64)
    s_crt = _small_key(cpuref, m2, qs, rng)
    out_crt = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, ext=x_p, out_crt=True)
    out_pow = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, ext=x_p)
    assert out_crt.shape == out_pow.shape == (2, B, n, T)
    # c1: exact
    assert np.array_equal(out_crt[1], er.uniform_crt(key, ctr, B, n, qs))
    # the two routes: the same integers up to crtInv
    P = Params(lm.factor_pps(m2), qs)
    for i in range(2):
        assert np.array_equal(out_pow[i], cpuref.crtinv(P, out_crt[i]).reshape(B, n, T)), i
    # e through the existing errorTerm, both bases
    rep = _rep(cpuref, m, m2, p, pt)
    e_want, near = _restated_e(m2, p, svar, key, ctr, B, rep)
    e_pow = pq.errorTerm(out_pow, s_crt, p)
    e_crt = pq.errorTerm(out_crt, s_crt, p, cs_crt=True)
    assert np.array_equal(e_pow, e_crt)
    bad = e_pow != e_want
    assert bad.sum() <= 4 and near[bad].all(), (int(bad.sum()), int(near.sum()))
    assert ((e_pow - rep) % p == 0).all()                                  # e in the coset rep + pR'
    assert np.abs(e_pow).max() < 2 ** 52
    # the round trip
    want = pt % p
    assert np.array_equal(pq.decrypt(out_pow, s_crt, pp, ext=x_p), want)
    assert np.array_equal(pq.decrypt(out_crt, s_crt, pp, ext=x_p, cs_crt=True), want)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2048, 45, 14400])
def test_error_rounded_matches_restatement(gpu, m):
    g = lm.good_qs(m, 2 ** 29)
    pq = gpu.Plan.for_index(m, [next(g)])
    pps = lm.factor_pps(m)
    B, svar, ctr, key = 4, 3.0, 7, bytes(range(1, 33))
    z = pq.errorRounded(svar, B=B, key=key, ctr=ctr).cpu().numpy()
    x = er.gaussians(key, er.DOM_ERR_ROUNDED, ctr, B, pq.n, er.sigma(pps, svar))
    if not _two_power(m):
        x = fr.gaussian_dec(pps, x).reshape(B, pq.n)
    want, near = er.round_coset(x, np.zeros_like(z), 1)
    bad = z != want
    assert bad.sum() <= 4 and near[bad].all()


# ---------------------------------------------------------------------------------------------
# 3. SymmSHE properties with a device-made key and device-made ciphertexts
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,p,lower", [(64, 257, 2 ** 29), (45, 181, 2 ** 30)])
def test_she_properties_with_device_key_and_ciphertexts(gpu, cpuref, m, p, lower):
    pps = lm.factor_pps(m)
    g = lm.good_qs(m, lower)
    qs = [next(g), next(g)]
    rng = np.random.default_rng(m + p)
    pq, pp = gpu.Plan(pps, qs), gpu.Plan(pps, [p])
    she = sm.SHE(pq, pp, qs, p, rng)
    z = pq.errorRounded(0.5, B=1, key=bytes(32), ctr=0).cpu().numpy()    # genSK
    assert np.abs(z).max() > 0
    she.s = np.ascontiguousarray(pq.l(she.reduce(z)))
    she.s_crt = np.ascontiguousarray(pq.crt(she.s))
    B, key = 3, bytes(range(32, 64))
    a = rng.integers(0, p, size=(B, pq.n), dtype=np.int64)
    b = rng.integers(0, p, size=(B, pq.n), dtype=np.int64)
    ca = pq.encrypt(a, she.s_crt[0], pp, 0.5, key=key, ctr=0)
    cb = pq.encrypt(b, she.s_crt[0], pp, 0.5, key=key, ctr=B)
    cta = {"enc": "LSD", "k": 0, "l": 1, "c": [ca[0], ca[1]]}
    ctb = {"enc": "LSD", "k": 0, "l": 1, "c": [cb[0], cb[1]]}
    assert np.array_equal(she.decrypt(cta), a)
    assert np.array_equal(she.decrypt(ctb), b)
    prod_ = she.mul(cta, ctb)
    want = cpuref.polymul(Params(pps, [p]), a[..., None], b[..., None]).reshape(a.shape)
    assert np.array_equal(she.decrypt(prod_), want), "Dec (Enc a * Enc b)"
    for base in (0, 256):
        lin = she.key_switch_quad(she.ks_quad_hint(base), base, prod_)
        assert np.array_equal(she.decrypt(lin), want), base


# ---------------------------------------------------------------------------------------------
# 4. determinism and sharding
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", [2048, 45])
def test_encrypt_is_a_function_of_key_and_position(gpu, cpuref, m):
    import torch
    g = lm.good_qs(m, 2 ** 29)
    qs = [next(g), next(g)]
    p = 5
    pq, pp = gpu.Plan.for_index(m, qs), gpu.Plan.for_index(m, [p])
    rng = np.random.default_rng(m)
    pt = torch.from_numpy(rng.integers(0, p, size=(8, pq.n), dtype=np.int64)).cuda()
    s_crt = torch.from_numpy(_small_key(cpuref, m, qs, rng)).cuda()
    key, c = bytes(range(7, 39)), 2 ** 32 - 3                               # ctr + b crosses into the high nonce word
    for out_crt in (False, True):
        whole = pq.encrypt(pt, s_crt, pp, 2.0, key=key, ctr=c, out_crt=out_crt)
        parts = torch.cat([pq.encrypt(pt[:5].contiguous(), s_crt, pp, 2.0, key=key, ctr=c, out_crt=out_crt),
                           pq.encrypt(pt[5:].contiguous(), s_crt, pp, 2.0, key=key, ctr=c + 5, out_crt=out_crt)], dim=1)
        assert torch.equal(whole, parts)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = pq.encrypt(pt, s_crt, pp, 2.0, key=key, ctr=c, out_crt=out_crt, stream=side.cuda_stream)
            z_side = pq.errorRounded(2.0, B=8, key=key, ctr=c, stream=side.cuda_stream)
        side.synchronize()
        assert torch.equal(whole, on_side)
        z = pq.errorRounded(2.0, B=8, key=key, ctr=c)
        assert torch.equal(z, z_side)
        assert torch.equal(z, torch.cat([pq.errorRounded(2.0, B=3, key=key, ctr=c),
                                         pq.errorRounded(2.0, B=5, key=key, ctr=c + 3)]))
        other = pq.encrypt(pt, s_crt, pp, 2.0, key=bytes(range(8, 40)), ctr=c, out_crt=True)
        if out_crt:
            same = (other[1] == whole[1]).double().mean().item()
            assert same < 1e-4, same
    # key = None draws a fresh key: two calls differ
    a = pq.encrypt(pt, s_crt, pp, 2.0, out_crt=True)
    b = pq.encrypt(pt, s_crt, pp, 2.0, out_crt=True)
    assert not torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------
# 5. distribution
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_rounded_mean_and_variance(gpu):
    m, svar, B = 2048, 1.0, 1000
    pq = gpu.Plan.for_index(m, [next(lm.good_qs(m, 2 ** 29))])
    z = pq.errorRounded(svar, B=B, key=bytes([3]) * 32, ctr=11).cpu().numpy().astype(np.float64).ravel()
    var_want = svar * pq.n / (2 * np.pi) + 1 / 12
    assert abs(z.mean()) < 5 * np.sqrt(var_want / z.size), z.mean()
    assert abs(z.var() / var_want - 1) < 0.01, (z.var(), var_want)


@pytest.mark.gpu
def test_uniform_c1_chi_square(gpu, cpuref):
    m = 2048
    qs = [next(lm.good_qs(m, 2 ** 20)), next(lm.good_qs(m, 2 ** 61))]
    assert qs[1] < 2 ** 62
    pq, pp = gpu.Plan.for_index(m, qs), gpu.Plan.for_index(m, [2])
    B = 64
    pt = np.zeros((B, pq.n), dtype=np.int64)
    s_crt = _small_key(cpuref, m, qs, np.random.default_rng(1))
    c1 = pq.encrypt(pt, s_crt, pp, 1.0, key=bytes([9]) * 32, ctr=0, out_crt=True)[1]
    for t, q in enumerate(qs):
        x = [int(v) for v in c1[..., t].ravel()]
        edges = [-(-k * q // 16) for k in range(17)]                       # ceil(k q / 16)
        counts = np.bincount(np.searchsorted(np.array(edges[1:-1], dtype=object), np.array(x, dtype=object), side="right")
                             .astype(np.int64), minlength=16)
        expect = np.array([(edges[k + 1] - edges[k]) * len(x) / q for k in range(16)])
        chi2 = float(((counts - expect) ** 2 / expect).sum())
        assert chi2 < 60, (q, chi2)                                        # 15 degrees of freedom: p ~ 1e-7


# ---------------------------------------------------------------------------------------------
# 6. errors: decided on the host, before any launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_encrypt_errors_leave_output_untouched(gpu):
    import torch
    L = gpu.lib()
    SENT = 0x5A5A5A5A
    B = 2
    key = bytes(32)

    def run(pq, pp, x_p=None, svar=1.0, b=B, n_m=None):
        n_m = n_m or pp.n
        pt = torch.zeros((max(b, 1), n_m), dtype=torch.int64, device="cuda")
        s_crt = torch.zeros((pq.n, pq.T), dtype=torch.int64, device="cuda")
        wl = L.lolhip_encrypt_work_len(pq._h, max(b, 1))
        work = torch.zeros((max(wl, 1),), dtype=torch.int64, device="cuda")
        out = torch.full((2, max(b, 1), pq.n, pq.T), SENT, dtype=torch.int64, device="cuda")
        rcs = []
        for out_crt in (0, 1):
            rcs.append(L.lolhip_encrypt_batch(pq._h, pp._h, None if x_p is None else x_p._h, None, pt.data_ptr(),
                                              s_crt.data_ptr(), svar, key, 5, out_crt, out.data_ptr(), work.data_ptr(), b))
        torch.cuda.synchronize()
        assert rcs[0] == rcs[1]
        return rcs[0], bool((out == SENT).all())

    def run_er(p, svar=1.0, b=B):
        out = torch.full((max(b, 1), p.n), SENT, dtype=torch.int64, device="cuda")
        rc = L.lolhip_error_rounded_batch(p._h, None, svar, key, 0, out.data_ptr(), None, b)
        torch.cuda.synchronize()
        return rc, bool((out == SENT).all())

    ERR_INVALID, ERR_NO_CRT = -1, -3
    qs = [1017857, 1032193]
    pq = gpu.Plan.for_index(2048, qs)
    pp = gpu.Plan.for_index(2048, [16])
    # valid calls write
    assert run(pq, pp) == (0, False)
    assert run_er(pq) == (0, False)
    # svar <= 0 or not finite; B < 0
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        assert run(pq, pp, svar=sv) == (ERR_INVALID, True), sv
        assert run_er(pq, svar=sv) == (ERR_INVALID, True), sv
    assert run(pq, pp, b=-1) == (ERR_INVALID, True)
    assert run_er(pq, b=-1) == (ERR_INVALID, True)
    # pp of another index / of two moduli
    assert run(pq, gpu.Plan.for_index(1024, [16])) == (ERR_INVALID, True)
    assert run(pq, gpu.Plan.for_index(2048, [16, 17])) == (ERR_INVALID, True)
    # x_p that does not end in pp
    pm = gpu.Plan.for_index(16, [16])
    assert run(pq, pp, gpu.Ext(gpu.Plan.for_index(16, [8]), gpu.Plan.for_index(2048, [8])), n_m=pm.n) == (ERR_INVALID, True)
    assert run(pq, pp, gpu.Ext(pm, gpu.Plan.for_index(1024, [16])), n_m=pm.n) == (ERR_INVALID, True)
    assert run(pq, pp, gpu.Ext(pm, pp), n_m=pm.n) == (0, False)
    # T > 16
    g = lm.good_qs(16, 2 ** 20)
    p17 = gpu.Plan.for_index(16, [next(g) for _ in range(17)])
    assert run(p17, gpu.Plan.for_index(16, [16])) == (ERR_INVALID, True)
    # indices beyond the sampler's limits: a prime > 13, n' > 8192 off the 2-powers, n' > 16384 for a 2-power
    for mm in (17, 3 * 2 ** 14, 2 ** 16):
        big = gpu.Plan.for_index(mm, [next(lm.good_qs(mm, 2 ** 29))])
        assert run(big, gpu.Plan.for_index(mm, [16])) == (ERR_INVALID, True), mm
        assert run_er(big) == (ERR_INVALID, True), mm
    # pq without a CRT basis
    no_crt = [q for q in range(1000003, 1001000, 2) if lm.is_prime(q) and (q - 1) % 2048][:2]
    pnc = gpu.Plan.for_index(2048, no_crt)
    assert not pnc.has_crt
    assert run(pnc, pp) == (ERR_NO_CRT, True)
    assert run_er(pnc) == (0, False)                                   # errorRounded needs the index only
    # the Python layer raises with the code (before it stages anything)
    with pytest.raises(gpu.LolHipError) as ei:
        pq.encrypt(np.zeros((1, pq.n), dtype=np.int64), np.zeros((pq.n, 2), dtype=np.int64), pp, -1.0)
    assert ei.value.code == ERR_INVALID
    # LOLHIP_ERR_MODULUS (p < 2) cannot be reached through a plan: plan creation already refuses a modulus below 2
