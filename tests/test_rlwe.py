"""gSqNormDec and batched RLWE / RLWR sampling and verification on the GPU (lol_amd.RLWE over include/lolhip.h).

The references are tests/golden/golden_norm.npz (the reference's own tensorNormSqR / tensorNormSqD) and the numpy /
Python-integer restatement of tests/rlwe_ref.py, with the CPU oracle for the transforms and oracle.floatref for the
Gaussian decoding-basis map.

    1 gSqNorm        int64 exact, doubles within relative 1e-12; the same bits twice and for a split batch
    2 saturation     exact or INT64_MAX, never wrapped.  The all-(2^31 - 1) sample at m = 8 has the true value
                     4 (2^31 - 1)^2 = 2^64 - 2^34 + 4, which does not fit int64: the expected value from Python
                     integers is INT64_MAX there; the largest such sample that fits is n = 2 (m = 4), checked exact
    3 samplers       a, secret: the restated streams exactly; Disc e = the restated rounded Gaussian (at most 4
                     coefficients off, each within 1e-9 of a tie), b = a s + crt (l (reduce e)) exactly; Cont
                     |e - g| <= 1e-12 |g| + q 2^-52, b in [0, q); split batches
    4 Cont           hand-made b around known x: bit-identical to the restatement
    5 RLWR           roundedProd bit-exact incl. exact multiples of q and l = -floor(q/2); mismatch counts
    6 verification   valid with the generating secret, invalid with another; norm-only = norm with e
    7 status codes   decided on the host, outputs untouched
"""
import os

import numpy as np
import pytest

import enc_ref as er
import rlwe_ref as rr
from oracle import lolmath as lm
from oracle.oracle import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [8, 12, 45, 81, 1456]
LARGE = [11648, 14400, 2 ** 14, 2 ** 15]
SVARS = (0.28125, 7.8125e-3, 4.0)
INT64_MAX, INT64_MIN = rr.INT64_MAX, rr.INT64_MIN


@pytest.fixture(scope="module")
def golden_norm():
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_norm.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _prime(m, bits):
    """the first good prime of at least `bits` bits"""
    return next(lm.good_qs(m, 2 ** (bits - 1)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _as_dec(cpuref, m, qs, a, s):
    """decoding-basis residues of a s: [B][n][T] in [0, q_t)"""
    P = Params(lm.factor_pps(m), qs)
    qv = np.array(qs, dtype=object)
    prod = ((np.asarray(a).astype(object) * np.asarray(s).astype(object)[None]) % qv).astype(np.int64)
    return cpuref.linv(P, cpuref.crtinv(P, prod)).reshape(prod.shape)


def _crt_of_dec(cpuref, m, qs, x):
    """x [B][n] integers (decoding basis) -> residues in the CRT basis [B][n][T]"""
    P = Params(lm.factor_pps(m), qs)
    res = np.stack([(np.asarray(x).astype(object) % q).astype(np.int64) for q in qs], axis=-1)
    return cpuref.crt(P, cpuref.l(P, res)).reshape(res.shape)


# ---------------------------------------------------------------------------------------------
# 1. gSqNorm
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", SMALL + LARGE + [23])
def test_gsqnorm_matches_golden_and_restatement(gpu, golden_norm, m):
    pps = rr.factor_pps(m)
    r = gpu.RLWE(gpu.Plan.for_index(m, [_prime(m, 30)]))
    ei, ed = golden_norm[f"e_i_{m}"].astype(np.int64), golden_norm[f"e_d_{m}"].astype(np.float64)
    for B in sorted({1, ei.shape[0]}):
        gi = r.gSqNorm(ei[:B])
        assert gi.dtype == np.int64 and np.array_equal(gi, golden_norm[f"n_i_{m}"][:B])
        assert np.array_equal(gi, rr.gsqnorm_sat(pps, ei[:B]))
        gd = r.gSqNorm(ed[:B])
        for want in (golden_norm[f"n_d_{m}"][:B], rr.gsqnorm_f64(pps, ed[:B])):
            assert (np.abs(gd - want) <= 1e-12 * np.abs(want)).all(), (gd, want)
        assert np.array_equal(_bits(gd), _bits(r.gSqNorm(ed[:B])))                 # run to run
    # B = 5 in one call = B = 2, then B = 3, bit for bit; against the restatement as well
    rng = np.random.default_rng(m)
    x = rng.normal(size=(5, r.plan.n)) * 1e3
    whole = r.gSqNorm(x)
    assert np.array_equal(_bits(whole), _bits(np.concatenate([r.gSqNorm(x[:2]), r.gSqNorm(x[2:])])))
    want = rr.gsqnorm_f64(pps, x)
    assert (np.abs(whole - want) <= 1e-12 * want).all()
    xi = rng.integers(-2 ** 31, 2 ** 31, size=(5, r.plan.n), dtype=np.int64)
    assert np.array_equal(r.gSqNorm(xi), rr.gsqnorm_sat(pps, xi))


@pytest.mark.gpu
def test_gsqnorm_more_samples_than_one_grid_pass(gpu):
    """m = 8: 64 samples per workgroup, 1094 tiles over a grid of 1024, and a tail tile of 49 samples"""
    B, n = 70001, 4
    r = gpu.RLWE(gpu.Plan.for_index(8, [_prime(8, 30)]))
    rng = np.random.default_rng(70001)
    xi = rng.integers(-2 ** 20, 2 ** 20, size=(B, n), dtype=np.int64)
    assert np.array_equal(r.gSqNorm(xi), (xi * xi).sum(axis=1))
    xd = rng.normal(size=(B, n))
    got, want = r.gSqNorm(xd), rr.gsqnorm_f64([(2, 3)], xd)
    assert (np.abs(got - want) <= 1e-12 * want).all()
    assert np.array_equal(_bits(got[60000:]), _bits(r.gSqNorm(xd[60000:])))       # independent of B and of the tile


# ---------------------------------------------------------------------------------------------
# 2. saturation
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", [12, 2 ** 14])
def test_gsqnorm_is_exact_or_saturated_never_wrapped(gpu, m):
    pps = rr.factor_pps(m)
    r = gpu.RLWE(gpu.Plan.for_index(m, [_prime(m, 30)]))
    n = r.plan.n
    rng = np.random.default_rng(m)
    rows = []
    for v in (2 ** 32, -2 ** 32, INT64_MIN, 2 ** 32 - 1, 3037000499, -3037000499, 3037000500, INT64_MAX):
        e = np.zeros(n, dtype=np.int64)
        e[int(rng.integers(0, n))] = v
        rows.append(e)
    noisy = rng.integers(-1000, 1000, size=n, dtype=np.int64)
    noisy[n // 2] = INT64_MIN
    rows += [noisy, np.full(n, 2 ** 31 - 1, dtype=np.int64), np.full(n, -(2 ** 31), dtype=np.int64)]
    e = np.stack(rows)
    want = rr.gsqnorm_sat(pps, e)
    got = r.gSqNorm(e)
    assert np.array_equal(got, want), (got, want)
    assert (want[:3] == INT64_MAX).all() and want[8] == INT64_MAX and want[9] == INT64_MAX
    if m == 2 ** 14:
        assert want[4] == 3037000499 ** 2 and want[6] == INT64_MAX                # either side of sqrt(2^63)


@pytest.mark.gpu
def test_gsqnorm_all_large_coefficients_at_small_indices(gpu):
    c = 2 ** 31 - 1
    for m, n in ((8, 4), (4, 2)):
        r = gpu.RLWE(gpu.Plan.for_index(m, [_prime(m, 30)]))
        e = np.full((1, n), c, dtype=np.int64)
        want = rr.gsqnorm_sat(rr.factor_pps(m), e)
        assert want[0] == min(n * c * c, INT64_MAX)
        assert np.array_equal(r.gSqNorm(e), want), m
    assert 2 * c * c < 2 ** 63 <= 4 * c * c                                       # m = 4 is exact, m = 8 saturates


# ---------------------------------------------------------------------------------------------
# 3. samplers
# ---------------------------------------------------------------------------------------------
def _disc_moduli(m):
    g = lm.good_qs(m, 2 ** 29)
    return [[_prime(m, 28)], [_prime(m, 60)], [_prime(m, 30), _prime(m, 61)], [next(g), next(g), next(g)]]


@pytest.mark.gpu
@pytest.mark.parametrize("m", SMALL + [2 ** 14])
@pytest.mark.parametrize("which", range(4))
def test_sample_disc_matches_restatement(gpu, cpuref, m, which):
    import torch
    qs = _disc_moduli(m)[which]
    assert all(q < 2 ** 62 for q in qs)
    pps = rr.factor_pps(m)
    r = gpu.RLWE(gpu.Plan.for_index(m, qs))
    n, T = r.plan.n, len(qs)
    B, svar, ctr = 3, SVARS[(which + m) % 3], 2 ** 32 - 2 + which               # the item number carries into the high word
    key = bytes(range(which, which + 32))
    s = r.secret(key=key, ctr=77)
    assert np.array_equal(s.cpu().numpy(), rr.uniform(key, rr.DOM_RLWE_SECRET, 77, 1, n, qs)[0])
    a, b = r.sampleDisc(s, B, svar, key=key, ctr=ctr)
    assert a.shape == b.shape == (B, n, T)
    a_h, b_h, s_h = a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(a_h, rr.uniform(key, rr.DOM_RLWE_UNIFORM, ctr, B, n, qs))
    e = r.errorTermDisc(s, a, b).cpu().numpy()
    want, near = er.round_coset(rr.gaussian_dec(pps, key, ctr, B, svar), np.zeros((B, n), dtype=np.int64), 1)
    bad = e != want
    assert bad.sum() <= 4 and near[bad].all(), (int(bad.sum()), int(near.sum()))
    qv = np.array(qs, dtype=object)
    b_want = (a_h.astype(object) * s_h.astype(object)[None] + _crt_of_dec(cpuref, m, qs, e).astype(object)) % qv
    assert np.array_equal(b_h, b_want.astype(np.int64))
    # the batch split at ctr, ctr + 2
    a5, b5 = r.sampleDisc(s, 5, svar, key=key, ctr=ctr)
    a2, b2 = r.sampleDisc(s, 2, svar, key=key, ctr=ctr)
    a3, b3 = r.sampleDisc(s, 3, svar, key=key, ctr=ctr + 2)
    assert torch.equal(a5, torch.cat([a2, a3])) and torch.equal(b5, torch.cat([b2, b3]))
    assert torch.equal(a5[:3], a) and torch.equal(b5[:3], b)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [8, 12, 45, 1456, 2 ** 14])
@pytest.mark.parametrize("bits", [28, 60])
def test_sample_cont_matches_restatement(gpu, cpuref, m, bits):
    import torch
    q = _prime(m, bits)
    pps = rr.factor_pps(m)
    r = gpu.RLWE(gpu.Plan.for_index(m, [q]))
    n = r.plan.n
    B, svar, ctr, key = 3, SVARS[m % 3], 1000 + m, bytes(range(5, 37))
    s = r.secret(key=key, ctr=3)
    a, b = r.sampleCont(s, B, svar, key=key, ctr=ctr)
    assert a.shape == (B, n, 1) and b.shape == (B, n) and b.dtype == torch.float64
    a_h, b_h = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a_h, rr.uniform(key, rr.DOM_RLWE_UNIFORM, ctr, B, n, [q]))
    assert (b_h >= 0).all() and (b_h < float(q)).all()
    a5, b5 = r.sampleCont(s, 5, svar, key=key, ctr=ctr)
    a2, b2 = r.sampleCont(s, 2, svar, key=key, ctr=ctr)
    a3, b3 = r.sampleCont(s, 3, svar, key=key, ctr=ctr + 2)
    assert torch.equal(a5, torch.cat([a2, a3])) and torch.equal(b5.view(torch.int64), torch.cat([b2, b3]).view(torch.int64))
    if bits == 28:
        g = rr.gaussian_dec(pps, key, ctr, B, svar)
        e = r.errorTermCont(s, a, b).cpu().numpy()
        assert (np.abs(e - g) <= 1e-12 * np.abs(g) + float(q) * 2.0 ** -52).all(), float(np.abs(e - g).max())
        # and b itself is the restated function of (x, g) up to the same bound, taken mod q
        x = _as_dec(cpuref, m, [q], a_h, s.cpu().numpy())[..., 0]
        d = np.abs(b_h - rr.cont_sample(x, g, q))
        d = np.minimum(d, float(q) - d)
        assert (d <= 1e-12 * np.abs(g) + float(q) * 2.0 ** -52).all()


# ---------------------------------------------------------------------------------------------
# 4. the K/(qR) arithmetic on its own
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", [8, 45])
def test_error_term_cont_is_bit_identical_on_hand_made_b(gpu, cpuref, m):
    q = _prime(m, 28)
    qd = float(q)
    r = gpu.RLWE(gpu.Plan.for_index(m, [q]))
    n = r.plan.n
    rng = np.random.default_rng(m)
    B = 7
    a = rng.integers(0, q, size=(B, n, 1), dtype=np.int64)
    s = rng.integers(0, q, size=(n, 1), dtype=np.int64)
    x = _as_dec(cpuref, m, [q], a, s)[..., 0]
    xd = x.astype(np.float64)
    b = np.stack([np.zeros(n), np.full(n, np.nextafter(qd, 0.0)), xd[2], rr.rrq_reduce(xd[3] + 0.25, qd),
                  rr.rrq_reduce(xd[4] - 0.25, qd), rr.rrq_reduce(xd[5] + qd / 2, qd),
                  rr.rrq_reduce(xd[6] + rng.normal(size=n) * 3.0, qd)])
    assert (b >= 0).all() and (b < qd).all()
    e, nm = r.errorTermCont(s, a, b, norm=True)
    want = rr.cont_error(x, b, q)
    assert np.array_equal(_bits(e), _bits(want))
    assert (e[2] == 0).all() and (np.abs(e[3]) == 0.25).all()
    nw = rr.gsqnorm_f64(rr.factor_pps(m), want)
    assert (np.abs(nm - nw) <= 1e-12 * nw).all()
    assert np.array_equal(_bits(nm), _bits(r.errorGSqNormCont(s, a, b)))


# ---------------------------------------------------------------------------------------------
# 5. RLWR
# ---------------------------------------------------------------------------------------------
def _rlwr_cases(m):
    q30, q61 = _prime(m, 30), _prime(m, 61)
    return [(q30, 2), (q30, 2 ** 8), (q61, 2 ** 30), (q61, q61 - 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", SMALL + [2 ** 14])
@pytest.mark.parametrize("which", range(4))
def test_rounded_prod_and_check(gpu, cpuref, m, which):
    import torch
    q, p = _rlwr_cases(m)[which]
    assert 2 <= p < q < 2 ** 62
    r = gpu.RLWE(gpu.Plan.for_index(m, [q]))
    n = r.plan.n
    key = bytes(range(9, 41))
    s = r.secret(key=key, ctr=1)
    B = 3
    a, b = r.sampleRLWR(s, B, p, key=key, ctr=40)
    a_h, b_h, s_h = a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(a_h, rr.uniform(key, rr.DOM_RLWE_UNIFORM, 40, B, n, [q]))
    want = rr.rlwr_round(_as_dec(cpuref, m, [q], a_h, s_h)[..., 0], q, p)
    assert np.array_equal(b_h, want) and b_h.min() >= 0 and b_h.max() < p
    assert torch.equal(r.roundedProd(s, a, p), b)
    assert np.array_equal(r.mismatchRLWR(s, a, b, p).cpu().numpy(), np.zeros(B, dtype=np.int32))
    assert r.validRLWR(s, a, b, p).all()
    # k changed coefficients of one sample
    k = min(n, 5)
    idx = np.random.default_rng(m + which).choice(n, size=k, replace=False)
    b2 = b_h.copy()
    b2[1, idx] = (b2[1, idx] + 1) % p
    assert list(r.mismatchRLWR(s_h, a_h, b2, p)) == [0, k, 0]
    assert list(r.validRLWR(s_h, a_h, b2, p)) == [True, False, True]
    # constructed residues under the secret 1: exact multiples of q, l = -floor(q/2) and their neighbours
    h = q // 2
    l0 = (-h * pow(p, -1, q)) % q                                                # p l0 + h = 0 (mod q)
    special = [l0, (l0 + 1) % q, (l0 - 1) % q, q - h, q - h - 1, (q - h + 1) % q, 0, 1, q - 1, h]
    for v in special[:1]:
        lc = v if 2 * v < q else v - q
        assert (p * lc + h) % q == 0
    assert (q - h) - q == -h
    x = np.array([(special * n)[:n], (special[::-1] * n)[:n]], dtype=np.int64)
    ones = np.ones((n, 1), dtype=np.int64)
    a_c = _crt_of_dec(cpuref, m, [q], x)
    assert np.array_equal(_as_dec(cpuref, m, [q], a_c, ones)[..., 0], x)
    assert np.array_equal(r.roundedProd(ones, a_c, p), rr.rlwr_round(x, q, p))


# ---------------------------------------------------------------------------------------------
# 6. verification end to end (Verify.hs:346-366)
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("q,svar", [(769, 7.8125e-3), (3329, 3.125e-2)])
def test_instances_verify_with_their_secret_only(gpu, q, svar):
    import torch
    m, B = 256, 100
    pps = rr.factor_pps(m)
    r = gpu.RLWE(gpu.Plan.for_index(m, [q]))
    key = bytes(range(64, 96))
    s, other = r.secret(key=key, ctr=0), r.secret(key=key, ctr=1)
    assert not torch.equal(s, other)
    # discrete
    bound = gpu.RLWE.errorBound(m, svar, eps=2.0 ** -25, kind="disc")
    assert bound == rr.error_bound_disc(m, svar, 2.0 ** -25)
    a, b = r.sampleDisc(s, B, svar, key=key, ctr=10)
    assert r.validDisc(bound, s, a, b).all()
    assert not r.validDisc(bound, other, a, b).any()
    e, nm = r.errorTermDisc(s, a, b, norm=True)
    only = r.errorGSqNormDisc(s, a, b)
    assert torch.equal(nm, only)
    assert np.array_equal(only.cpu().numpy(), rr.gsqnorm_sat(pps, e.cpu().numpy()))
    wrong = r.errorGSqNormDisc(other, a, b).cpu().numpy()
    assert (wrong > bound).all() and np.array_equal(wrong, rr.gsqnorm_sat(pps, r.errorTermDisc(other, a, b).cpu().numpy()))
    # continuous
    cb = gpu.RLWE.errorBound(m, svar, eps=2.0 ** -25, kind="cont")
    a, b = r.sampleCont(s, B, svar, key=key, ctr=10 + B)
    assert r.validCont(cb, s, a, b).all()
    assert not r.validCont(cb, other, a, b).any()
    e, nm = r.errorTermCont(s, a, b, norm=True)
    only = r.errorGSqNormCont(s, a, b)
    assert torch.equal(nm.view(torch.int64), only.view(torch.int64))
    want = rr.gsqnorm_f64(pps, e.cpu().numpy())
    assert (np.abs(only.cpu().numpy() - want) <= 1e-12 * want).all()


# ---------------------------------------------------------------------------------------------
# 7. status codes on a device plan: decided on the host, outputs untouched
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rlwe_errors_leave_outputs_untouched(gpu):
    import torch
    L = gpu.lib()
    SENT = 0x5A5A5A5A
    ERR_INVALID, ERR_NO_CRT = -1, -3
    key = bytes(32)

    def bufs(pl, B):
        B = max(B, 1)
        wl = max(L.lolhip_rlwe_work_len(pl._h, 0, B), 2 * B * pl.n, 1)
        mk = lambda *sh: torch.full(sh, SENT, dtype=torch.int64, device="cuda")
        return mk(B, pl.n, pl.T), mk(B, pl.n, pl.T), mk(B, pl.n), mk(B), torch.zeros((wl,), dtype=torch.int64, device="cuda")

    def clean(*ts):
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in ts)

    def sample(pl, kind, p=4, svar=1.0, B=2):
        a, b, _, _, w = bufs(pl, B)
        s = torch.zeros((pl.n, pl.T), dtype=torch.int64, device="cuda")
        rc = L.lolhip_rlwe_sample_batch(pl._h, None, kind, p, s.data_ptr(), svar, key, 0, a.data_ptr(), b.data_ptr(),
                                        w.data_ptr(), B)
        return rc, clean(a, b)

    def error(pl, kind, B=2, e_null=False, n_null=False):
        a, b, e, nm, w = bufs(pl, B)
        a.zero_(); b.zero_()
        s = torch.zeros((pl.n, pl.T), dtype=torch.int64, device="cuda")
        rc = L.lolhip_rlwe_error_batch(pl._h, None, kind, a.data_ptr(), b.data_ptr(), s.data_ptr(),
                                       None if e_null else e.data_ptr(), None if n_null else nm.data_ptr(), w.data_ptr(), B)
        return rc, clean(e, nm)

    def rlwr(pl, p, B=2):
        a, _, out, _, w = bufs(pl, B)
        a.zero_()
        mm = torch.full((max(B, 1),), SENT, dtype=torch.int32, device="cuda")
        s = torch.zeros((pl.n, pl.T), dtype=torch.int64, device="cuda")
        rc1 = L.lolhip_rlwr_rounded_prod_batch(pl._h, p, None, a.data_ptr(), s.data_ptr(), out.data_ptr(), w.data_ptr(), B)
        rc2 = L.lolhip_rlwr_check_batch(pl._h, p, None, a.data_ptr(), a.data_ptr(), s.data_ptr(), mm.data_ptr(),
                                        w.data_ptr(), B)
        assert rc1 == rc2
        return rc1, clean(out, mm)

    def norm(pl, B=2):
        e = torch.zeros((max(B, 1), pl.n), dtype=torch.int64, device="cuda")
        o = torch.full((max(B, 1),), SENT, dtype=torch.int64, device="cuda")
        rcs = (L.lolhip_gsqnorm_batch(pl._h, None, e.data_ptr(), o.data_ptr(), B),
               L.lolhip_gsqnorm_f64_batch(pl._h, None, e.data_ptr(), o.data_ptr(), B))
        assert rcs[0] == rcs[1]
        return rcs[0], clean(o)

    p1 = gpu.Plan.for_index(64, [_prime(64, 30)])
    p2 = gpu.Plan.for_index(64, [_prime(64, 30), _prime(64, 31)])
    q = p1.qs[0]
    # valid calls write
    for kind in (0, 1, 2):
        assert sample(p1, kind) == (0, False), kind
    assert sample(p2, 0) == (0, False)
    assert error(p1, 0) == error(p1, 1) == error(p2, 0) == (0, False)
    assert rlwr(p1, 4) == (0, False) and norm(p1) == (0, False)
    # svar <= 0 or not finite (RLWR ignores it); B < 0; an unknown kind
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        assert sample(p1, 0, svar=sv) == sample(p1, 1, svar=sv) == (ERR_INVALID, True), sv
        assert sample(p1, 2, svar=sv) == (0, False)
    for kind in (0, 1, 2):
        assert sample(p1, kind, B=-1) == (ERR_INVALID, True)
    assert sample(p1, 3) == (ERR_INVALID, True) and sample(p1, -1) == (ERR_INVALID, True)
    assert error(p1, 2) == (ERR_INVALID, True) and error(p1, 0, B=-1) == (ERR_INVALID, True)
    assert error(p1, 0, e_null=True, n_null=True)[0] == ERR_INVALID
    assert rlwr(p1, 4, B=-1) == (ERR_INVALID, True) and norm(p1, B=-1) == (ERR_INVALID, True)
    # one modulus only for Cont and RLWR
    assert sample(p2, 1) == sample(p2, 2) == (ERR_INVALID, True)
    assert error(p2, 1) == (ERR_INVALID, True) and rlwr(p2, 4) == (ERR_INVALID, True)
    # 2 <= p < q
    for p in (q, q + 1, 1, 0, -5):
        assert sample(p1, 2, p=p) == (ERR_INVALID, True), p
        assert rlwr(p1, p) == (ERR_INVALID, True), p
    assert sample(p1, 2, p=q - 1) == (0, False) and rlwr(p1, q - 1) == (0, False)
    # T > 16
    g = lm.good_qs(16, 2 ** 20)
    p17 = gpu.Plan.for_index(16, [next(g) for _ in range(17)])
    assert sample(p17, 0) == (ERR_INVALID, True) and error(p17, 0) == (ERR_INVALID, True)
    # the sampler's index limits (a prime above 13); RLWR and the norm have none
    pb = gpu.Plan.for_index(17, [_prime(17, 30)])
    assert sample(pb, 0) == sample(pb, 1) == (ERR_INVALID, True)
    assert sample(pb, 2) == (0, False) and norm(pb) == (0, False) and error(pb, 0) == (0, False)
    # the norm's limit: n <= 16384
    assert norm(gpu.Plan.for_index(2 ** 16, [65537])) == (ERR_INVALID, True)
    # no CRT basis
    no_crt = [v for v in range(1000003, 1001000, 2) if lm.is_prime(v) and (v - 1) % 64][0]
    pn = gpu.Plan.for_index(64, [no_crt])
    assert not pn.has_crt
    for kind in (0, 1, 2):
        assert sample(pn, kind) == (ERR_NO_CRT, True), kind
    assert error(pn, 0) == error(pn, 1) == rlwr(pn, 4) == (ERR_NO_CRT, True)
    s_out = torch.full((pn.n, 1), SENT, dtype=torch.int64, device="cuda")
    assert L.lolhip_rlwe_secret(pn._h, None, key, 0, s_out.data_ptr()) == ERR_NO_CRT and clean(s_out)
    assert norm(pn) == (0, False)                                          # the norm needs the index only
    # the Python layer raises with the code before it stages anything
    with pytest.raises(gpu.LolHipError) as ei:
        gpu.RLWE(p1).sampleDisc(np.zeros((p1.n, 1), dtype=np.int64), 2, -1.0)
    assert ei.value.code == ERR_INVALID
