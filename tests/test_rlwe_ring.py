"""Batched RLWE / RLWR instances over one modulus without a CRT basis on the GPU (lol_amd.RingRLWE over
lolhip_rlwe_ring_*, include/lolhip.h), against the restatement of tests/rlwe_ring_ref.py.

    1 RLWR           a = the restated stream, b bit-exact, split batches, mismatch counts, boundary residues under the
                     secret 1
    2 Disc           b = (a s + l(e)) mod q exactly with e from errorTermDisc; e = the restated rounded Gaussian (at most
                     4 coefficients off, each within 1e-9 of a tie); e bit-identical to the plan route's e over a CRT prime
    3 Cont           b in [0, q), split batches, |e - g| <= 1e-12 |g| + q 2^-52; hand-made b bit-identical
    4 routes         the fused tails and the general composition give the same bits, each proven to have run
    5 conventions    over a CRT prime the ring route and the plan route verify each other's samples
    6 verification   challenge lines: valid under their own secret, invalid under another
    7 status codes   decided on the host, outputs untouched; a side stream; numpy and CUDA inputs

B = 3 throughout.  Shapes (m, q, p): K = 1, 2 and 3 NTT primes, 2-power and other indices, odd and even n / 8 tails."""
import math

import numpy as np
import pytest

import enc_ref as er
import rlwe_ref as rr
import rlwe_ring_ref as rg

pytestmark = pytest.mark.gpu

SHAPES = [(8, 16, 2), (32, 32, 2), (27, 81, 3), (12, 105, 7), (45, 900, 2),              # K = 1
          (16, 2 ** 40, 2 ** 8), (9, 3 ** 37, 3),                                         # K = 2
          (16, 2 ** 61, 2 ** 30), (45, 2 ** 61 - 1, 2),                                   # K = 3
          (2 ** 14, 2 ** 17, 2)]                                                          # one full-size
KS = {16: 1, 32: 1, 81: 1, 105: 1, 900: 1, 2 ** 40: 2, 3 ** 37: 2, 2 ** 61: 3, 2 ** 61 - 1: 3, 2 ** 17: 1}
B = 3
KEY = bytes(range(3, 35))
S_CTR = 2 ** 32 - 1                     # the secret's item: the low nonce word is all ones
INVALID = -1


def _svar(q):
    """the challenge list's smallest variance at the two smallest moduli; wider where q leaves room"""
    return 7.8125e-3 if q <= 32 else 0.28125 if q < 2 ** 20 else 4.0


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _h(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


_CTX = {}


class Ctx:
    """one (m, q): the handles and a secret drawn on the device, shared by the tests of that shape"""

    def __init__(self, gpu, m, q):
        self.m, self.q, self.pps = m, q, rr.factor_pps(m)
        self.plan = gpu.Plan.for_index(m, [q])
        self.r = gpu.RingRLWE(self.plan)
        self.n = self.plan.n
        self.s, self.shat = self.r.secret(key=KEY, ctr=S_CTR)
        self.s_h = _h(self.s)


def ctx(gpu, m, q):
    if (m, q) not in _CTX:
        _CTX[(m, q)] = Ctx(gpu, m, q)
    return _CTX[(m, q)]


@pytest.fixture
def info(monkeypatch, capfd):
    """route lines of the calls made since the last read: [(entry, kind, route, K)]"""
    monkeypatch.setenv("LOLHIP_RLWE_RING_INFO", "1")

    def read():
        out = []
        for ln in capfd.readouterr().err.splitlines():
            if ln.startswith("rlwe_ring: "):
                f = ln.replace(",", "").split()
                out.append((f[1], int(f[3]), f[5], int(f[7])))
        return out
    return read


# ---------------------------------------------------------------------------------------------
# 1. RLWR
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,q,p", SHAPES)
def test_rlwr_matches_restatement(gpu, m, q, p):
    import torch
    c = ctx(gpu, m, q)
    r, n = c.r, c.n
    assert r.K == KS[q] == len(rg.rm.moduli(m, [q]))
    assert c.s.shape == (n,) and c.shat.shape == (n, r.K)
    assert np.array_equal(c.s_h, rg.uniform(KEY, rr.DOM_RLWE_SECRET, S_CTR, 1, n, q)[0])
    assert torch.equal(r.prepare(c.s), c.shat)
    ctr = 2 ** 32 - 2                                            # the item number carries into the high word
    a, b = r.sampleRLWR(c.shat, B, p, key=KEY, ctr=ctr)
    assert a.shape == b.shape == (B, n)
    a_h, b_h = _h(a), _h(b)
    assert np.array_equal(a_h, rg.uniform(KEY, rr.DOM_RLWE_UNIFORM, ctr, B, n, q))
    assert np.array_equal(b_h, rg.rlwr_b(m, q, p, a_h, c.s_h)) and b_h.min() >= 0 and b_h.max() < p
    a5, b5 = r.sampleRLWR(c.shat, 5, p, key=KEY, ctr=ctr)
    a2, b2 = r.sampleRLWR(c.shat, 2, p, key=KEY, ctr=ctr)
    a3, b3 = r.sampleRLWR(c.shat, 3, p, key=KEY, ctr=ctr + 2)
    assert torch.equal(a5, torch.cat([a2, a3])) and torch.equal(b5, torch.cat([b2, b3]))
    assert torch.equal(a5[:3], a) and torch.equal(b5[:3], b)
    assert torch.equal(r.roundedProd(c.shat, a, p), b)
    assert list(_h(r.mismatchRLWR(c.shat, a, b, p))) == [0, 0, 0] and r.validRLWR(c.shat, a, b, p).all()
    k = min(n, 5)
    idx = np.random.default_rng(m).choice(n, size=k, replace=False)
    bad = b_h.copy()
    bad[1, idx] = (bad[1, idx] + 1) % p
    assert list(r.mismatchRLWR(_h(c.shat), a_h, bad, p)) == [0, k, 0]
    assert list(r.validRLWR(_h(c.shat), a_h, bad, p)) == [True, False, True]


@pytest.mark.parametrize("m,q,p", SHAPES[:-1])
def test_rlwr_boundary_residues_under_the_secret_one(gpu, m, q, p):
    """exact multiples of q in p l + floor(q/2) (where p is a unit mod q), l = -floor(q/2) and their neighbours"""
    c = ctx(gpu, m, q)
    n, h = c.n, q // 2
    special = [q - h, q - h - 1, (q - h + 1) % q, 0, 1, q - 1, h]
    if math.gcd(p, q) == 1:
        l0 = (-h * pow(p, -1, q)) % q
        lc = l0 if 2 * l0 < q else l0 - q
        assert (p * lc + h) % q == 0
        special = [l0, (l0 + 1) % q, (l0 - 1) % q] + special
    x = np.array([(special * n)[:n], (special[::-1] * n)[:n]], dtype=np.int64)
    one = np.zeros(n, dtype=np.int64)
    one[0] = 1                                                   # the ring's 1 in the powerful basis
    a_pow = rg.l_mod(m, x, q)                                    # a = l(x): lInv (a 1) = x
    assert np.array_equal(rg.x_dec(m, q, a_pow, one), x)
    got = c.r.roundedProd(c.r.prepare(one), a_pow, p)
    assert np.array_equal(got, rr.rlwr_round(x, q, p))


# ---------------------------------------------------------------------------------------------
# 2. Disc
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,q,p", SHAPES)
def test_disc_matches_restatement_and_the_plan_route(gpu, m, q, p):
    import torch
    c = ctx(gpu, m, q)
    r, n, svar, ctr = c.r, c.n, _svar(q), 1000 + m
    g = rr.gaussian_dec(c.pps, KEY, ctr, 5, svar)
    assert np.abs(g).max() + 1 < q / 2                           # the lift recovers e: no wrap mod q
    a, b = r.sampleDisc(c.shat, B, svar, key=KEY, ctr=ctr)
    assert a.shape == b.shape == (B, n)
    a_h, b_h = _h(a), _h(b)
    assert np.array_equal(a_h, rg.uniform(KEY, rr.DOM_RLWE_UNIFORM, ctr, B, n, q))
    assert b_h.min() >= 0 and b_h.max() < q
    e, nm = r.errorTermDisc(c.shat, a, b, norm=True)
    e_h = _h(e)
    assert np.array_equal(b_h, rg.disc_b(m, q, a_h, c.s_h, e_h))
    assert np.array_equal(e_h, rg.disc_error(m, q, a_h, b_h, c.s_h))
    want, near = er.round_coset(g[:B], np.zeros((B, n), dtype=np.int64), 1)
    off = e_h != want
    assert off.sum() <= 4 and near[off].all(), (int(off.sum()), int(near.sum()))
    assert np.array_equal(_h(nm), rr.gsqnorm_sat(c.pps, e_h))
    assert torch.equal(r.errorGSqNormDisc(c.shat, a, b), nm)
    # the same integers as the plan route draws for (m, svar, key, ctr), whatever q, a and s are
    qp = gpu.good_q(m, 2 ** 20)
    pr = gpu.RLWE(gpu.Plan.for_index(m, [qp]))
    sp = pr.secret(key=KEY, ctr=5)
    ap, bp = pr.sampleDisc(sp, B, svar, key=KEY, ctr=ctr)
    assert torch.equal(pr.errorTermDisc(sp, ap, bp), e)
    # the batch split at ctr, ctr + 2
    a5, b5 = r.sampleDisc(c.shat, 5, svar, key=KEY, ctr=ctr)
    a2, b2 = r.sampleDisc(c.shat, 2, svar, key=KEY, ctr=ctr)
    a3, b3 = r.sampleDisc(c.shat, 3, svar, key=KEY, ctr=ctr + 2)
    assert torch.equal(a5, torch.cat([a2, a3])) and torch.equal(b5, torch.cat([b2, b3]))
    assert torch.equal(a5[:3], a) and torch.equal(b5[:3], b)


# ---------------------------------------------------------------------------------------------
# 3. Cont
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,q,p", SHAPES)
def test_cont_matches_restatement(gpu, m, q, p):
    import torch
    c = ctx(gpu, m, q)
    r, n, svar, ctr = c.r, c.n, _svar(q), 2000 + m
    a, b = r.sampleCont(c.shat, B, svar, key=KEY, ctr=ctr)
    assert a.shape == b.shape == (B, n) and b.dtype == torch.float64
    a_h, b_h = _h(a), _h(b)
    assert np.array_equal(a_h, rg.uniform(KEY, rr.DOM_RLWE_UNIFORM, ctr, B, n, q))
    assert (b_h >= 0).all() and (b_h < float(q)).all()
    a5, b5 = r.sampleCont(c.shat, 5, svar, key=KEY, ctr=ctr)
    a2, b2 = r.sampleCont(c.shat, 2, svar, key=KEY, ctr=ctr)
    a3, b3 = r.sampleCont(c.shat, 3, svar, key=KEY, ctr=ctr + 2)
    assert torch.equal(a5, torch.cat([a2, a3]))
    assert torch.equal(b5.view(torch.int64), torch.cat([b2, b3]).view(torch.int64))
    assert torch.equal(b5[:3].view(torch.int64), b.view(torch.int64))
    g = rr.gaussian_dec(c.pps, KEY, ctr, B, svar)
    e, nm = r.errorTermCont(c.shat, a, b, norm=True)
    e_h = _h(e)
    assert (np.abs(e_h - g) <= 1e-12 * np.abs(g) + float(q) * 2.0 ** -52).all(), float(np.abs(e_h - g).max())
    nw = rr.gsqnorm_f64(c.pps, e_h)
    assert (np.abs(_h(nm) - nw) <= 1e-12 * nw).all()
    assert np.array_equal(_bits(nm), _bits(r.errorGSqNormCont(c.shat, a, b)))


@pytest.mark.parametrize("m,q", [(8, 2 ** 20), (45, 900)])
def test_error_term_cont_is_bit_identical_on_hand_made_b(gpu, m, q):
    c = ctx(gpu, m, q)
    r, n, qd = c.r, c.n, float(q)
    rng = np.random.default_rng(m)
    nb = 7
    a = rng.integers(0, q, size=(nb, n), dtype=np.int64)
    x = rg.x_dec(m, q, a, c.s_h)
    xd = x.astype(np.float64)
    b = np.stack([np.zeros(n), np.full(n, np.nextafter(qd, 0.0)), xd[2], rr.rrq_reduce(xd[3] + 0.25, qd),
                  rr.rrq_reduce(xd[4] - 0.25, qd), rr.rrq_reduce(xd[5] + qd / 2, qd),
                  rr.rrq_reduce(xd[6] + rng.normal(size=n) * 3.0, qd)])
    assert (b >= 0).all() and (b < qd).all()
    e, nm = r.errorTermCont(_h(c.shat), a, b, norm=True)
    want = rr.cont_error(x, b, q)
    assert np.array_equal(_bits(e), _bits(want))
    assert (e[2] == 0).all() and (np.abs(e[3]) == 0.25).all()
    nw = rr.gsqnorm_f64(c.pps, want)
    assert (np.abs(nm - nw) <= 1e-12 * nw).all()


# ---------------------------------------------------------------------------------------------
# 4. the fused tails against the general composition
# ---------------------------------------------------------------------------------------------
def _every_kind(c, p, svar):
    """every entry once: the outputs as bit patterns, in a fixed order"""
    r = c.r
    ad, bd = r.sampleDisc(c.shat, B, svar, key=KEY, ctr=10)
    ac, bc = r.sampleCont(c.shat, B, svar, key=KEY, ctr=20)
    ar, br = r.sampleRLWR(c.shat, B, p, key=KEY, ctr=30)
    ed, nd = r.errorTermDisc(c.shat, ad, bd, norm=True)
    ec, nc = r.errorTermCont(c.shat, ac, bc, norm=True)
    rp = r.roundedProd(c.shat, ar, p)
    mm = r.mismatchRLWR(c.shat, ar, br, p)
    return [_h(t).view(np.int64) if _h(t).dtype == np.float64 else _h(t) for t in (ad, bd, ac, bc, ar, br, ed, nd, ec, nc, rp, mm)]


@pytest.mark.parametrize("m,q,p", [(16, 2 ** 40, 2 ** 8), (16, 2 ** 61, 2 ** 30), (2 ** 14, 2 ** 17, 2)])
def test_fused_and_unfused_routes_give_the_same_bits(gpu, info, m, q, p):
    c = ctx(gpu, m, q)
    svar = _svar(q)
    info()
    fused = _every_kind(c, p, svar)
    lines = info()
    want = [("sample", 0), ("sample", 1), ("sample", 2), ("error", 0), ("error", 1), ("rounded_prod", 2), ("check", 2)]
    assert [(e, k) for e, k, _, _ in lines] == want
    assert [rt for _, _, rt, _ in lines] == ["fused"] * 6 + ["unfused"] and {K for *_, K in lines} == {KS[q]}
    gpu.debug_set("RLWE_RING_UNFUSED", True)
    try:
        unfused = _every_kind(c, p, svar)
        lines = info()
    finally:
        gpu.debug_set("RLWE_RING_UNFUSED", False)
    assert [(e, k) for e, k, _, _ in lines] == want and [rt for _, _, rt, _ in lines] == ["unfused"] * 7
    for i, (x, y) in enumerate(zip(fused, unfused)):
        assert np.array_equal(x, y), i


def test_other_indices_take_the_general_route(gpu, info):
    c = ctx(gpu, 12, 105)
    info()
    c.r.sampleRLWR(c.shat, B, 7, key=KEY, ctr=1)
    assert info() == [("sample", 2, "unfused", 1)]


# ---------------------------------------------------------------------------------------------
# 5. two conventions, one ring
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [16, 45])
def test_ring_route_and_plan_route_verify_each_other(gpu, m):
    import torch
    q = gpu.good_q(m, 2 ** 20)
    c = ctx(gpu, m, q)
    n, svar = c.n, 0.28125
    pr = gpu.RLWE(c.plan)
    crt = lambda t: c.plan.crt(t.clone().reshape(-1, n, 1))
    inv = lambda t: c.plan.crtInv(t.clone()).reshape(-1, n)
    s_crt = crt(c.s)[0]
    # ring-route samples, taken to the CRT basis, under the plan route
    a, b = c.r.sampleDisc(c.shat, B, svar, key=KEY, ctr=50)
    e = c.r.errorTermDisc(c.shat, a, b)
    assert torch.equal(pr.errorTermDisc(s_crt, crt(a), crt(b)), e)
    ar, br = c.r.sampleRLWR(c.shat, B, 2, key=KEY, ctr=60)
    assert pr.validRLWR(s_crt, crt(ar), br, 2).all() and torch.equal(pr.roundedProd(s_crt, crt(ar), 2), br)
    # plan-route samples, taken to the powerful basis, under the ring route
    s2 = pr.secret(key=KEY, ctr=9)
    shat2 = c.r.prepare(inv(s2.reshape(1, n, 1))[0])
    a2, b2 = pr.sampleDisc(s2, B, svar, key=KEY, ctr=70)
    e2 = pr.errorTermDisc(s2, a2, b2)
    assert torch.equal(c.r.errorTermDisc(shat2, inv(a2), inv(b2)), e2)
    assert torch.equal(e2, c.r.errorTermDisc(c.shat, *c.r.sampleDisc(c.shat, B, svar, key=KEY, ctr=70)))   # the same e
    a3, b3 = pr.sampleCont(s2, B, svar, key=KEY, ctr=80)
    e3 = pr.errorTermCont(s2, a3, b3)
    assert np.array_equal(_bits(c.r.errorTermCont(shat2, inv(a3), b3)), _bits(e3))


# ---------------------------------------------------------------------------------------------
# 6. verification end to end on challenge lines
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,q,svar", [(256, 512, 7.8125e-3), (243, 729, 6.172839506172839e-3), (500, 500, 5e-3)])
def test_challenge_instances_verify_with_their_secret_only(gpu, m, q, svar):
    import torch
    assert ("Disc", m, q, svar) in rg.challenge_lines() and ("Cont", m, q, svar) in rg.challenge_lines()
    c = ctx(gpu, m, q)
    r = c.r
    _, other = r.secret(key=KEY, ctr=1)
    assert not torch.equal(other, c.shat)
    bound = r.errorBound(m, svar, eps=2.0 ** -25, kind="disc")
    assert bound == rr.error_bound_disc(m, svar, 2.0 ** -25)
    a, b = r.sampleDisc(c.shat, B, svar, key=KEY, ctr=10)
    assert r.validDisc(bound, c.shat, a, b).all() and not r.validDisc(bound, other, a, b).any()
    e = _h(r.errorTermDisc(c.shat, a, b))
    assert np.array_equal(_h(b), rg.disc_b(m, q, _h(a), c.s_h, e))
    cb = r.errorBound(m, svar, eps=2.0 ** -25, kind="cont")
    a, b = r.sampleCont(c.shat, B, svar, key=KEY, ctr=20)
    assert r.validCont(cb, c.shat, a, b).all() and not r.validCont(cb, other, a, b).any()


@pytest.mark.parametrize("m,q,p", [(32, 32, 2), (84, 42, 2)])
def test_challenge_rlwr_instances_verify_with_their_secret_only(gpu, m, q, p):
    assert ("RLWR", m, q, p) in rg.challenge_lines()
    c = ctx(gpu, m, q)
    r = c.r
    _, other = r.secret(key=KEY, ctr=1)
    a, b = r.sampleRLWR(c.shat, B, p, key=KEY, ctr=10)
    assert np.array_equal(_h(b), rg.rlwr_b(m, q, p, _h(a), c.s_h))
    assert r.validRLWR(c.shat, a, b, p).all() and not r.validRLWR(other, a, b, p).any()


# ---------------------------------------------------------------------------------------------
# 7. status codes on the device, a side stream, numpy and CUDA inputs
# ---------------------------------------------------------------------------------------------
def test_host_statuses_leave_the_outputs_untouched(gpu):
    import torch
    L = gpu.lib()
    c = ctx(gpu, 12, 105)
    n, K = c.n, c.r.K
    h, pq = c.r.ring._h, c.plan._h
    other = gpu.Plan.for_index(12, [104])
    SENT = -0x0123456789ABCDEF
    a = torch.full((B, n), SENT, dtype=torch.int64, device="cuda")
    b = torch.full((B, n), SENT, dtype=torch.int64, device="cuda")
    nm = torch.full((B,), SENT, dtype=torch.int64, device="cuda")
    mm = torch.full((B,), 0x1234567, dtype=torch.int32, device="cuda")
    work = torch.zeros(c.r._work_len(0, B)(), dtype=torch.int64, device="cuda")
    P = lambda t: t.data_ptr()
    sample = lambda kind, p, svar, hh, pp, shat, ao, bo, w, nb: L.lolhip_rlwe_ring_sample_batch(
        hh, pp, None, kind, p, shat, svar, KEY, 0, ao, bo, w, nb)
    good = (h, pq, P(c.shat), P(a), P(b), P(work), B)
    assert sample(3, 2, 1.0, *good) == INVALID and sample(2, 105, 1.0, *good) == INVALID
    assert sample(2, 1, 1.0, *good) == INVALID and sample(0, 0, 0.0, *good) == INVALID
    assert sample(1, 0, float("nan"), *good) == INVALID
    assert sample(2, 2, 1.0, h, other._h, *good[2:]) == INVALID
    assert sample(2, 2, 1.0, h, pq, P(c.shat), P(a), P(b), P(work), -1) == INVALID
    for hole in range(2, 6):                                     # one NULL pointer at B > 0
        args = list(good)
        args[hole] = None
        assert sample(2, 2, 1.0, *args) == INVALID, hole
    assert L.lolhip_rlwe_ring_sample_batch(h, pq, None, 2, 2, P(c.shat), 1.0, None, 0, P(a), P(b), P(work), B) == INVALID
    err = lambda kind, eo, no, nb=B, bb=P(b): L.lolhip_rlwe_ring_error_batch(h, pq, None, kind, P(a), bb, P(c.shat), eo, no,
                                                                           P(work), nb)
    assert err(0, None, None) == INVALID and err(2, P(b), P(nm)) == INVALID and err(0, P(b), P(nm), bb=None) == INVALID
    assert L.lolhip_rlwr_ring_rounded_prod_batch(h, pq, 105, None, P(a), P(c.shat), P(b), P(work), B) == INVALID
    assert L.lolhip_rlwr_ring_rounded_prod_batch(h, pq, 7, None, P(a), P(c.shat), None, P(work), B) == INVALID
    assert L.lolhip_rlwr_ring_check_batch(h, pq, 7, None, P(a), P(b), P(c.shat), None, P(work), B) == INVALID
    assert L.lolhip_rlwr_ring_check_batch(h, pq, 0, None, P(a), P(b), P(c.shat), P(mm), P(work), B) == INVALID
    torch.cuda.synchronize()
    assert (a == SENT).all() and (b == SENT).all() and (nm == SENT).all() and (mm == 0x1234567).all()
    # B = 0 is OK and writes nothing, null pointers or not
    assert sample(2, 2, 1.0, h, pq, None, None, None, None, 0) == 0 and err(0, None, None, nb=0) == 0
    torch.cuda.synchronize()
    assert (a == SENT).all() and (b == SENT).all()


def test_side_stream_and_numpy_inputs(gpu):
    import torch
    c = ctx(gpu, 27, 81)
    r, svar = c.r, 0.28125
    a, b = r.sampleDisc(c.shat, B, svar, key=KEY, ctr=300)
    e, nm = r.errorTermDisc(c.shat, a, b, norm=True)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a1, b1 = r.sampleDisc(c.shat, B, svar, key=KEY, ctr=300, stream=st.cuda_stream)
        e1, n1 = r.errorTermDisc(c.shat, a1, b1, norm=True, stream=st.cuda_stream)
    st.synchronize()
    assert torch.equal(a1, a) and torch.equal(b1, b) and torch.equal(e1, e) and torch.equal(n1, nm)
    # numpy in, numpy out; the samplers return CUDA tensors whatever the secret is given as
    shat_h = _h(c.shat)
    a2, b2 = r.sampleDisc(shat_h, B, svar, key=KEY, ctr=300)
    assert a2.is_cuda and torch.equal(a2, a) and torch.equal(b2, b)
    e2 = r.errorTermDisc(shat_h, _h(a), _h(b))
    assert isinstance(e2, np.ndarray) and np.array_equal(e2, _h(e))
    assert isinstance(r.roundedProd(shat_h, _h(a), 3), np.ndarray)
    assert np.array_equal(_h(r.prepare(c.s_h)), shat_h)
