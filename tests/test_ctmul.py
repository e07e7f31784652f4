"""The SymmSHE ciphertext product (*) of any degree on the device (GPU): lolhip_ct_mul_batch / Plan.ctMul, the
ciphertext-level key switches and embedCT / twaceCT.

 1. parity, bit for bit, with the restatement of tests/ctmul_ref.py: every component-count class of the kernel (the
    compiled-in counts up to 3 x 3 and the run-time form), all four encoding pairs, both bases in and out, narrow, wide,
    mixed and 16 moduli, B = 1 and 3; the square against the general route on two copies;
 2. tiles: a slab below one tile, tile starts inside polynomials, the one-word route against the 16-byte route, a side
    stream, guard rows around the output, the work buffer's tail;
 3. saturation in closed form: every residue q_t - 1, 8 x 8 components, at the top of every modulus class;
 4. properties with the GPU as the engine: encrypt, multiply, (key switch,) decrypt;
 5. statuses on the device, the output untouched.
Shapes are the smallest at which the pass can still go wrong: n = 16, 24, 32 for parity (one tile), index 512 for more
than one tile.
"""
import ctypes as C
from math import gcd, prod

import numpy as np
import pytest

import ctmul_ref as cm
import public_ref as pr
import saturate as sat
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params
from test_rns_width_host import good_below, mixed16

pytestmark = pytest.mark.gpu
KEY = bytes(range(32))
SENT = 0x5A5A5A5A5A5A5A5A
INVALID, NO_CRT = -1, -3
ENCS = [("LSD", "LSD"), ("LSD", "MSD"), ("MSD", "LSD"), ("MSD", "MSD")]
SHAPES = [(1, 1), (1, 3), (2, 2), (3, 2), (2, 3), (4, 5), (8, 8)]


def _moduli(m, kind):
    if kind == "30":
        return [good_below(m, 2 ** 30)]
    if kind == "61":
        return [good_below(m, 2 ** 61)]
    if kind == "mixed3":
        return [good_below(m, 2 ** 27), good_below(m, 2 ** 62), good_below(m, 2 ** 32)]
    return mixed16(m)


def _uniform(rng, shape, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=shape, dtype=np.int64) for q in qs], axis=-1))


def _crt(cpuref, P, x):
    return np.asarray(cpuref.crt(P, np.ascontiguousarray(x.reshape(-1, P.n, P.T)))).reshape(x.shape)


# ---------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["30", "61", "mixed3", "mixed16"])
@pytest.mark.parametrize("m", [32, 96, 45])
def test_product_equals_the_restatement_bit_for_bit(gpu, cpuref, m, kind):
    qs = _moduli(m, kind)
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(m + len(qs))
    p = 5
    assert gcd(prod(qs), p) == 1
    seen = set()
    for si, (na, nb) in enumerate(SHAPES):
        B = (1, 3)[si % 2]
        a, b = _uniform(rng, (na, B, P.n), qs), _uniform(rng, (nb, B, P.n), qs)
        ac, bc = _crt(cpuref, P, a), _crt(cpuref, P, b)
        for bi, (cs_crt, out_crt) in enumerate([(False, False), (False, True), (True, False), (True, True)]):
            # 2 x 2 without a factor runs the kernel of lolhip_ctmul_crt_batch, with one k_ct_mul<2, 2>: both, every time
            pairs = [ENCS[0], ENCS[3]] if (na, nb) == (2, 2) else [ENCS[(si + bi) % 4]]
            for e1, e2 in pairs:
                k1, l1, k2, l2 = (0, 1, 3)[si % 3], (1, p - 1, 2)[bi % 3], (0, 1, 3)[bi % 3], (2, 1, p - 1)[si % 3]
                want = cm.ct_mul(cpuref, P, {"enc": e1, "k": k1, "l": l1, "c": ac, "crt": True},
                                 {"enc": e2, "k": k2, "l": l2, "c": bc, "crt": True}, p, out_crt=out_crt)
                x, y = (ac, bc) if cs_crt else (a, b)
                if bi % 2:                                        # representatives in (-q, 0]
                    x, y = sat.neg_rep(x, qs), sat.neg_rep(y, qs)
                got, enc, k, l = pq.ctMul((x, e1, k1, l1), (y, e2, k2, l2), p=p, cs_crt=cs_crt, out_crt=out_crt)
                assert (enc, k, l) == (want["enc"], want["k"], want["l"]), (na, nb, e1, e2)
                assert got.shape == (na + nb - 1, B, P.n, P.T)
                assert np.array_equal(got, want["c"]), (na, nb, e1, e2, cs_crt, out_crt)
                seen.add((e1, e2))
    assert len(seen) == 4


@pytest.mark.parametrize("m,kind", [(32, "mixed3"), (96, "61"), (45, "mixed16")])
def test_square_equals_the_general_route_on_two_copies(gpu, cpuref, m, kind):
    import torch
    qs = _moduli(m, kind)
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(m)
    p = 5
    for na in (1, 2, 3, 8):
        for cs_crt, enc in ((True, "MSD"), (False, "LSD")):
            a = _uniform(rng, (na, 3, P.n), qs)
            ta = torch.from_numpy(a).cuda()
            ct = (ta, enc, 1, 2)
            sq = pq.ctMul(ct, p=p, cs_crt=cs_crt)
            same = pq.ctMul(ct, ct, p=p, cs_crt=cs_crt)
            two = pq.ctMul(ct, (ta.clone(), enc, 1, 2), p=p, cs_crt=cs_crt)
            assert torch.equal(ta.cpu(), torch.from_numpy(a))       # the operands are only read
            assert sq[1:] == two[1:] == same[1:]
            assert torch.equal(sq[0], two[0]) and torch.equal(same[0], two[0]), (na, cs_crt)
            ref = {"enc": enc, "k": 1, "l": 2, "c": a, "crt": cs_crt}
            want = cm.ct_mul(cpuref, P, ref, ref, p, out_crt=cs_crt)
            assert np.array_equal(sq[0].cpu().numpy(), want["c"]) and sq[1:] == (want["enc"], want["k"], want["l"])


# ---------------------------------------------------------------------------------------------
# 2. tiles
# ---------------------------------------------------------------------------------------------
def _raw(gpu, pq, a, na, b, nb, cs_crt, alpha, out, out_crt, work, B, stream=None):
    import torch
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    al = None if alpha is None else (C.c_int64 * pq.T)(*[int(x) for x in alpha])
    return gpu.lib().lolhip_ct_mul_batch(pq._h, st, a.data_ptr(), na, b.data_ptr(), nb, int(cs_crt), al,
                                         None if out is None else out.data_ptr(), int(out_crt),
                                         None if work is None else work.data_ptr(), B)


def test_slab_below_one_tile(gpu, cpuref):
    """B = 3, n = 16, T = 3: 144 words, one partly filled workgroup"""
    qs = _moduli(32, "mixed3")
    P = Params(lm.factor_pps(32), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(1)
    a, b = _uniform(rng, (2, 3, P.n), qs), _uniform(rng, (2, 3, P.n), qs)
    for enc in ("MSD", "LSD"):                                     # k_ct_mul<2, 2> (the toLSD factor), then k_ctmul
        got = pq.ctMul((a, enc, 0, 1), (b, enc, 0, 1), p=5, cs_crt=True)[0]
        want = cm.ct_mul(cpuref, P, {"enc": enc, "k": 0, "l": 1, "c": a, "crt": True},
                         {"enc": enc, "k": 0, "l": 1, "c": b, "crt": True}, 5, out_crt=True)
        assert np.array_equal(got, want["c"]), enc


def test_tile_starts_inside_polynomials_routes_stream_guards_and_work_tail(gpu, cpuref):
    """Index 512, T = 3, B = 5: slabs of 3840 words are 3.75 tiles of the 16-byte route and 7.5 of the one-word route,
    and every tile start but the first falls inside a polynomial (768 words).  The one-word route (every operand and the
    output offset by 8 bytes) equals the 16-byte route bit for bit; so does a side stream; the rows before and after the
    output keep their sentinel; the work buffer's tail (work_len + 4096 words) keeps its sentinel."""
    import torch
    m, B, p = 512, 5, 3
    qs = _moduli(m, "mixed3")
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    rng = np.random.default_rng(2)
    slab = B * P.n * P.T
    assert slab % 1024 and slab % 512 and 1024 % (P.n * P.T)
    for na, nb in ((2, 2), (2, 3), (4, 5)):
        a, b = _uniform(rng, (na, B, P.n), qs), _uniform(rng, (nb, B, P.n), qs)
        ca = {"enc": "MSD", "k": 0, "l": 1, "c": a, "crt": True}
        cb = {"enc": "MSD", "k": 2, "l": 2, "c": b, "crt": True}
        alpha = cm.rule(qs, p, "MSD", 0, 1, "MSD", 2, 2)[0]
        want = torch.from_numpy(cm.ct_mul(cpuref, P, ca, cb, p, out_crt=True)["c"]).cuda()
        no = na + nb - 1
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        # the 16-byte route, guard rows around the output
        buf = torch.full(((no + 2) * slab,), SENT, dtype=torch.int64, device="cuda")
        out = buf[slab:(no + 1) * slab]
        assert all(t.data_ptr() % 16 == 0 for t in (ta, tb, out))
        assert _raw(gpu, pq, ta, na, tb, nb, True, alpha, out, True, None, B) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.reshape(want.shape), want)
        assert bool((buf[:slab] == SENT).all()) and bool((buf[(no + 1) * slab:] == SENT).all())
        # the one-word route: views offset by 8 bytes
        oa = torch.empty(ta.numel() + 1, dtype=torch.int64, device="cuda")[1:].copy_(ta.reshape(-1))
        ob = torch.empty(tb.numel() + 1, dtype=torch.int64, device="cuda")[1:].copy_(tb.reshape(-1))
        buf1 = torch.full(((no + 2) * slab + 1,), SENT, dtype=torch.int64, device="cuda")
        out1 = buf1[slab + 1:(no + 1) * slab + 1]
        assert all(t.data_ptr() % 16 == 8 for t in (oa, ob, out1))
        assert _raw(gpu, pq, oa, na, ob, nb, True, alpha, out1, True, None, B) == 0
        torch.cuda.synchronize()
        assert torch.equal(out1, out)
        assert bool((buf1[:slab + 1] == SENT).all()) and bool((buf1[(no + 1) * slab + 1:] == SENT).all())
        # a side stream
        side = torch.cuda.Stream()
        out2 = torch.full_like(out, SENT)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert _raw(gpu, pq, ta, na, tb, nb, True, alpha, out2, True, None, B, stream=side.cuda_stream) == 0
        side.synchronize()
        assert torch.equal(out2, out)
    # powerful basis in and out over a work buffer with a sentinel tail; the square's shorter layout too
    a = _uniform(rng, (3, B, P.n), qs)
    ta = torch.from_numpy(a).cuda()
    L = gpu.lib()
    for tb, sq in ((ta.clone(), 0), (ta, 1)):
        wl = L.lolhip_ct_mul_work_len(pq._h, 3, 3, 0, sq, B)
        assert wl == cm.work_len(P.n, P.T, 3, 3, False, sq, B) > 0
        work = torch.full((wl + 4096,), SENT, dtype=torch.int64, device="cuda")
        out = torch.zeros((5, B, P.n, P.T), dtype=torch.int64, device="cuda")
        assert _raw(gpu, pq, ta, 3, tb, 3, False, None, out, False, work, B) == 0
        torch.cuda.synchronize()
        assert bool((work[wl:] == SENT).all()) and not bool((work[:wl] == SENT).all())
        want = pq.ctMul((ta, "LSD", 0, 1), p=p)[0]
        assert torch.equal(out, want) and torch.equal(ta.cpu(), torch.from_numpy(a))
    ref = {"enc": "LSD", "k": 0, "l": 1, "c": a}
    assert np.array_equal(want.cpu().numpy(), cm.ct_mul(cpuref, P, ref, ref, p)["c"])


# ---------------------------------------------------------------------------------------------
# 3. saturation
# ---------------------------------------------------------------------------------------------
def _sat_moduli(m):
    tops = {k: sat.class_top(m, k)[0] for k in ("62", "61", "32", "30")}
    return [[tops[k]] for k in ("62", "61", "32", "30")] + [[tops["30"], tops["62"], tops["32"]]]


@pytest.mark.parametrize("which", range(5))
def test_saturated_accumulators_in_closed_form(gpu, which):
    """CRT in and out, every residue q_t - 1, na = nb = 8: every raw product is (q_t - 1)^2 and
    out_k = alpha_t gCRT (number of pairs i + j = k) mod q_t, with no transform in the way.  The general route and the
    square, alpha = 1 and the toLSD factor p mod q_t."""
    import torch
    m, B, p = 96, 2, 5
    qs = _sat_moduli(m)[which]
    P = Params(lm.factor_pps(m), qs)
    pq = gpu.Plan(P.pps, qs)
    g = cm.g_crt(P)
    assert np.array_equal(pq.gCRT(), g.astype(np.int64))
    a = torch.from_numpy(sat.full_q1((8, B, P.n), qs)).cuda()
    b = a.clone()
    for e in ("LSD", "MSD"):
        alpha = cm.rule(qs, p, e, 0, 1, e, 0, 1)[0]
        want = cm.saturated(qs, alpha, g, 8, 8)[:, None]
        for ct2 in ((b, e, 0, 1), None):
            got = pq.ctMul((a, e, 0, 1), ct2, p=p, cs_crt=True)[0].cpu().numpy()
            assert np.array_equal(got, np.broadcast_to(want, got.shape)), (e, ct2 is None)
    # representatives -1 (in (-q, 0]) give the same
    neg = torch.full_like(a, -1)
    got = pq.ctMul((neg, "LSD", 0, 1), (b, "LSD", 0, 1), p=p, cs_crt=True)[0].cpu().numpy()
    assert np.array_equal(got, np.broadcast_to(cm.saturated(qs, [1] * len(qs), g, 8, 8)[:, None], got.shape))


# ---------------------------------------------------------------------------------------------
# 4. properties, the GPU as the engine
# ---------------------------------------------------------------------------------------------
class _Dev:
    """device plans, a key and helpers for plaintext index 8 inside ciphertext index mp"""

    def __init__(self, gpu, cpuref, mp, p, qs, ctr=0):
        self.p, self.qs, self.mp = p, qs, mp
        pps = lm.factor_pps(mp)
        self.P = Params(pps, qs)
        self.pq, self.pp = gpu.Plan(pps, qs), gpu.Plan(pps, [p])
        self.ext = gpu.Ext(gpu.Plan(lm.factor_pps(8), [p]), self.pp)
        self.s_crt = self.key(ctr)
        self.cpuref, self.ctr = cpuref, 100

    def key(self, ctr):
        z = self.pq.errorRounded(0.5, B=1, key=KEY, ctr=ctr).cpu().numpy()
        return np.ascontiguousarray(self.pq.crt(self.pq.l(pr.reduce(z, self.qs)))[0])

    def encrypt(self, pt):
        self.ctr += pt.shape[0]
        cs = self.pq.encrypt(pt, self.s_crt, self.pp, 0.5, key=KEY, ctr=self.ctr - pt.shape[0], ext=self.ext)
        return cs, "LSD", 0, 1

    def decrypt(self, ct, s_crt=None, cs_crt=False):
        cs, enc, k, l = ct
        return self.pq.decrypt(cs, self.s_crt if s_crt is None else s_crt, self.pp, ext=self.ext, enc=enc, k=k, l=l,
                               cs_crt=cs_crt)

    def error_ratio(self, ct):
        """Q / (2 p max |errorTerm|) of an LSD ciphertext ct (powerful basis), errorTerm in Python integers over the
        CPU model (oracle/she_model.py)"""
        cs, enc, _, _ = ct
        assert enc == "LSD"
        she = sm.SHE(sm.CpuEngine(self.cpuref, self.P), None, self.qs, self.p, None)
        she.s_crt = self.s_crt[None]
        err = she.lift(she.e.lInv(she.evaluate([np.ascontiguousarray(c) for c in cs])))
        return she.Q / (2 * self.p * max(1, int(np.abs(err).max())))


def _pts(rng, count, B, p):
    return [rng.integers(0, p, size=(B, 4), dtype=np.int64) for _ in range(count)]


def _ptmul(p, *pts):
    out = pts[0]
    for x in pts[1:]:
        out = np.stack([pr.negacyclic(out[i], x[i], p) for i in range(len(x))]).astype(np.int64)
    return out


PROPS = [(32, 3, "2x30"), (32, 5, "61"), (96, 5, "2x30"), (96, 5, "61")]


def _prop_moduli(mp, which):
    if which == "61":
        return [good_below(mp, 2 ** 61)]
    g = lm.good_qs(mp, 2 ** 29)
    return [next(g), next(g)]


@pytest.mark.parametrize("mp,p,which", PROPS)
def test_products_decrypt_to_the_plaintext_products(gpu, cpuref, mp, p, which):
    """encrypt on the device, multiply, decrypt.  Index 96 = 32 * 3 takes p = 5 only: a product has k >= 1 and decrypt
    divides by g, which needs oddRad(m') = 3 invertible mod p (the reference's own condition on p).

    Before a parameter set is trusted, the degree-3 error is computed: the restatement's ct1 * ct2 * ct3 (tests/ctmul_ref.py)
    through the CPU model's integer errorTerm must stay below Q / (2 p) by a factor of at least 4, so that a decryption
    failure can only mean a wrong product.  Computed Q / (2 p max |errorTerm|) for B = 2, the key and streams below (each
    run prints it): m' = 32, p = 3, two 30-bit moduli 2.2e13; m' = 32, p = 5, one 61-bit modulus 2.1e13; m' = 96, p = 5,
    two 30-bit moduli 3.4e11; m' = 96, p = 5, one 61-bit modulus 2.7e12."""
    qs = _prop_moduli(mp, which)
    d = _Dev(gpu, cpuref, mp, p, qs)
    pq, B = d.pq, 2
    rng = np.random.default_rng(mp + p)
    x1, x2, x3 = _pts(rng, 3, B, p)
    c1, c2, c3 = d.encrypt(x1), d.encrypt(x2), d.encrypt(x3)
    assert np.array_equal(d.decrypt(c1), x1)
    # the noise budget, from the restatement and integer arithmetic alone
    as_ref = lambda ct: {"enc": ct[1], "k": ct[2], "l": ct[3], "c": ct[0]}
    r123 = cm.ct_mul(cpuref, d.P, cm.ct_mul(cpuref, d.P, as_ref(c1), as_ref(c2), p), as_ref(c3), p)
    ratio = d.error_ratio((r123["c"], r123["enc"], r123["k"], r123["l"]))
    print(f"ctmul noise: m'={mp} p={p} moduli={which}: Q / (2 p max|errorTerm|) of degree 3 = {ratio:.3e}")
    assert ratio >= 4
    # ct1 * ct2 * ct3, no key switch in between: four components
    c12 = pq.ctMul(c1, c2, p=p)
    c123 = pq.ctMul(c12, c3, p=p)
    assert c123[0].shape[0] == 4 and c123[1:] == ("LSD", 2, 1)
    assert np.array_equal(c123[0], r123["c"])
    assert np.array_equal(d.decrypt(c123), _ptmul(p, x1, x2, x3))
    # the same through the CRT basis, and with an MSD operand
    to_crt = lambda ct: (np.stack([pq.crt(np.ascontiguousarray(c)) for c in ct[0]]),) + tuple(ct[1:])
    m3 = pq.toMSD(c3[0], p, "LSD", 1)
    k123 = pq.ctMul(pq.ctMul(to_crt(c1), to_crt(c2), p=p, cs_crt=True), to_crt((m3[0], m3[1], 0, m3[2])), p=p, cs_crt=True)
    assert k123[1] == "MSD" and k123[2] == 2
    assert np.array_equal(d.decrypt(k123, cs_crt=True), _ptmul(p, x1, x2, x3))
    # the square of a quadratic ciphertext: five components
    c12sq = pq.ctMul(c12, p=p)
    assert c12sq[0].shape[0] == 5 and c12sq[2] == 3
    x12 = _ptmul(p, x1, x2)
    assert np.array_equal(d.decrypt(c12sq), _ptmul(p, x12, x12))
    # keySwitchQuadCirc hint (ct1 * ct2)
    base = 256
    hint = pq.ksQuadCircHint(d.s_crt, 0.5, base, key=KEY, ctr=1000)
    lin = pq.keySwitchQuadCirc(hint, c12, base, p)
    assert lin[0].shape == (2, B, pq.n, pq.T) and lin[1] == "MSD" and lin[2] == 1
    assert np.array_equal(d.decrypt(lin, cs_crt=True), x12)
    assert pq.keySwitchQuadCirc(hint, c1, base, p) is c1              # too short: returned unchanged
    # ct * one: (enc, k, l) as the rule says, the plaintext unchanged
    one = np.zeros((1, B, pq.n, pq.T), dtype=np.int64)
    one[0, :, 0, :] = 1
    for ct in (c1, (m3[0], m3[1], 0, m3[2])):
        t1 = pq.ctMul(ct, (one, "LSD", 0, 1), p=p)
        assert t1[0].shape[0] == 2 and t1[1:] == (ct[1], 1, ct[3] % p)
        assert np.array_equal(d.decrypt(t1), x1 if ct is c1 else x3)
    # (a * b) + (b * a): equal (enc, k, l), so (+) aligns nothing
    ab, ba = pq.ctMul(c1, (m3[0], m3[1], 0, m3[2]), p=p), pq.ctMul((m3[0], m3[1], 0, m3[2]), c1, p=p)
    assert ab[1:] == ba[1:] and np.array_equal(ab[0], ba[0])
    s = pq.ctAdd(ab, ba, p)
    assert s[1:] == ab[1:] and np.array_equal(s[0], pq.ctLinComb(ab[0], 1, ba[0], 1))
    assert np.array_equal(d.decrypt(s), 2 * _ptmul(p, x1, x3) % p)


@pytest.mark.parametrize("mp,p", [(32, 3), (96, 3), (96, 5)])
def test_key_switch_linear_and_ring_maps_keep_the_plaintext(gpu, cpuref, mp, p):
    """keySwitchLinear from s_in to s_out, and twaceCT . embedCT; k = 0 throughout, so p = 3 serves index 96 too"""
    g = lm.good_qs(3 * mp, 2 ** 29)                               # moduli that also serve the ring embedCT maps into
    qs = [next(g), next(g)]
    d = _Dev(gpu, cpuref, mp, p, qs)
    pq, B, base = d.pq, 2, 256
    rng = np.random.default_rng(mp * p)
    (x,) = _pts(rng, 1, B, p)
    ct = d.encrypt(x)
    s_out = d.key(1)
    hint = pq.ksLinearHint(s_out, d.s_crt, 0.5, base, key=KEY, ctr=2000)
    for c, crt in ((ct, False), ((np.stack([pq.crt(np.ascontiguousarray(v)) for v in ct[0]]), "LSD", 0, 1), True)):
        sw = pq.keySwitchLinear(hint, c, base, p, cs_crt=crt)
        assert sw[0].shape == (2, B, pq.n, pq.T) and sw[1] == "MSD" and sw[2] == 0
        assert np.array_equal(d.decrypt(sw, s_crt=s_out, cs_crt=True), x)
    short = (ct[0][:1], "LSD", 0, 1)
    assert pq.keySwitchLinear(hint, short, base, p) is short
    with pytest.raises(ValueError):
        pq.keySwitchLinear(hint, (np.concatenate([ct[0], ct[0][:1]]), "LSD", 0, 1), base, p)
    # embedCT into a larger ciphertext ring and twaceCT back
    hi = gpu.Plan.for_index(3 * mp, qs)
    x_ct = gpu.Ext(pq, hi)
    for basis in ("pow", "crt"):
        cs = ct[0] if basis == "pow" else np.stack([pq.crt(np.ascontiguousarray(v)) for v in ct[0]])
        up = x_ct.embedCT((cs, "LSD", 0, 1), basis)
        assert up[0].shape == (2, B, hi.n, hi.T) and up[1:] == ("LSD", 0, 1)
        back = x_ct.twaceCT(up, basis)
        assert back[0].shape == (2, B, pq.n, pq.T) and back[1:] == ("LSD", 0, 1)
        assert np.array_equal(d.decrypt(back, cs_crt=basis == "crt"), x)
    for f, c in ((x_ct.embedCT, ct[0]), (x_ct.twaceCT, up[0])):
        with pytest.raises(ValueError):
            f((c, "LSD", 1, 1), "pow")


# ---------------------------------------------------------------------------------------------
# 5. statuses on the device
# ---------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_output_untouched(gpu):
    import torch
    qs = _moduli(32, "mixed3")
    pq = gpu.Plan(lm.factor_pps(32), qs)
    ncrt = gpu.Plan(lm.factor_pps(32), [2 ** 20, 2 ** 21 + 1, 2 ** 22 + 3])
    B = 2
    a = torch.zeros((9, B, pq.n, pq.T), dtype=torch.int64, device="cuda")
    b = torch.ones((9, B, pq.n, pq.T), dtype=torch.int64, device="cuda")
    out = torch.full((17, B, pq.n, pq.T), SENT, dtype=torch.int64, device="cuda")
    work = torch.zeros(18 * B * pq.n * pq.T, dtype=torch.int64, device="cuda")
    assert _raw(gpu, pq, a, 2, b, 2, True, None, a, True, work, B) == INVALID        # out = a
    assert _raw(gpu, pq, a, 2, b, 2, True, None, b, True, work, B) == INVALID        # out = b
    assert _raw(gpu, pq, a, 9, b, 2, True, None, out, True, work, B) == INVALID
    assert _raw(gpu, pq, a, 2, b, 9, False, None, out, False, work, B) == INVALID
    assert _raw(gpu, pq, a, 2, b, 2, False, None, out, False, None, B) == INVALID    # no work for the powerful basis
    assert _raw(gpu, ncrt, a, 2, b, 2, True, None, out, True, work, B) == NO_CRT
    assert _raw(gpu, ncrt, a, 2, b, 2, False, None, out, False, work, B) == NO_CRT
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and not bool(a.any()) and bool((b == 1).all())
    with pytest.raises(gpu.LolHipError) as e:
        pq.ctMul((a, "LSD", 0, 1), (b[:2], "LSD", 0, 1), p=3, cs_crt=True)
    assert e.value.code == INVALID
    # a valid call on the same buffers still works
    assert _raw(gpu, pq, a, 2, b, 2, True, None, out, True, None, B) == 0
    torch.cuda.synchronize()
    assert not bool(out[:3].any()) and bool((out[3:] == SENT).all())
