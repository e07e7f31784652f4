"""Host side of the homomorphic rounding 2^e -> 2 (include/lolhip.h lolhip_ct_affine_mul_batch, lolhip_ptround_*;
lol-apps HomomPRF.hs:215-270): no GPU needed.

 - the five entries are exported and declared, and lol_amd has Plan.ctAffineMul and PTRound;
 - the restatement of tests/ptround_ref.py over the CPU oracle against the closed form: for p = 4, 8, 16 and every
   constant plaintext c the result decrypts to floor((c + p/4) / (p/2)) mod 2, with k_out = 2^(e-1) - 1;
 - the same at p = 8 on random plaintexts, against the tree run on plaintexts with exact ring arithmetic;
 - every status of the entries on host-only plans by dry runs, sentinel-filled outputs untouched; work lengths;
 - the kernel's 128-bit bound and the k / l arithmetic in Python integers at q just below 2^62.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ptround_ref as ptr
import public_ref as pr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_ct_affine_mul_batch", "lolhip_ptround_create", "lolhip_ptround_destroy", "lolhip_ptround_work_len",
       "lolhip_ptround_batch")
INVALID, MODULUS, NO_CRT, NO_DEVICE = -1, -2, -3, -5
SENT = 0x5A5A5A5A


def test_ptround_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"
    assert callable(lolhip.Plan.ctAffineMul)
    for nm in ("__call__", "workLen", "hints"):
        assert callable(getattr(lolhip.PTRound, nm))


# ---- the model against the closed form ---------------------------------------------------------------------------------
def _ladder(cpuref, p, seed, m=16, base=0):
    """m = m' = 16 over 30-bit moduli, one per level and one for U_0: the model alone decrypts correctly there (the
    product's noise is about n (p n)^2 < 2^20 against moduli of 2^30 and more)"""
    e = p.bit_length() - 1
    g = lm.good_qs(m, 2 ** 29)
    moduli = [next(g) for _ in range(e + 1)]
    L = ptr.Ladder(lambda pps, qs: sm.CpuEngine(cpuref, Params(pps, qs)), cpuref, m, m, moduli, p, base,
                   np.random.default_rng(seed))
    L.keygen()
    return L, L.round_hints()


@pytest.mark.parametrize("p", [4, 8, 16])
def test_model_rounds_every_constant(cpuref, p):
    """0110, 00111100, 0000111111110000: msb(c + p/4)"""
    L, hints = _ladder(cpuref, p, seed=p)
    pt = np.zeros((p, L.ez[0].n), dtype=np.int64)
    pt[:, 0] = np.arange(p)
    out = ptr.pt_round(L, hints, ptr.encrypt(L, pt))
    want = [(c + p // 4) // (p // 2) % 2 for c in range(p)]
    assert want == {4: [0, 1, 1, 0], 8: [0, 0, 1, 1, 1, 1, 0, 0], 16: [0] * 4 + [1] * 8 + [0] * 4}[p]
    assert [int(ptr.closed_form(c, p)) for c in range(p)] == want
    assert out["enc"] == "MSD" and out["k"] == 2 ** (L.e - 1) - 1 and len(out["c"]) == 2
    assert out["c"][0].shape == (p, L.ez[0].n, 1)
    dec = ptr.decrypt(L, out)
    assert dec[:, 0].tolist() == want and not dec[:, 1:].any()


def test_model_identity_at_p_2(cpuref):
    L, hints = _ladder(cpuref, 2, seed=2)
    assert hints == []
    ct = ptr.encrypt(L, np.array([[1, 0, 1, 1, 0, 0, 0, 1]], dtype=np.int64))
    assert ptr.pt_round(L, hints, ct) is ct


@pytest.mark.parametrize("base", [0, 4])
def test_model_on_random_plaintexts_at_p_8(cpuref, base):
    """x = c + 4 r, c a constant of [0, 4) and r random in R_2: the plaintexts on which every modSwitchPT of the tree
    halves exactly (x (x + 1) is even because x mod 2 is 0 or 1; the pair product is even because (x mod 4) / 2 is), so
    the tree on plaintexts is well defined; it is run with exact negacyclic arithmetic mod p_i"""
    p = 8
    L, hints = _ladder(cpuref, p, seed=80 + base, base=base)
    rng = np.random.default_rng(8)
    n = L.ez[0].n
    pt = (rng.integers(0, 4, size=(12, 1)) * (np.arange(n) == 0) + 4 * rng.integers(0, 2, size=(12, n))).astype(np.int64) % p
    assert (pt[:, 1:] != 0).any()
    want = np.stack([ptr.pt_recursion(x, p, pr.negacyclic) for x in pt]).astype(np.int64)
    assert want.any() and (want[:, 1:] != 0).any()
    dec = ptr.decrypt(L, ptr.pt_round(L, hints, ptr.encrypt(L, pt)))
    assert np.array_equal(dec, want)


# ---- statuses -------------------------------------------------------------------------------------------------------------
def _host_ladder(lolhip, e, m=16, T_extra=0, bits=30):
    g = lm.good_qs(m, 2 ** (bits - 1))
    qs = [next(g) for _ in range(e + 1 + T_extra)]
    mk = lambda q: lolhip.Plan.for_index(m, q, host_only=True)
    return qs, [mk(qs[i + 1:]) for i in range(e)], [mk(qs[i:]) for i in range(e - 1)], mk


def test_ct_affine_mul_statuses(lolhip):
    L = lolhip.lib()
    qs, lv, _, mk = _host_ladder(lolhip, 2)
    pq = lv[0]
    B = 2
    a = np.zeros((2, B, pq.n, pq.T), dtype=np.int64)
    out = np.full((2, 3, B, pq.n, pq.T), SENT, dtype=np.int64)
    one = (C.c_int64 * pq.T)(*([1] * pq.T))
    P = lambda x: None if x is None else x.ctypes.data

    def call(h=pq, a_=a, al=one, b_=a, be=one, np_=1, o=out, Bn=B):
        return L.lolhip_ct_affine_mul_batch(None if h is None else h._h, None, P(a_), al, None, P(b_), be, None, np_, P(o), Bn)

    assert call() == NO_DEVICE
    for kw in (dict(h=None), dict(a_=None), dict(b_=None), dict(o=None), dict(al=None), dict(be=None), dict(np_=0),
               dict(np_=65536), dict(Bn=-1), dict(np_=2, o=a)):
        assert call(**kw) == INVALID, kw
    assert call(np_=1, o=a) == NO_DEVICE                          # one pair: out may be a
    assert call(np_=2) == NO_DEVICE
    g = lm.good_qs(16, 2 ** 20)
    assert call(h=mk([next(g) for _ in range(17)])) == INVALID
    assert call(h=mk([2 ** 20, 2 ** 21 + 1])) == NO_CRT
    assert call(Bn=0, a_=None, b_=None, o=None) == NO_DEVICE
    assert (out == SENT).all()
    # the Python method raises the same codes before it stages anything
    for plan, kw, code in ((pq, {}, NO_DEVICE), (pq, dict(npairs=0), INVALID), (mk([2 ** 20, 2 ** 21 + 1]), {}, NO_CRT)):
        with pytest.raises(lolhip.LolHipError) as e:
            plan.ctAffineMul(a, 1, **kw)
        assert e.value.code == code


def test_ptround_statuses_and_work_len(lolhip):
    L = lolhip.lib()
    e, p = 3, 8
    qs, lv, up, mk = _host_ladder(lolhip, e)
    pp = mk([p])
    vp = lambda vals: (C.c_void_p * max(len(vals), 1))(*[None if v is None else (v if isinstance(v, int) else v._h) for v in vals])
    fake = [8, 8]                                                 # borrowed device pointers: only stored by create

    def create(e=e, p=p, lv=lv, up=up, hints=fake, base=2, pp=pp, x0=None, x1=None, ok_out=True):
        h = C.c_void_p()
        rc = L.lolhip_ptround_create(e, p, vp(lv), vp(up), vp(hints), base, None if pp is None else pp._h,
                                     None if x0 is None else x0._h, None if x1 is None else x1._h,
                                     C.byref(h) if ok_out else None)
        assert (h.value is None) == (rc != 0)
        return rc, h

    rc, h = create()
    assert rc == 0
    # work_len: the formula of the header
    n, T0 = lv[0].n, 3
    ev = lambda x: x + (x & 1)
    Lmax = max(u.decomposeLen(2) for u in up)
    for B in (1, 5):
        N, Tu, np1, nc = B * n, T0 + 1, p // 8, p // 4 + 1
        want = (ev(max(3 * N * T0, 3 * np1 * N * (T0 - 1))) + 2 * ev(max(2 * N * T0, 2 * np1 * N * (T0 - 2))) + ev(3 * N * Tu)
                + ev(2 * N * Tu) + ev(Lmax * N * Tu) + ev(max(3 * N * T0, 2 * N * Tu)) + ev(nc * n * T0) + ev(nc * n * T0)
                + ev(nc * n) + ev(n * T0))
        assert L.lolhip_ptround_work_len(h, B) == want
    assert L.lolhip_ptround_work_len(h, 0) == 0
    assert L.lolhip_ptround_work_len(h, -1) == INVALID and L.lolhip_ptround_work_len(None, 1) == INVALID
    B = 2
    cs = np.zeros((2, B, n, T0), dtype=np.int64)
    out = np.full((2, B, n, 1), SENT, dtype=np.int64)
    work = np.zeros(L.lolhip_ptround_work_len(h, B), dtype=np.int64)
    ko, lo = C.c_int64(SENT), C.c_int64(SENT)

    def batch(hh=h, c=cs, crt=0, enc=1, k=0, l=1, o=out, ocrt=0, kout=True, lout=True, w=work, Bn=B):
        return L.lolhip_ptround_batch(hh, None, None if c is None else c.ctypes.data, crt, enc, k, l,
                                      None if o is None else o.ctypes.data, ocrt, C.byref(ko) if kout else None,
                                      C.byref(lo) if lout else None, None if w is None else w.ctypes.data, Bn)

    assert batch() == NO_DEVICE and batch(enc=0) == NO_DEVICE and batch(l=5, k=2) == NO_DEVICE
    for kw in (dict(hh=None), dict(c=None), dict(o=None), dict(w=None), dict(kout=False), dict(lout=False), dict(Bn=-1),
               dict(enc=2), dict(enc=-1), dict(k=-1)):
        assert batch(**kw) == INVALID, kw
    for l in (0, 2, 4, 6, 8):
        assert batch(l=l) == MODULUS, l                           # l has no inverse mod 8
    assert batch(Bn=0, c=None, o=None, w=None) == NO_DEVICE
    assert (out == SENT).all() and ko.value == SENT and lo.value == SENT
    L.lolhip_ptround_destroy(h)
    # the Python class raises the same codes before it stages anything
    rnd = lolhip.PTRound(lv, up, fake, 2, p, pp_m=pp)
    for l, code in ((1, NO_DEVICE), (2, MODULUS)):
        with pytest.raises(lolhip.LolHipError) as e:
            rnd(cs, l=l)
        assert e.value.code == code
    # create
    assert create(e=0)[0] == INVALID and create(e=17)[0] == INVALID and create(ok_out=False)[0] == INVALID
    assert create(lv=[lv[0], None, lv[2]])[0] == INVALID and create(up=[up[0], None])[0] == INVALID
    assert create(hints=[8, 0])[0] == INVALID and create(pp=None)[0] == INVALID and create(base=1)[0] == INVALID
    assert create(lv=[lv[0], lv[2], lv[2]])[0] == INVALID         # not ZqDown
    assert create(lv=[lv[0], lv[1], lv[1]])[0] == INVALID
    assert create(up=[up[1], up[1]])[0] == INVALID                # not ZqUp of Z_0
    assert create(up=[up[0], lv[1]])[0] == INVALID                # U_1 = Z_1: no modulus in front
    alt = mk([qs[0]] + qs[2:])
    rc, h2 = create(up=[up[0], alt])                              # any modulus may stand in front
    assert rc == 0
    L.lolhip_ptround_destroy(h2)
    other = lolhip.Plan.for_index(32, qs[2:], host_only=True)
    assert create(lv=[lv[0], other, lv[2]])[0] == INVALID         # another index
    assert create(up=[lolhip.Plan.for_index(32, qs, host_only=True), up[1]])[0] == INVALID
    assert create(pp=mk([16]))[0] == INVALID                      # pp_m not over p
    assert create(pp=lolhip.Plan.for_index(8, [p], host_only=True))[0] == INVALID      # pp_m not of index m
    assert create(pp=mk([p, qs[0]]))[0] == INVALID
    g = lm.good_qs(16, 2 ** 20)
    many = [next(g) for _ in range(18)]
    big_lv, big_up = [mk(many[i + 1:]) for i in range(3)], [mk(many[i:]) for i in range(2)]
    assert create(lv=big_lv, up=big_up)[0] == INVALID             # T > 16
    assert create(p=16, pp=mk([16]))[0] == MODULUS and create(p=6, pp=mk([6]))[0] == MODULUS          # p is not 2^e
    assert create(e=2, p=8, lv=lv[:2], up=up[:1])[0] == MODULUS
    ev_qs = [qs[0], qs[1], 2 ** 20, qs[3]]
    ev_lv, ev_up = [mk(ev_qs[i + 1:]) for i in range(3)], [mk(ev_qs[i:]) for i in range(2)]
    assert create(lv=ev_lv, up=ev_up)[0] == MODULUS               # an even modulus: gcd(Q, 2) != 1
    nc_qs = [qs[0], qs[1], qs[2], 2 ** 21 + 1]
    nc_lv, nc_up = [mk(nc_qs[i + 1:]) for i in range(3)], [mk(nc_qs[i:]) for i in range(2)]
    assert create(lv=nc_lv, up=nc_up)[0] == NO_CRT
    # exts: m = 8 under m' = 16
    lo0, lo1 = (lolhip.Plan.for_index(8, q, host_only=True) for q in (qs[1:], qs[2:]))
    x0, x1 = lolhip.Ext(lo0, lv[0]), lolhip.Ext(lo1, lv[1])
    pp8 = lolhip.Plan.for_index(8, [p], host_only=True)
    rc, hx = create(pp=pp8, x0=x0, x1=x1)
    assert rc == 0 and batch(hh=hx) == NO_DEVICE
    L.lolhip_ptround_destroy(hx)
    assert create(pp=pp8, x0=x0)[0] == INVALID and create(pp=pp8, x1=x1)[0] == INVALID
    assert create(pp=pp8, x0=x1, x1=x0)[0] == INVALID             # exts that do not end in p_lvl[0] / p_lvl[1]
    assert create(pp=pp, x0=x0, x1=x1)[0] == INVALID              # pp_m of index m', not m
    # e = 1: the identity needs no up plans, hints or pp_m
    rc, h1 = create(e=1, p=2, lv=lv[2:], up=[], hints=[], pp=None)
    assert rc == 0 and L.lolhip_ptround_work_len(h1, 7) == 0
    assert batch(hh=h1, w=None) == NO_DEVICE and batch(hh=h1, c=None) == INVALID
    L.lolhip_ptround_destroy(h1)
    L.lolhip_ptround_destroy(None)
    assert (out == SENT).all() and ko.value == SENT and lo.value == SENT


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def test_cross_term_bound_and_metadata_arithmetic():
    """k_ct_affine_mul keeps A0 B1 + A1 B0 in 128 bits and reduces once: the 2-by-1 division step needs the high word below
    q.  With canonical operands the sum is at most 2 (q - 1)^2 < 2^125 for q < 2^62, and its high word is below q.  Then
    the k / l recursions of ptRound in Python integers."""
    q = 2 ** 62 - 57
    worst = 2 * (q - 1) ** 2
    assert worst < 2 ** 128 and worst >> 64 < q
    assert 2 * (2 ** 62 - 1) ** 2 >> 64 < 2 ** 62 - 1
    # alpha x + v stays canonical: [0, 2q) trimmed, then one modular addition of two canonical values
    assert 2 * q < 2 ** 64 and (q - 1) + (q - 1) < 2 ** 64
    # k: each product gives k_a + k_b + 1
    for e in range(1, 17):
        for k in (0, 1, 5):
            kk = k
            for _ in range(e - 1):
                kk = 2 * kk + 1
            assert kk == 2 ** (e - 1) * (k + 1) - 1
    # l: toLSD then toMSD over one modulus list is the identity on l (zp_L zp_M = 1 mod p), and reduce . lift into p / 2 is
    # l mod p / 2 because p / 2 divides p
    Q = q * (2 ** 61 - 1)
    for p in (4, 8, 16, 2 ** 16):
        zpm = -Q % p
        zpl = pow(zpm, -1, p)
        assert zpm * zpl % p == 1
        for l in range(1, p, 2):
            dec = l - p if 2 * l >= p else l
            assert dec % (p // 2) == l % (p // 2)
