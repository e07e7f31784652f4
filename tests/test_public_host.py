"""Host side of the SymmSHE public operations and ciphertext addition (include/lolhip.h lolhip_encode_scales,
lolhip_ct_lincomb_batch, lolhip_add_public_batch, lolhip_mul_public_batch): no GPU needed.

 - the new entries are exported and declared;
 - encode_scales equals a big-integer derivation of lsdToMSD / msdToLSD for T = 1..16;
 - work lengths, and every status of the compute entries on host-only plans, the outputs untouched;
 - the restatement of tests/public_ref.py against decryption in the CPU SHE model (oracle/she_model.py): pt + b, a pt,
   -pt, pt1 + pt2 after the reference's alignment, and modSwitchPT.
"""
import ctypes as C
import os
import re
from math import gcd, prod

import numpy as np
import pytest

import public_ref as pr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_encode_scales", "lolhip_ct_lincomb_batch", "lolhip_public_work_len", "lolhip_add_public_batch",
       "lolhip_mul_public_batch")
INVALID, MODULUS, NO_CRT, NO_DEVICE = -1, -2, -3, -5
SENT = 0x5A5A5A5A


def test_public_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"
    for nm in ("encodeScales", "ctLinComb", "toMSD", "toLSD", "mulScalar", "ctNegate", "ctAdd", "addPublic", "mulPublic",
               "modSwitchPT", "mulGCT", "absorbGFactors"):
        assert callable(getattr(lolhip.Plan, nm))


def _moduli(m, bits, T):
    g = lm.good_qs(m, 2 ** (bits - 1))
    return [next(g) for _ in range(T)]


@pytest.mark.parametrize("T", list(range(1, 17)))
def test_encode_scales_equal_big_integer_derivation(lolhip, T):
    qs = _moduli(16, (20, 30, 59, 61)[T % 4], T)
    P = lolhip.Plan([(2, 4)], qs, host_only=True)
    Q = prod(qs)
    for p in (2, 3, 8, 16, 257, 65537, 2 ** 61 - 1):
        zq, zp = P.encodeScales(p, True)
        assert zq == [pow(p, -1, q) for q in qs] and zp == (-Q) % p
        assert (zq, zp) == pr.encode_scales(qs, p, True)
        if gcd(Q, p) == 1:
            zq, zp = P.encodeScales(p, False)
            assert zq == [p % q for q in qs] and zp == pow((-Q) % p, -1, p)
            assert (zq, zp) == pr.encode_scales(qs, p, False)
            assert ((-Q) % p) * zp % p == 1
    L = lolhip.lib()
    zq = np.full(T, SENT, dtype=np.int64)
    zp = C.c_int64(SENT)
    for p in (1, 0, -5, 2 ** 62):
        assert L.lolhip_encode_scales(P._h, p, 1, zq.ctypes.data_as(lolhip.tensor._i64p), C.byref(zp)) == MODULUS
    assert L.lolhip_encode_scales(P._h, 3, 2, zq.ctypes.data_as(lolhip.tensor._i64p), C.byref(zp)) == INVALID
    assert L.lolhip_encode_scales(None, 3, 1, zq.ctypes.data_as(lolhip.tensor._i64p), C.byref(zp)) == INVALID
    assert (zq == SENT).all() and zp.value == SENT


def test_encode_scales_refuse_what_has_no_inverse(lolhip):
    qs = [17, 97]                                               # Q = 1649 = 17 * 97
    P = lolhip.Plan([(2, 4)], qs, host_only=True)
    with pytest.raises(lolhip.LolHipError) as e:
        P.encodeScales(17, True)                                # 17 has no inverse mod q_0 = 17
    assert e.value.code == MODULUS
    with pytest.raises(lolhip.LolHipError) as e:
        P.encodeScales(97 * 2, False)                           # gcd(Q, p) = 97: (-Q)^-1 mod p does not exist
    assert e.value.code == MODULUS


def test_public_work_len(lolhip):
    L = lolhip.lib()
    qs = [lm.first_good_q(1024, 2 ** 30)]
    hi = lolhip.Plan.for_index(1024, qs, host_only=True)
    lo = lolhip.Plan.for_index(16, qs, host_only=True)
    x = lolhip.Ext(lo, hi)
    for B in (0, 1, 7, 4096):
        assert L.lolhip_public_work_len(hi._h, None, B) == B * hi.n * 2
        assert L.lolhip_public_work_len(hi._h, x._h, B) == B * lo.n * 2
    assert L.lolhip_public_work_len(hi._h, None, -1) == INVALID
    assert L.lolhip_public_work_len(None, None, 1) == INVALID
    other = lolhip.Plan.for_index(2048, [lm.first_good_q(2048, 2 ** 30)], host_only=True)
    assert L.lolhip_public_work_len(other._h, x._h, 1) == INVALID          # x does not end in other's ring


def _args():
    """host-only plans: (hi, lo, ext, pp_m, pq without a CRT basis, its ext)"""
    import lol_amd
    qs = lm.good_qs(1024, 2 ** 30)
    qs = [next(qs), next(qs)]
    hi = lol_amd.Plan.for_index(1024, qs, host_only=True)
    lo = lol_amd.Plan.for_index(16, qs, host_only=True)
    ncrt = lol_amd.Plan.for_index(1024, [2 ** 20, 2 ** 21 + 1], host_only=True)
    nlo = lol_amd.Plan.for_index(16, [2 ** 20, 2 ** 21 + 1], host_only=True)
    return hi, lo, lol_amd.Ext(lo, hi), lol_amd.Plan.for_index(16, [8], host_only=True), ncrt, lol_amd.Ext(nlo, ncrt)


def test_every_status_on_host_only_plans(lolhip):
    L = lolhip.lib()
    hi, lo, x, pp, ncrt, nx = _args()
    B, ncs = 2, 2
    cs = np.zeros((ncs, B, hi.n, hi.T), dtype=np.int64)
    out = np.full_like(cs, SENT)
    work = np.zeros(hi.n * B * 3, dtype=np.int64)
    pub = np.zeros((B, hi.n), dtype=np.int64)
    lo_out = C.c_int64(SENT)
    P = lambda a: a.ctypes.data

    def add(pq=hi, xq=x, ppm=None, stride=lo.n, ncs=ncs, shared=0, crt=0, enc=0, k=0, l=1, p=8, o=None, lout=True, Bn=B,
            b=pub, c=cs, w=work):
        return L.lolhip_add_public_batch(pq._h if pq else None, xq._h if xq else None, ppm._h if ppm else None, None,
                                         None if b is None else P(b), stride, None if c is None else P(c), ncs, shared, crt,
                                         enc, k, l, p, P(out) if o is None else o, C.byref(lo_out) if lout else None,
                                         None if w is None else P(w), Bn)

    def mul(pq=hi, xq=x, stride=lo.n, ncs=ncs, shared=0, p=8, o=None, Bn=B, a=pub, c=cs, w=work):
        return L.lolhip_mul_public_batch(pq._h if pq else None, xq._h if xq else None, None, None if a is None else P(a),
                                         stride, p, None if c is None else P(c), ncs, shared, P(out) if o is None else o,
                                         None if w is None else P(w), Bn)

    for f in (add, mul):
        assert f(pq=None) == INVALID
        assert f(ncs=0) == INVALID
        assert f(Bn=-1) == INVALID
        assert f(xq=nx) == INVALID                               # x does not end in pq's ring and moduli
        assert f(stride=lo.n - 1) == INVALID and f(stride=-1) == INVALID
        assert f(c=None) == INVALID and f(w=None) == INVALID
        assert f(shared=1, o=P(cs)) == INVALID                   # out = a shared ciphertext with B > 1
        assert f(p=1) in (MODULUS,) and f(p=2 ** 62) == MODULUS
        assert f() == NO_DEVICE and f(stride=0) == NO_DEVICE and f(Bn=0) == NO_DEVICE
    assert add(b=None) == INVALID and mul(a=None) == INVALID
    assert add(lout=False) == INVALID
    assert add(enc=2) == INVALID and add(k=-1) == INVALID
    assert add(k=1) == INVALID                                   # pp_m missing
    assert add(k=1, ppm=hi) == INVALID                           # not of index m over p alone
    assert add(k=1, ppm=pp, p=16) == INVALID                     # pp_m's modulus is not p
    assert add(k=1, ppm=pp) == NO_DEVICE
    assert add(l=2) == MODULUS and add(l=0) == MODULUS           # l not invertible mod 8
    assert add(l=3) == NO_DEVICE and add(l=-1) == NO_DEVICE
    Q = prod(hi.qs)
    assert add(enc=1, p=hi.qs[0]) == MODULUS                     # gcd(Q, p) != 1
    assert add(enc=1, p=Q % 1000003 and 1000003) == NO_DEVICE
    assert add(pq=ncrt, xq=nx, crt=1) == NO_CRT and mul(pq=ncrt, xq=nx) == NO_CRT
    assert add(pq=ncrt, xq=nx, crt=0) == NO_DEVICE
    assert add(crt=1) == NO_DEVICE
    # lincomb
    al = (C.c_int64 * hi.T)(1, 2)

    def lc(pq=hi, na=2, nb=0, b=None, beta=None, alpha=al, Bn=B, a=cs, o=None):
        return L.lolhip_ct_lincomb_batch(pq._h if pq else None, None, None if a is None else P(a), na, alpha,
                                         None if b is None else P(b), nb, beta, P(out) if o is None else o, Bn)
    assert lc(pq=None) == INVALID and lc(na=0) == INVALID and lc(nb=-1) == INVALID and lc(Bn=-1) == INVALID
    assert lc(alpha=None) == INVALID and lc(nb=1) == INVALID and lc(nb=1, b=cs) == INVALID and lc(b=cs) == INVALID
    assert lc(a=None) == INVALID
    assert lc() == NO_DEVICE and lc(nb=2, b=cs, beta=al) == NO_DEVICE
    assert (out == SENT).all() and lo_out.value == SENT
    # the Python layer runs the same checks first
    with pytest.raises(lolhip.NoDeviceError):
        hi.addPublic(pub[:, :lo.n], cs, 8, ext=x)
    with pytest.raises(lolhip.NoDeviceError):
        hi.mulPublic(pub[0, :lo.n], cs, 8, ext=x)
    with pytest.raises(lolhip.NoDeviceError):
        hi.ctNegate(cs)


# ---------------------------------------------------------------------------------------------
# the restatement against decryption in the CPU SHE model
# ---------------------------------------------------------------------------------------------
def _she(cpuref, m, p, lower, T, seed):
    pps = lm.factor_pps(m)
    g = lm.good_qs(m, lower)
    qs = [next(g) for _ in range(T)]
    rng = np.random.default_rng(seed)
    P = Params(pps, qs)
    she = sm.SHE(sm.CpuEngine(cpuref, P), sm.CpuEngine(cpuref, pr.params(m, [p])), qs, p, rng)
    she.keygen()
    return she, P, rng


def _pt(rng, B, n, p):
    pt = rng.integers(0, p, size=(B, n), dtype=np.int64)
    pt[0, :4] = [p // 2, p // 2 - 1, p - 1, 0]
    return pt


@pytest.mark.parametrize("m,p", [(64, 257), (64, 16), (45, 181)])
@pytest.mark.parametrize("msd,k", [(False, 0), (True, 0), (True, 1), (False, 2)])
def test_add_public_decrypts_to_the_sum(cpuref, m, p, msd, k):
    she, P, rng = _she(cpuref, m, p, 2 ** 29, 2, 100 + m + p + k)
    B = 2
    pt = _pt(rng, B, P.n, p)
    ct = she.encrypt(pt)
    for _ in range(k):
        ct = pr.mul_gct(cpuref, P, ct)
    if msd:
        ct = she.toMSD(ct)
    assert np.array_equal(she.decrypt(ct), pt)
    b = rng.integers(-2 ** 62, 2 ** 62, size=(B, P.n), dtype=np.int64)
    b[0, :3] = [p // 2, -1, p + 3]
    got = pr.add_public(cpuref, P, None, b, dict(ct, c=np.stack(ct["c"])), p, B)
    assert got["enc"] == "LSD" and got["k"] == k
    assert np.array_equal(she.decrypt(dict(got, c=list(got["c"]))), (pt + b) % p)


def test_mul_public_negate_and_scalar_decrypt(cpuref):
    m, p = 64, 257
    she, P, rng = _she(cpuref, m, p, 2 ** 29, 2, 7)
    B = 2
    pt = _pt(rng, B, P.n, p)
    ct = she.toMSD(she.encrypt(pt))
    a = np.zeros((B, P.n), dtype=np.int64)
    a[:, 0] = [3, p - 2]                                          # small public values keep the noise small
    a[1, 5] = p // 2 + 1
    crt = dict(ct, c=np.stack([cpuref.crt(P, c).reshape(c.shape) for c in ct["c"]]), crt=True)
    got = pr.mul_public(cpuref, P, None, a, crt, p, B)
    back = dict(got, c=[cpuref.crtinv(P, c).reshape(c.shape) for c in got["c"]])
    want = np.stack([pr.negacyclic(pt[i], pr.decode(a[i], p), p) for i in range(B)]).astype(np.int64)
    assert np.array_equal(she.decrypt(back), want)
    neg = pr.negate(dict(ct, c=np.stack(ct["c"])), P.qs)
    assert np.array_equal(she.decrypt(dict(neg, c=list(neg["c"]))), (-pt) % p)
    sc = pr.mul_scalar(dict(ct, c=np.stack(ct["c"])), P.qs, p - 3, p)
    assert np.array_equal(she.decrypt(dict(sc, c=list(sc["c"]))), (-3 * pt) % p)


@pytest.mark.parametrize("m,p", [(45, 181), (64, 16)])
def test_ct_add_aligns_l_k_and_encoding(cpuref, m, p):
    she, P, rng = _she(cpuref, m, p, 2 ** 29, 2, 11 + m)
    B = 2
    pt1, pt2 = _pt(rng, B, P.n, p), _pt(rng, B, P.n, p)
    c1 = she.toMSD(she.encrypt(pt1))                             # MSD, k 0, l = -Q mod p
    c2 = pr.mul_gct(cpuref, P, she.encrypt(pt2))                 # LSD, k 1, l 1
    c2 = dict(c2, c=np.stack(c2["c"]))
    s = pr.ct_add(cpuref, P, dict(c1, c=np.stack(c1["c"])), c2, p)
    assert s["k"] == 1 and s["enc"] == "MSD"
    assert np.array_equal(she.decrypt(dict(s, c=list(s["c"]))), (pt1 + pt2) % p)
    # a three-component ciphertext plus a two-component one: the shorter is padded with zeros
    prod_ = she.mul(she.encrypt(pt1), she.encrypt(pt2))
    s = pr.ct_add(cpuref, P, dict(prod_, c=np.stack(prod_["c"])), dict(c1, c=np.stack(c1["c"])), p)
    assert len(s["c"]) == 3
    want = she.decrypt(prod_)
    assert np.array_equal(she.decrypt(dict(s, c=list(s["c"]))), (want + pt1) % p)


def test_mod_switch_pt_decrypts_under_the_smaller_modulus(cpuref):
    """p = 16 -> p' = 8 on multiples of p / p': MSD keeps the plaintext in the top digits"""
    m, p, p2 = 64, 16, 8
    she, P, rng = _she(cpuref, m, p, 2 ** 29, 2, 5)
    B = 2
    x = rng.integers(0, p2, size=(B, P.n), dtype=np.int64)
    ct = she.encrypt((p // p2) * x)
    got = pr.mod_switch_pt(dict(ct, c=np.stack(ct["c"])), P.qs, p, p2)
    assert got["enc"] == "MSD"
    she2 = sm.SHE(she.e, sm.CpuEngine(cpuref, pr.params(m, [p2])), P.qs, p2, rng)
    she2.s, she2.s_crt = she.s, she.s_crt
    assert np.array_equal(she2.decrypt(dict(got, c=list(got["c"]))), x)
