"""The SymmSHE public operations and ciphertext addition on the GPU (lolhip_ct_lincomb_batch, lolhip_add_public_batch,
lolhip_mul_public_batch), against the CPU restatement of tests/public_ref.py and through lolhip_decrypt_batch.

    parity        bit-exact at m = m' = 2^11 (p = 257, 16), 16 in 1024 / 2048 (p = 8), 128 in 11648 (ZQ4), 15 in 45 and
                  45 (k = 1, 2), 61-bit T = 3 at 2^12, T = 16: both bases, LSD and MSD input, shared and per-item
                  operands, boundary public values, out aliasing the ciphertext
    decryption    device key and ciphertexts: addPublic, mulPublic, mulScalar, negate, (+), modSwitchPT, absorbGFactors
    HomomPRF      mulPublic of KHPRF.lifted's A_T(x)_0 (stride L n) on one encryption of s at m' = 11648
    errors        statuses leave the output untouched; a side stream
"""
import numpy as np
import pytest

import khprf_lifted_ref as klr
import public_ref as pr
from oracle import lolmath as lm
from oracle.oracle import Params

pytestmark = pytest.mark.gpu

ZQ4 = [25159681, 19918081, 19393921, 18869761]


def _moduli(m, bits, T):
    g = lm.good_qs(m, 2 ** (bits - 1))
    return [next(g) for _ in range(T)]


# (m, m', qs, p, ks)
SHAPES = [
    (2048, 2048, _moduli(2048, 30, 2), 257, (0,)),
    (2048, 2048, _moduli(2048, 30, 2), 16, (0,)),
    (16, 1024, _moduli(1024, 30, 2), 8, (0,)),
    (16, 2048, _moduli(2048, 30, 2), 8, (0,)),
    (128, 11648, ZQ4, 8, (0,)),
    (15, 45, _moduli(45, 30, 2), 181, (1, 2)),
    (45, 45, _moduli(45, 30, 2), 16, (1, 2)),
    (4096, 4096, _moduli(4096, 61, 3), 257, (0,)),
    (64, 64, _moduli(64, 30, 16), 257, (0,)),
]
IDS = [f"{m}in{m2}-T{len(qs)}-p{p}" for m, m2, qs, p, _ in SHAPES]


def _setup(gpu, m, m2, qs):
    hi = gpu.Plan.for_index(m2, qs)
    P_hi = Params(lm.factor_pps(m2), qs)
    if m == m2:
        return hi, None, None, P_hi, None
    lo = gpu.Plan.for_index(m, qs)
    return hi, lo, gpu.Ext(lo, hi), P_hi, Params(lm.factor_pps(m), qs)


def _public(rng, B, n, p):
    v = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, n), dtype=np.int64, endpoint=True)
    edge = [p // 2, p // 2 - 1, p - 1, -1, -(p // 2), p, p + p // 2, 2 ** 63 - 1, -2 ** 63, 0]
    v[0, :min(n, len(edge))] = edge[:n]
    if B > 1:
        v[1] = rng.integers(-3 * p, 3 * p, size=n)
    return v


def _cs(rng, qs, ncs, B, n):
    c = np.stack([rng.integers(0, q, size=(ncs, B, n), dtype=np.int64) for q in qs], axis=-1)
    neg = rng.integers(0, 2, size=c.shape).astype(bool) & (c > 0)
    return np.ascontiguousarray(np.where(neg, c - np.array(qs, dtype=np.int64), c))     # some in (-q, 0)


def _canon(c, qs):
    return np.ascontiguousarray((np.asarray(c).astype(object) % np.array(qs, dtype=object)).astype(np.int64))


@pytest.mark.parametrize("m,m2,qs,p,ks", SHAPES, ids=IDS)
def test_add_public_parity(gpu, cpuref, m, m2, qs, p, ks):
    import torch
    hi, lo, x, P_hi, P_lo = _setup(gpu, m, m2, qs)
    pp_m = gpu.Plan.for_index(m, [p])
    rng = np.random.default_rng(m + m2 + p)
    B, ncs = 3, 2
    n_m = hi.n if lo is None else lo.n
    combos = [(False, 0, False, False, False), (True, 1, True, True, False), (True, 0, False, True, True),
              (False, 1, True, False, False)]
    for k in ks:
        for crt, enc, cs_shared, b_shared, alias in combos:
            if crt and not hi.has_crt:
                continue
            cs = _cs(rng, qs, ncs, 1 if cs_shared else B, hi.n)
            b = _public(rng, 1 if b_shared else B, n_m, p)
            l = int(rng.integers(1, p))
            while np.gcd(l, p) != 1:
                l += 1
            ct = {"enc": ("LSD", "MSD")[enc], "k": k, "l": l, "c": cs, "crt": crt}
            want = pr.add_public(cpuref, P_hi, P_lo, b, ct, p, B)
            dcs = torch.from_numpy(cs).cuda()
            db = torch.from_numpy(b[0] if b_shared else b).cuda()
            kw = dict(pp_m=pp_m, ext=x, enc=enc, k=k, l=l, cs_crt=crt, cs_shared=cs_shared, B=B)
            if alias:
                import ctypes as C
                L = gpu.lib()
                lo_out = C.c_int64(0)
                work = torch.empty((L.lolhip_public_work_len(hi._h, None if x is None else x._h, B),), dtype=torch.int64,
                                   device="cuda")
                rc = L.lolhip_add_public_batch(hi._h, None if x is None else x._h, pp_m._h, None, db.data_ptr(),
                                               0 if b_shared else n_m,
                                               dcs.data_ptr(), ncs, 0, int(crt), enc, k, l, p, dcs.data_ptr(),
                                               C.byref(lo_out), work.data_ptr(), B)
                assert rc == 0
                got, l_out = dcs.cpu().numpy(), int(lo_out.value)
            else:
                got, enc_out, l_out = hi.addPublic(db, dcs, p, **kw)
                assert enc_out == "LSD"
                got = got.cpu().numpy()
            assert l_out == want["l"]
            assert np.array_equal(got, want["c"]), (k, crt, enc, cs_shared, b_shared, alias)


@pytest.mark.parametrize("m,m2,qs,p,ks", SHAPES, ids=IDS)
def test_mul_public_and_lincomb_parity(gpu, cpuref, m, m2, qs, p, ks):
    import torch
    hi, lo, x, P_hi, P_lo = _setup(gpu, m, m2, qs)
    rng = np.random.default_rng(7 * m + m2 + p)
    B, ncs = 3, 3
    n_m = hi.n if lo is None else lo.n
    for cs_shared, a_shared, alias in ((False, False, False), (True, True, False), (False, True, True), (True, False, False)):
        cs = _cs(rng, qs, ncs, 1 if cs_shared else B, hi.n)
        a = _public(rng, 1 if a_shared else B, n_m, p)
        want = pr.mul_public(cpuref, P_hi, P_lo, a, {"c": cs}, p, B)["c"]
        dcs = torch.from_numpy(cs).cuda()
        da = torch.from_numpy(a[0] if a_shared else a).cuda()
        got = hi.mulPublic(da, dcs, p, ext=x, cs_shared=cs_shared, B=B, out=dcs if alias else None)
        if alias:
            assert got.data_ptr() == dcs.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want), (cs_shared, a_shared, alias)
    # the linear combinations: toMSD, toLSD, mulScalar, negate, subtraction with unequal lengths, out aliasing b
    c1, c2 = _cs(rng, qs, 3, B, hi.n), _cs(rng, qs, 2, B, hi.n)
    for pp in (p, 3):
        for f, g in ((lambda c: hi.toMSD(c, pp)[0], lambda c: pr.to_msd({"enc": "LSD", "l": 1, "c": c}, qs, pp)["c"]),
                     (lambda c: hi.toLSD(c, pp)[0], lambda c: pr.to_lsd({"enc": "MSD", "l": 1, "c": c}, qs, pp)["c"]),
                     (lambda c: hi.mulScalar(c, pp // 2, pp), lambda c: pr.mul_scalar({"c": c}, qs, pp // 2, pp)["c"]),
                     (lambda c: hi.ctNegate(c), lambda c: pr.negate({"c": c}, qs)["c"])):
            if pp == 3 and any(q % 3 == 0 for q in qs):
                continue
            assert np.array_equal(f(c1), g(c1))
    d1, d2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    out = torch.empty_like(d1)
    hi.ctLinComb(d2, 1, d1, -1, out=out)                                   # c2 - c1: 3 components
    assert np.array_equal(out.cpu().numpy(), pr.lincomb(qs, c2, [1] * len(qs), c1, [-1] * len(qs)))
    hi.ctLinComb(d1, [5] * len(qs), d1, [2 ** 62] * len(qs), out=d1)        # out = a = b
    assert np.array_equal(d1.cpu().numpy(), pr.lincomb(qs, c1, [5] * len(qs), c1, [2 ** 62] * len(qs)))
    # a slab that is not 16-byte aligned takes the scalar kernels
    raw = torch.from_numpy(np.concatenate([[0], c2.reshape(-1)])).cuda()
    view = raw[1:]
    got = hi.ctNegate(view.view(c2.shape))
    assert np.array_equal(got.cpu().numpy(), _canon(-c2, qs))


# ---------------------------------------------------------------------------------------------
# decryption of device-made ciphertexts
# ---------------------------------------------------------------------------------------------
def _she(gpu, m, qs, p, seed):
    pq, pp = gpu.Plan.for_index(m, qs), gpu.Plan.for_index(m, [p])
    z = pq.errorRounded(0.5, B=1, key=bytes([seed]) * 32, ctr=0).cpu().numpy()
    s = np.ascontiguousarray(pq.l(pr.reduce(z, qs)))
    s_crt = np.ascontiguousarray(pq.crt(s))[0]
    return pq, pp, s_crt


@pytest.mark.parametrize("m,p,bits", [(64, 257, 30), (2048, 16, 30), (45, 181, 30)])
def test_decryption_of_every_operation(gpu, cpuref, m, p, bits):
    qs = _moduli(m, bits, 2)
    pq, pp, s_crt = _she(gpu, m, qs, p, m % 251)
    rng = np.random.default_rng(m + p)
    B, key = 3, bytes(range(32))
    pt1 = rng.integers(0, p, size=(B, pq.n), dtype=np.int64)
    pt2 = rng.integers(0, p, size=(B, pq.n), dtype=np.int64)
    ct1 = pq.encrypt(pt1, s_crt, pp, 0.5, key=key, ctr=0)
    ct2 = pq.encrypt(pt2, s_crt, pp, 0.5, key=key, ctr=B)
    dec = lambda cs, enc="LSD", k=0, l=1, crt=False: pq.decrypt(cs, s_crt, pp, enc=enc, k=k, l=l, cs_crt=crt)
    assert np.array_equal(dec(ct1), pt1)
    # addPublic on an MSD ciphertext with k = 1
    c, k = pq.mulGCT(ct1, 0)
    c, enc, l = pq.toMSD(c, p)
    b = rng.integers(-1000, 1000, size=(B, pq.n), dtype=np.int64)
    c2, enc2, l2 = pq.addPublic(b, c, p, pp_m=pp, enc=enc, k=k, l=l)
    assert np.array_equal(dec(c2, enc2, k, l2), (pt1 + b) % p)
    # mulPublic, CRT basis: a small public value
    a = np.zeros((B, pq.n), dtype=np.int64)
    a[:, 0] = [2, p - 1, p // 2]
    cc = np.stack([pq.crt(x) for x in ct1])
    got = dec(pq.mulPublic(a, cc, p), crt=True)
    want = np.stack([np.asarray(pp.polymul(pt1[i].reshape(1, -1, 1), (a[i] % p).reshape(1, -1, 1))).reshape(-1)
                     for i in range(B)]) if pp.has_crt else None
    if want is not None:
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(got, np.stack([pr.negacyclic(pt1[i], pr.decode(a[i], p), p) for i in range(B)]))
    # mulScalar, negate, (+) with alignment, modSwitchPT
    assert np.array_equal(dec(pq.mulScalar(ct1, p - 2, p)), (-2 * pt1) % p)
    assert np.array_equal(dec(pq.ctNegate(ct1)), (-pt1) % p)
    m1, e1, l1 = pq.toMSD(ct1, p)
    g2, k2 = pq.mulGCT(ct2, 0)
    s, es, ks, ls = pq.ctAdd((m1, e1, 0, l1), (g2, "LSD", k2, 1), p)
    assert (es, ks) == ("MSD", 1)
    assert np.array_equal(dec(s, es, ks, ls), (pt1 + pt2) % p)
    if p % 2 == 0:
        p2 = p // 2
        c0 = pq.encrypt(2 * (pt1 % p2), s_crt, pp, 0.5, key=key, ctr=2 * B)
        cs, e, l = pq.modSwitchPT(c0, p, p2)
        pp2 = gpu.Plan.for_index(m, [p2])
        assert np.array_equal(pq.decrypt(cs, s_crt, pp2, enc=e, l=l), pt1 % p2)
    # absorbGFactors: k becomes 0 and the plaintext stays
    gc, k = pq.mulGCT(np.stack([pq.crt(x) for x in ct1]), 0, cs_crt=True)
    gc, k = pq.mulGCT(gc, k, cs_crt=True)
    assert np.array_equal(dec(gc, k=k, crt=True), pt1)
    try:
        ab, k0 = pq.absorbGFactors(gc, k, pp)
    except gpu.LolHipError as e:
        assert e.code == -7 and m % 2 == 1 and p % 3 == 0       # divG mod p impossible
        return
    assert k0 == 0
    assert np.array_equal(dec(ab, k=0, crt=True), pt1)
    want = pr.absorb_g(cpuref, Params(lm.factor_pps(m), qs), {"k": k, "c": np.stack([np.asarray(v) for v in gc])}, p)
    assert np.array_equal(ab, want["c"])


def test_homomprf_first_step(gpu, cpuref):
    """mulPublic firstElt ct (HomomPRF.hs:136-141): A_T(x)_0 of the lifted KHPRF at m = 128, q = 8 times one encryption
    of s at m' = 11648; decryption = A_T(x)_0 s in R_8 for every x"""
    import torch
    m, m2, q, base, k = 128, 11648, 8, 2, 6
    need = klr.bound(m, q, base)
    Qp = lm.first_good_q(m, max(need + 1, 2 ** 30))
    Pq, PQ = gpu.Plan.for_index(m, [q]), gpu.Plan.for_index(m, [Qp])
    rng = np.random.default_rng(12)
    nL = Pq.decomposeLen(base)
    a0, a1 = (rng.integers(0, q, size=(nL, Pq.n), dtype=np.int64) for _ in range(2))
    f = gpu.KHPRF.lifted(Pq, PQ, base, gpu.balanced_tree(k), a0, a1)
    B = 1 << k
    A = f.eval(0, B)                                                         # [B][L][n] powerful basis mod 8
    pq, pp = gpu.Plan.for_index(m2, ZQ4), gpu.Plan.for_index(m2, [q])
    lo, lo_p = gpu.Plan.for_index(m, ZQ4), gpu.Plan.for_index(m, [q])
    x_q, x_p = gpu.Ext(lo, pq), gpu.Ext(lo_p, pp)
    z = pq.errorRounded(0.5, B=1, key=bytes(32), ctr=0).cpu().numpy()
    s_key = np.ascontiguousarray(pq.crt(pq.l(pr.reduce(z, ZQ4))))[0]
    s_pt = rng.integers(0, q, size=(1, Pq.n), dtype=np.int64)
    ct = pq.encrypt(s_pt, s_key, pp, 0.5, key=bytes(range(32)), ctr=0, ext=x_p, out_crt=True)
    out = pq.mulPublic(A, torch.from_numpy(ct).cuda(), q, ext=x_q, cs_shared=True, stride=nL * Pq.n, B=B)
    got = pq.decrypt(out, torch.from_numpy(s_key).cuda(), pp, ext=x_p, cs_crt=True)
    first = A[:, 0, :].cpu().numpy()
    want = np.stack([pr.negacyclic(first[i], pr.decode(s_pt[0], q), q) for i in range(B)]).astype(np.int64)
    assert np.array_equal(got.cpu().numpy(), want)


def test_statuses_leave_output_untouched_and_side_stream(gpu):
    import torch
    qs = _moduli(1024, 30, 2)
    hi, lo = gpu.Plan.for_index(1024, qs), gpu.Plan.for_index(16, qs)
    x = gpu.Ext(lo, hi)
    rng = np.random.default_rng(3)
    B = 4
    cs = torch.from_numpy(_cs(rng, qs, 2, B, hi.n)).cuda()
    a = torch.from_numpy(_public(rng, B, lo.n, 8)).cuda()
    out = torch.full_like(cs, 0x5A5A)
    L = gpu.lib()
    work = torch.empty((L.lolhip_public_work_len(hi._h, x._h, B),), dtype=torch.int64, device="cuda")
    args = lambda p=8, stride=lo.n, ncs=2: (hi._h, x._h, None, a.data_ptr(), stride, p, cs.data_ptr(), ncs, 0,
                                            out.data_ptr(), work.data_ptr(), B)
    assert L.lolhip_mul_public_batch(*args(p=1)) == -2
    assert L.lolhip_mul_public_batch(*args(stride=3)) == -1
    assert L.lolhip_mul_public_batch(*args(ncs=0)) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())
    with pytest.raises(gpu.LolHipError):
        hi.addPublic(a, cs, 8, ext=x, l=2)
    side = torch.cuda.Stream()
    ref = hi.mulPublic(a, cs, 8, ext=x)
    with torch.cuda.stream(side):
        got = hi.mulPublic(a, cs, 8, ext=x, stream=side.cuda_stream)
        got2, _, _ = hi.addPublic(a, cs, 8, ext=x, l=3, cs_crt=True, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(got2, hi.addPublic(a, cs, 8, ext=x, l=3, cs_crt=True)[0])
