"""The homomorphic rounding 2^e -> 2 on the device (lolhip_ct_affine_mul_batch, lolhip_ptround_batch; lol-apps
HomomPRF.hs:215-270).  Every comparison is bit for bit.

 - Plan.ctAffineMul against Python integers: T = 1, 2, 3, 5, 16; slabs smaller than a tile and not a multiple of one;
   n' = 4, where a tile spans many polynomials and both component boundaries; inputs all q - 1, in (-q, 0] and random;
   alpha / beta 1, p, -1 and 2^63 - 1; va / vb present or not; a = b; out = a; 1, 2 and 4 pairs; the 8-byte route (one
   pointer off a 16-byte boundary) and the 16-byte route; 61-bit moduli at m' = 64; a side stream between guard words;
 - PTRound against the restatement of tests/ptround_ref.py over the CPU oracle: components, k_out and l_out;
 - the device's own key, PTRound.hints, encrypt and decrypt give the closed form;
 - the hints survive lolhip_chain_write / lolhip_chain_read.
"""
import ctypes as C

import numpy as np
import pytest

import ptround_ref as ptr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params

pytestmark = pytest.mark.gpu

P_PLAIN = 8


def _mixed(m, T):
    """T good moduli of index m, widths cycling over 20, 31, 59 and 61 bits"""
    gens = [lm.good_qs(m, 2 ** (b - 1)) for b in (20, 31, 59, 61)]
    return [next(gens[t % 4]) for t in range(T)]


def _wide(m, T):
    g = lm.good_qs(m, 2 ** 60)
    return [next(g) for _ in range(T)]


def _rand(rng, qs, shape, kind):
    """[shape][T]: 'top' = every residue q - 1, 'neg' = in (-q, 0], 'rand' = uniform in (-q, q)"""
    qa = np.array(qs, dtype=np.int64)
    if kind == "top":
        return np.ascontiguousarray(np.broadcast_to(qa - 1, shape + (len(qs),)))
    x = np.stack([rng.integers(0, q, size=shape, dtype=np.int64) for q in qs], axis=-1)
    if kind == "neg":
        return np.ascontiguousarray(-x)
    flip = rng.integers(0, 2, size=x.shape).astype(bool) & (x > 0)
    return np.ascontiguousarray(x - qa * flip)


def affine_mul_ref(qs, g, a, alpha, va, b, beta, vb, npairs):
    """[npairs][3][B][n][T] in Python integers"""
    q = np.array(qs, dtype=object)
    O = lambda x: np.asarray(x).astype(object)
    per = lambda v: np.array([int(v)] * len(qs) if np.ndim(v) == 0 else [int(x) for x in v], dtype=object)
    al, be, g = per(alpha), per(beta), O(g)
    out = []
    for j in range(npairs):
        A0 = (al * O(a[0]) + (0 if va is None else O(va[j]))) % q
        A1 = (al * O(a[1])) % q
        B0 = (be * O(b[0]) + (0 if vb is None else O(vb[j]))) % q
        B1 = (be * O(b[1])) % q
        out.append(np.stack([g * A0 * B0 % q, g * (A0 * B1 + A1 * B0) % q, g * A1 * B1 % q]))
    return np.stack(out).astype(np.int64)


# (m', T, B, input kind, alpha, beta, va?, vb?, a = b, npairs, moduli)
BIG = 2 ** 63 - 1
AM_CASES = [
    (12, 1, 300, "rand", 1, P_PLAIN, False, True, True, 1, _mixed),        # level 0: x (p x + v); 1200 words, partial tile
    (12, 2, 3, "rand", P_PLAIN, 1, True, True, True, 2, _mixed),           # the fan-out; 24 words: less than one tile
    (12, 3, 131, "neg", -1, BIG, True, False, False, 4, _mixed),           # 1572 words
    (12, 5, 77, "top", BIG, -1, False, False, False, 1, _mixed),           # the plain product, every input q - 1
    (12, 16, 37, "rand", P_PLAIN, P_PLAIN, True, True, False, 2, _mixed),
    (12, 3, 131, "top", 1, 1, True, True, True, 4, _wide),                 # 61-bit moduli, the 128-bit cross term at its largest
    (64, 3, 21, "rand", BIG, P_PLAIN, True, True, False, 2, _wide),        # 61-bit moduli at m' = 64
    (64, 3, 21, "neg", 1, 1, False, True, True, 1, _wide),
]


@pytest.mark.parametrize("case", AM_CASES, ids=lambda c: f"m{c[0]}-T{c[1]}-B{c[2]}-{c[3]}-np{c[9]}-{c[10].__name__}")
def test_ct_affine_mul_is_bit_exact(gpu, case):
    import torch
    m, T, B, kind, alpha, beta, has_va, has_vb, same, npairs, moduli = case
    qs = moduli(m, T)
    P = gpu.Plan(lm.factor_pps(m), qs)
    rng = np.random.default_rng(m * 1000 + T * 10 + npairs)
    a = _rand(rng, qs, (2, B, P.n), kind)
    b = a if same else _rand(rng, qs, (2, B, P.n), "rand" if kind == "top" else kind)
    va = _rand(rng, qs, (npairs, P.n), kind) if has_va else None
    vb = _rand(rng, qs, (npairs, P.n), "rand") if has_vb else None
    if not np.isscalar(alpha) or alpha == P_PLAIN:
        alpha = [P_PLAIN % q for q in qs]                              # per modulus, as lolhip_encode_scales gives it
    want = affine_mul_ref(qs, P.gCRT(), a, alpha, va, b, beta, vb, npairs)
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()
    da, dva, dvb = dev(a), dev(va), dev(vb)
    got = P.ctAffineMul(da, alpha, None if same else dev(b), beta, dva, dvb, npairs)
    torch.cuda.synchronize()
    assert got.shape == (npairs, 3, B, P.n, T)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(da.cpu().numpy(), a)                         # the inputs are only read
    # numpy in, numpy out
    assert np.array_equal(P.ctAffineMul(a, alpha, None if same else b, beta, va, vb, npairs), want)


@pytest.mark.parametrize("off", ["a", "b", "va", "vb", "out"])
def test_ct_affine_mul_eight_byte_route_and_side_stream(gpu, off):
    """Everything 16-byte aligned but one pointer, which is one word off: the 8-byte route, on a side stream, with guard
    words around out.  The aligned call (the 16-byte route) gives the same words."""
    import torch
    m, T, B, npairs = 12, 3, 131, 2
    qs = _mixed(m, T)
    P = gpu.Plan(lm.factor_pps(m), qs)
    rng = np.random.default_rng(ord(off[0]))
    a, b = _rand(rng, qs, (2, B, P.n), "rand"), _rand(rng, qs, (2, B, P.n), "rand")
    va, vb = _rand(rng, qs, (npairs, P.n), "rand"), _rand(rng, qs, (npairs, P.n), "neg")
    alpha, beta = [P_PLAIN] * T, [-1] * T
    want = affine_mul_ref(qs, P.gCRT(), a, alpha, va, b, beta, vb, npairs)
    GUARD = 0x7E7E7E7E7E7E
    bufs = {}
    for nm, x in (("a", a), ("b", b), ("va", va), ("vb", vb)):
        t = torch.zeros(x.size + 2, dtype=torch.int64, device="cuda")
        k = 1 if nm == off else 0
        t[k:k + x.size] = torch.from_numpy(x).cuda().reshape(-1)
        bufs[nm] = t[k:k + x.size]
    k = 1 if off == "out" else 0
    outb = torch.full((want.size + 66,), GUARD, dtype=torch.int64, device="cuda")
    out = outb[32 + k:32 + k + want.size]
    for nm, t in list(bufs.items()) + [("out", out)]:
        assert t.data_ptr() % 16 == (8 if nm == off else 0)
    arr = lambda v: (C.c_int64 * T)(*v)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = gpu.lib().lolhip_ct_affine_mul_batch(P._h, side.cuda_stream, bufs["a"].data_ptr(), arr(alpha), bufs["va"].data_ptr(),
                                              bufs["b"].data_ptr(), arr(beta), bufs["vb"].data_ptr(), npairs, out.data_ptr(), B)
    side.synchronize()
    assert rc == 0
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    assert (outb[:32 + k] == GUARD).all() and (outb[32 + k + want.size:] == GUARD).all()
    got = P.ctAffineMul(torch.from_numpy(a).cuda(), alpha, torch.from_numpy(b).cuda(), beta, torch.from_numpy(va).cuda(),
                        torch.from_numpy(vb).cuda(), npairs)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("same", [True, False])
def test_ct_affine_mul_out_may_be_a(gpu, same):
    """one pair, out = a: every input word is read before the stores (e_0, e_1 land on a_0, a_1)"""
    import torch
    m, T, B = 12, 2, 300
    qs = _mixed(m, T)
    P = gpu.Plan(lm.factor_pps(m), qs)
    rng = np.random.default_rng(5 + same)
    a, b = _rand(rng, qs, (2, B, P.n), "rand"), _rand(rng, qs, (2, B, P.n), "rand")
    vb = _rand(rng, qs, (1, P.n), "rand")
    want = affine_mul_ref(qs, P.gCRT(), a, 1, None, a if same else b, P_PLAIN, vb, 1)
    buf = torch.zeros((1, 3, B, P.n, T), dtype=torch.int64, device="cuda")
    buf[0, :2] = torch.from_numpy(a).cuda()
    got = P.ctAffineMul(buf[0, :2], 1, None if same else torch.from_numpy(b).cuda(), P_PLAIN, None, torch.from_numpy(vb).cuda(),
                        1, out=buf)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), want)


# ---- the chain against the model ---------------------------------------------------------------------------------------
def _ladder(cpuref, m, mp, p, base, seed, moduli=None):
    e = p.bit_length() - 1
    if moduli is None:
        g = lm.good_qs(mp, 2 ** 29)
        moduli = [next(g) for _ in range(e + 1)]
    L = ptr.Ladder(lambda pps, qs: sm.CpuEngine(cpuref, Params(pps, qs)), cpuref, m, mp, moduli, p, base,
                   np.random.default_rng(seed))
    L.keygen()
    return L


def _device(gpu, L, hints):
    """the device ladder of a model ladder: (PTRound, plans)"""
    import torch
    pps = lm.factor_pps(L.mp)
    plans = [gpu.Plan(pps, q) for q in L.zq]
    ups = [gpu.Plan(pps, q) for q in L.uq]
    exts = None
    if L.m != L.mp:
        exts = tuple(gpu.Ext(gpu.Plan(lm.factor_pps(L.m), q), pl) for q, pl in zip(L.zq[:2], plans[:2]))
    dh = [torch.from_numpy(np.ascontiguousarray(h)).cuda() for h in hints]
    return gpu.PTRound(plans, ups, dh, L.base, L.p, exts=exts), plans


# (m, m', p, base, [(enc, k, l, cs_crt, out_crt)])
CHAIN_CASES = [
    (16, 16, 4, 0, [("MSD", 0, 1, False, False), ("LSD", 0, 3, True, True)]),
    (16, 16, 8, 4, [("MSD", 0, 1, False, False), ("LSD", 0, 5, True, False), ("MSD", 0, 7, False, True)]),
    (16, 16, 16, 0, [("MSD", 0, 1, True, True), ("LSD", 0, 11, False, False)]),
    (45, 45, 8, 0, [("MSD", 0, 1, False, False), ("MSD", 1, 3, True, True), ("LSD", 1, 1, False, True)]),
    (15, 45, 8, 4, [("MSD", 0, 1, False, False), ("LSD", 1, 5, True, True)]),
    (16, 1024, 8, 0, [("MSD", 0, 3, False, True)]),
    (2048, 2048, 8, 0, [("LSD", 0, 1, True, False)]),
]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: f"m{c[0]}-mp{c[1]}-p{c[2]}-base{c[3]}")
def test_ptround_matches_the_model(gpu, cpuref, case):
    import torch
    m, mp, p, base, runs = case
    L = _ladder(cpuref, m, mp, p, base, seed=m + mp + p)
    hints = L.round_hints()
    rnd, plans = _device(gpu, L, hints)
    B = 3
    she0 = L.she(L.zq[0], L.ez[0], p)
    for enc, k, l, cs_crt, out_crt in runs:
        ct = {"enc": enc, "k": k, "l": l, "c": [she0.uniform(B), she0.uniform(B)]}
        want = ptr.pt_round(L, hints, ct)
        cs = np.stack([L.ez[0].crt(c) for c in ct["c"]]) if cs_crt else np.stack(ct["c"])
        got, genc, gk, gl = rnd(torch.from_numpy(np.ascontiguousarray(cs)).cuda(), enc, k, l, cs_crt, out_crt)
        torch.cuda.synchronize()
        wc = np.stack([L.ez[-1].crt(c) for c in want["c"]]) if out_crt else np.stack(want["c"])
        assert (genc, gk, gl) == (want["enc"], want["k"], want["l"]), (enc, k, l)
        assert gk == 2 ** (L.e - 1) * (k + 1) - 1
        assert np.array_equal(got.cpu().numpy(), wc), (enc, k, l, cs_crt, out_crt)


def test_ptround_61_bit_moduli(gpu, cpuref):
    """m' = 64, p = 4 over 61-bit moduli (the 64-bit arithmetic classes of every pass)"""
    L = _ladder(cpuref, 64, 64, 4, 0, seed=61, moduli=_wide(64, 3))
    hints = L.round_hints()
    rnd, _ = _device(gpu, L, hints)
    she0 = L.she(L.zq[0], L.ez[0], 4)
    for enc, l in (("MSD", 1), ("LSD", 3)):
        ct = {"enc": enc, "k": 0, "l": l, "c": [she0.uniform(3), she0.uniform(3)]}
        want = ptr.pt_round(L, hints, ct)
        got, genc, gk, gl = rnd(np.stack(ct["c"]), enc, 0, l)
        assert (genc, gk, gl) == ("MSD", 1, want["l"]) and np.array_equal(got, np.stack(want["c"]))


def test_ptround_identity_at_p_2(gpu, cpuref):
    """e = 1: the input itself, in the basis asked for; enc, k and l unchanged"""
    L = _ladder(cpuref, 45, 45, 2, 0, seed=1)
    rnd, plans = _device(gpu, L, [])
    she0 = L.she(L.zq[0], L.ez[0], 2)
    cs = np.stack([she0.uniform(3), she0.uniform(3)])
    for enc in ("LSD", "MSD"):
        got, genc, gk, gl = rnd(cs, enc, 2, 1)
        assert (genc, gk, gl) == (enc, 2, 1) and np.array_equal(got, cs)
    got, _, _, _ = rnd(cs, "MSD", 0, 1, out_crt=True)
    assert np.array_equal(got, np.stack([L.ez[0].crt(c) for c in cs]))
    got, _, _, _ = rnd(got, "MSD", 0, 1, cs_crt=True)
    assert np.array_equal(got, cs)


def _device_run(gpu, p, base, wire):
    """device key -> PTRound.hints -> encrypt every constant -> PTRound -> decrypt"""
    import torch
    m, svar, key = 16, 1.0, bytes(range(32))
    e = p.bit_length() - 1
    g = lm.good_qs(m, 2 ** 29)
    moduli = [next(g) for _ in range(e + 1)]
    pps = lm.factor_pps(m)
    plans = [gpu.Plan(pps, moduli[i + 1:]) for i in range(e)]
    ups = [gpu.Plan(pps, moduli[i:]) for i in range(e - 1)]
    sk = ups[0].errorRounded(svar, 1, key=key, ctr=1000)
    s_up = torch.remainder(sk.reshape(ups[0].n, 1), torch.tensor(moduli, dtype=torch.int64, device="cuda")).contiguous()
    ups[0].crt(ups[0].l(s_up))                                   # [n][T(U_0)], CRT basis; U_i and Z_i are its last columns
    hints, ctr = gpu.PTRound.hints(ups, [s_up[:, i:].contiguous() for i in range(e - 1)], svar, base, key=key, ctr=0)
    assert ctr == sum(u.decomposeLen(base) for u in ups)
    if wire:
        msgs = []
        for U, h in zip(ups, hints):
            Lh = h.shape[0]
            dec = U.lInv(U.crtInv(h.reshape(Lh * 2, U.n, U.T).clone())).cpu().numpy().reshape(Lh, 2, U.n, U.T)
            msgs.append(gpu.kshint_write(m, U.qs, dec))
        back = gpu.chain_read(gpu.chain_write(msgs))
        assert len(back) == e - 1
        hints2 = []
        for U, data, h in zip(ups, back, hints):
            mm, qq, xs = gpu.kshint_read(data)
            assert mm == m and qq == U.qs
            slab = U.crt(U.l(torch.from_numpy(xs.reshape(-1, U.n, U.T)).cuda())).reshape(h.shape)
            assert torch.equal(slab, h)
            hints2.append(slab.contiguous())
        hints = hints2
    rnd = gpu.PTRound(plans, ups, hints, base, p)
    pt = np.zeros((p, plans[0].n), dtype=np.int64)
    pt[:, 0] = np.arange(p)
    pp = gpu.Plan(pps, [p])
    ct = plans[0].encrypt(torch.from_numpy(pt).cuda(), s_up[:, 1:].contiguous(), pp, svar, key=key, ctr=5000)
    out, enc, k_out, l_out = rnd(ct, "LSD", 0, 1)
    dec = plans[-1].decrypt(out, s_up[:, e:].contiguous(), gpu.Plan(pps, [2]), enc=enc, k=k_out, l=l_out)
    torch.cuda.synchronize()
    return out, dec.cpu().numpy(), k_out


@pytest.mark.parametrize("p,base", [(4, 0), (8, 4), (16, 0)])
def test_ptround_decrypts_to_the_closed_form(gpu, p, base):
    _, dec, k_out = _device_run(gpu, p, base, wire=False)
    assert k_out == p // 2 - 1
    assert dec[:, 0].tolist() == [(c + p // 4) // (p // 2) % 2 for c in range(p)] and not dec[:, 1:].any()


def test_ptround_hints_survive_the_wire(gpu):
    """RoundHintChain: kshint_write per level -> chain_write -> chain_read -> kshint_read -> the same slabs, the same output"""
    import torch
    direct, dec_d, _ = _device_run(gpu, 8, 4, wire=False)
    wired, dec_w, _ = _device_run(gpu, 8, 4, wire=True)
    assert torch.equal(direct, wired) and np.array_equal(dec_d, dec_w)
