"""Ciphertext modSwitch and multi-hop tunnelling on the device (lolhip_modswitch_batch, lolhip_tunnel_chain_batch;
lol-apps SymmSHE.hs:236-246, HomomPRF.hs:427-431) against the restatement of tests/modswitch_ref.py.

 - lolhip_modswitch_batch bit for bit: down, up and same-modulus cases over mixed-width moduli, both encodings, both
   bases on each side, 1-3 components, edge residues (0, q-1, the lift tie, negatives), a partial last tile, slabs
   that are not 16-byte aligned (the scalar kernels) and a side stream;
 - the same words as the route callers took before: toMSD + lInv + one rescaleDropFirst per modulus + l;
 - scratch stays inside work_len words and cs is only read;
 - encrypt -> ct x ct -> keySwitchQuadCirc -> modSwitch -> decrypt is the plaintext product;
 - tunnelH: the chain call equals the hop-by-hop composition bit for bit and decrypts to f_2 (f_1 x); nhops = 0 is
   modSwitch; the reference's shape pattern m != m' with the device's own encrypt / hints / decrypt.
"""
import ctypes as C
import math

import numpy as np
import pytest

import modswitch_ref as mr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle.oracle import Params

pytestmark = pytest.mark.gpu

# (m, T -> T')
CASES = [(16, 2, 1), (16, 5, 3), (16, 16, 11), (16, 6, 1), (45, 3, 1), (45, 1, 3), (16, 1, 6), (16, 4, 4)]
P_PLAIN = 257


def _mixed(m, T):
    """T good moduli of index m, widths cycling over 20, 31, 59 and 61 bits"""
    gens = [lm.good_qs(m, 2 ** (b - 1)) for b in (20, 31, 59, 61)]
    return [next(gens[t % 4]) for t in range(T)]


def _inputs(rng, qs, ncs, B, n, negatives):
    """[ncs][B][n][T] with the edge residues in the first rows of every component"""
    c = np.stack([rng.integers(0, q, size=(ncs, B, n), dtype=np.int64) for q in qs], axis=-1)
    qa = np.array(qs, dtype=np.int64)
    c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 0, 3] = 0, qa - 1, qa // 2, qa // 2 + 1
    c[:, 0, 4, 1:] = 0                                           # the tie against zeros in the kept components
    c[:, 0, 4, 0] = qa[0] // 2 + 1
    if negatives:                                                # the same residues, written in (-q, 0)
        flip = rng.integers(0, 2, size=c.shape).astype(bool) & (c > 0)
        c = c - qa * flip
    return np.ascontiguousarray(c)


def _moduli_pair(m, T, To):
    qs = _mixed(m, max(T, To))
    return qs[max(T, To) - T:], qs[max(T, To) - To:]


@pytest.mark.parametrize("m,T,To", CASES)
def test_modswitch_is_bit_exact(gpu, cpuref, m, T, To):
    import torch
    pps = lm.factor_pps(m)
    qf, qt = _moduli_pair(m, T, To)
    F, G = gpu.Plan(pps, qf), gpu.Plan(pps, qt)
    ef, et = sm.CpuEngine(cpuref, Params(pps, qf)), sm.CpuEngine(cpuref, Params(pps, qt))
    rng = np.random.default_rng(100 * m + 16 * T + To)
    B = 67 if m == 16 else 23                                   # more than one tile, the last one partial
    k = 0
    for enc in ("LSD", "MSD"):
        for cs_crt in (False, True):
            for out_crt in (False, True):
                ncs = 1 + k % 3
                k += 1
                cs = _inputs(rng, qf, ncs, B, F.n, negatives=True)
                got, genc, gl = F.modSwitch(G, torch.from_numpy(cs).cuda(), P_PLAIN, enc, 5, cs_crt, out_crt)
                want, wl = mr.mod_switch(ef, et, list(cs % np.array(qf, dtype=np.int64)), P_PLAIN, enc, 5, cs_crt, out_crt)
                assert genc == "MSD" and gl == wl, (enc, cs_crt, out_crt)
                assert np.array_equal(got.cpu().numpy(), want), (enc, cs_crt, out_crt, ncs)


def test_modswitch_to_the_same_moduli_off_a_power_of_two(gpu, cpuref):
    """m = 45, T = 2 -> 2: the scale alone, where the call leaves the l / lInv passes over c_0 out; the restatement
    makes them"""
    import torch
    pps = lm.factor_pps(45)
    qs = _mixed(45, 2)
    F, G = gpu.Plan(pps, qs), gpu.Plan(pps, qs)
    e = sm.CpuEngine(cpuref, Params(pps, qs))
    rng = np.random.default_rng(4522)
    for enc in ("LSD", "MSD"):
        for cs_crt, out_crt in ((False, False), (True, False), (False, True), (True, True)):
            cs = _inputs(rng, qs, 2, 23, F.n, negatives=True)
            got, genc, gl = F.modSwitch(G, torch.from_numpy(cs).cuda(), P_PLAIN, enc, 5, cs_crt, out_crt)
            want, wl = mr.mod_switch(e, e, list(cs % np.array(qs, dtype=np.int64)), P_PLAIN, enc, 5, cs_crt, out_crt)
            assert genc == "MSD" and gl == wl, (enc, cs_crt, out_crt)
            assert np.array_equal(got.cpu().numpy(), want), (enc, cs_crt, out_crt)


def _raw(gpu, F, G, cs, ncs, B, p, enc, l, out, work, cs_crt=0, out_crt=0, stream=0):
    lo = C.c_int64(0)
    rc = gpu.lib().lolhip_modswitch_batch(F._h, G._h, stream, cs.data_ptr(), ncs, cs_crt, enc, l, p, out.data_ptr(), out_crt,
                                          C.byref(lo), work.data_ptr(), B)
    assert rc == 0
    return lo.value


@pytest.mark.parametrize("T,To", [(2, 1), (4, 2), (2, 4)])
def test_modswitch_partial_tile_unaligned_slabs_and_side_stream(gpu, cpuref, T, To):
    """m = 64, B = 1001: 2 * 1001 * 32 rows end inside a tile.  Then the same call with cs and out one word off a
    16-byte boundary (the scalar kernels), on a side stream."""
    import torch
    pps = lm.factor_pps(64)
    qf, qt = _moduli_pair(64, T, To)
    F, G = gpu.Plan(pps, qf), gpu.Plan(pps, qt)
    ef, et = sm.CpuEngine(cpuref, Params(pps, qf)), sm.CpuEngine(cpuref, Params(pps, qt))
    rng = np.random.default_rng(T * 7 + To)
    ncs, B = 2, 1001
    cs = _inputs(rng, qf, ncs, B, F.n, negatives=True)
    want, wl = mr.mod_switch(ef, et, list(cs % np.array(qf, dtype=np.int64)), P_PLAIN, "LSD", 3)
    got, _, gl = F.modSwitch(G, torch.from_numpy(cs).cuda(), P_PLAIN, "LSD", 3)
    assert gl == wl and np.array_equal(got.cpu().numpy(), want)
    buf_in = torch.zeros(cs.size + 1, dtype=torch.int64, device="cuda")
    buf_out = torch.zeros(want.size + 1, dtype=torch.int64, device="cuda")
    buf_in[1:] = torch.from_numpy(cs).cuda().reshape(-1)
    work = torch.zeros(max(gpu.lib().lolhip_modswitch_work_len(F._h, G._h, ncs, B), 1), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert buf_in[1:].data_ptr() % 16 == 8 and buf_out[1:].data_ptr() % 16 == 8
    gl = _raw(gpu, F, G, buf_in[1:], ncs, B, P_PLAIN, 0, 3, buf_out[1:], work, stream=side.cuda_stream)
    side.synchronize()
    assert gl == wl and np.array_equal(buf_out[1:].cpu().numpy().reshape(want.shape), want)
    assert int(buf_out[0]) == 0


def test_modswitch_equals_the_composition_of_single_drops(gpu):
    """down by 2 at m = 45, T = 4 -> 2 equals Plan.toMSD + lInv + rescaleDropFirst on successive plans + l, bit for bit"""
    import torch
    pps = lm.factor_pps(45)
    qs = _mixed(45, 4)
    P4, P3, P2 = (gpu.Plan(pps, qs[i:]) for i in range(3))
    rng = np.random.default_rng(45)
    B = 9
    cs = torch.from_numpy(_inputs(rng, qs, 2, B, P4.n, negatives=False)).cuda()
    got, _, gl = P4.modSwitch(P2, cs, P_PLAIN, "LSD", 7)
    msd, _, l = P4.toMSD(cs, P_PLAIN, "LSD", 7)
    c0 = P4.lInv(msd[0].clone())
    c0 = P2.l(P3.rescaleDropFirst(P4.rescaleDropFirst(c0)))
    c1 = P3.rescaleDropFirst(P4.rescaleDropFirst(msd[1].contiguous()))
    torch.cuda.synchronize()
    assert gl == l
    assert torch.equal(got[0], c0) and torch.equal(got[1], c1)


@pytest.mark.parametrize("m", [45, 64])
def test_modswitch_scratch_stays_inside_work_len_and_cs_is_only_read(gpu, m):
    import torch
    pps = lm.factor_pps(m)
    qs = _mixed(m, 3)
    F, G = gpu.Plan(pps, qs), gpu.Plan(pps, qs[2:])
    rng = np.random.default_rng(m)
    ncs, B, GUARD = 3, 5, 0x7E7E7E7E7E7E
    cs_h = _inputs(rng, qs, ncs, B, F.n, negatives=False)
    cs = torch.from_numpy(cs_h).cuda()
    wl = gpu.lib().lolhip_modswitch_work_len(F._h, G._h, ncs, B)
    assert wl == ncs * B * F.n * F.T
    buf = torch.full((wl + 64,), GUARD, dtype=torch.int64, device="cuda")
    outb = torch.full((ncs * B * G.n * G.T + 64,), GUARD, dtype=torch.int64, device="cuda")
    for cs_crt, out_crt in ((1, 1), (0, 0)):
        _raw(gpu, F, G, cs, ncs, B, P_PLAIN, 0, 1, outb[32:], buf[32:], cs_crt, out_crt)
        torch.cuda.synchronize()
        assert (buf[:32] == GUARD).all() and (buf[32 + wl:] == GUARD).all()
        assert (outb[:32] == GUARD).all() and (outb[-32:] == GUARD).all()
        assert np.array_equal(cs.cpu().numpy(), cs_h)


@pytest.mark.parametrize("m,p,lower", [(64, 257, 2 ** 29), (45, 181, 2 ** 30)])
def test_she_product_survives_modswitch(gpu, cpuref, m, p, lower):
    """encrypt -> ct x ct -> keySwitchQuadCirc -> Plan.modSwitch -> decrypt = the plaintext product, the GPU as the
    engine of oracle/she_model.py"""
    pps = lm.factor_pps(m)
    g = lm.good_qs(m, lower)
    qs = [next(g), next(g)]
    rng = np.random.default_rng(m + p)
    P2, P1, Pp = gpu.Plan(pps, qs), gpu.Plan(pps, qs[1:]), gpu.Plan(pps, [p])
    she = sm.SHE(P2, Pp, qs, p, rng)
    she.keygen()
    B = 3
    pt1 = rng.integers(0, p, size=(B, she.n), dtype=np.int64)
    pt2 = rng.integers(0, p, size=(B, she.n), dtype=np.int64)
    want = cpuref.polymul(Params(pps, [p]), pt1[..., None], pt2[..., None]).reshape(pt1.shape)
    lin = she.key_switch_quad(she.ks_quad_hint(0), 0, she.mul(she.encrypt(pt1), she.encrypt(pt2)))
    assert np.array_equal(she.decrypt(lin), want)
    she1 = sm.SHE(P1, Pp, qs[1:], p, rng)
    she1.s = np.ascontiguousarray(she.s[..., 1:])
    she1.s_crt = P1.crt(she1.s)
    for enc_in in ("MSD", "LSD"):
        ct = lin if enc_in == "MSD" else she.toLSD(lin)
        out, enc, l = P2.modSwitch(P1, np.stack(ct["c"]), p, ct["enc"], ct["l"])
        assert enc == "MSD"
        assert np.array_equal(she1.decrypt({"enc": "MSD", "k": lin["k"], "l": l, "c": [out[0], out[1]]}), want), enc_in


# ---- tunnelH ----------------------------------------------------------------------------------------------------------
class TunnelEngine:
    """lol_amd.Ext pairs as the engine of oracle/she_model.py's tunnel"""

    def __init__(self, gpu, GE, GR, GS):
        self.XR, self.XS = gpu.Ext(GE, GR), gpu.Ext(GE, GS)

    def evalLin(self, r_dec, ys_crt): return self.XR.evalLin(self.XS, r_dec, ys_crt)
    def tunnel(self, c0_dec, c1_pow, ys_crt, hints, base): return self.XR.tunnel(self.XS, c0_dec, c1_pow, ys_crt, hints, base)


@pytest.mark.parametrize("p,base", mr.CHAIN_CASES)
def test_tunnel_chain_on_the_device(gpu, cpuref, p, base):
    """r = 8 -> 12 -> 30 (r' = r): the model with the GPU as its engine decrypts to f_2 (f_1 x); the one-call chain
    equals the hop-by-hop composition over the device API bit for bit and decrypts to the same; nhops = 0 is modSwitch"""
    import torch
    ch, ct, funcs, x, want = mr.run_chain(lambda pps, qs: gpu.Plan(pps, qs),
                                          lambda pe, pr, ps, qs: TunnelEngine(gpu, gpu.Plan(pe, qs), gpu.Plan(pr, qs), gpu.Plan(ps, qs)),
                                          cpuref, p, base, seed=31 * p + base, B=3)
    assert np.array_equal(mr.decrypt_lin(ch.she_out, ch.tunnel_h(ct)), want)
    up = ch.up_qs
    p_in, p_out, mid = ch.she_in.e, ch.she_out.e, gpu.Plan(lm.factor_pps(30), up[1:])
    plans = [s.e for s in ch.she]                                       # R_0, S_0 = R_1, S_1 over the up list
    exts = [(h["xeng"].XR, h["xeng"].XS) for h in ch.hops]
    ys = [torch.from_numpy(h["ys"]).cuda() for h in ch.hops]
    hints = [torch.from_numpy(h["hints"]).cuda() for h in ch.hops]
    chain = gpu.TunnelChain([e[0] for e in exts], [e[1] for e in exts], ys, hints, base, p_in, p_out)
    cs = torch.from_numpy(np.stack(ct["c"])).cuda()
    for out_crt in (False, True):
        got, enc, gl = chain(cs, p, "LSD", 1, out_crt=out_crt)
        # hop by hop: modSwitch up, then per hop lInv c0 / tunnel / crtInv, then two one-step modSwitches down
        cur, _, l = p_in.modSwitch(plans[0], cs, p, "LSD", 1)
        for (xr, xs), R, S, y, h in zip(exts, plans[:-1], plans[1:], ys, hints):
            c0 = R.lInv(cur[0].clone())
            cur = S.crtInv(xr.tunnel(xs, c0, cur[1].contiguous(), y, h, base))
        cur, _, l = plans[-1].modSwitch(mid, cur, p, "MSD", l)
        cur, _, l = mid.modSwitch(p_out, cur, p, "MSD", l, out_crt=out_crt)
        torch.cuda.synchronize()
        assert enc == "MSD" and gl == l
        assert torch.equal(got, cur), out_crt
    c = got.cpu().numpy()
    c = [p_out.crtInv(np.ascontiguousarray(c[0])), p_out.crtInv(np.ascontiguousarray(c[1]))]
    assert np.array_equal(mr.decrypt_lin(ch.she_out, {"enc": "MSD", "k": 0, "l": gl, "c": c}), want)
    # nhops = 0
    none = gpu.TunnelChain([], [], [], [], base, plans[-1], p_out)
    fresh = torch.from_numpy(np.stack([ch.she[-1].uniform(3), ch.she[-1].uniform(3)])).cuda()
    a, _, la = none(fresh, p, "LSD", 3)
    b, _, lb = plans[-1].modSwitch(p_out, fresh, p, "LSD", 3)
    assert la == lb and torch.equal(a, b)


def test_tunnel_chain_reference_shape_pattern(gpu, cpuref):
    """(r, r') = (8, 120) -> (12, 60) -> (30, 30), the pattern of HomomPRFParams' RngList (H_i' = H_i times the odd part
    still to come), p = 8, base 2, with the device's own errorRounded / encrypt / TunnelChain.hints / decrypt:
    decrypt (chain (encrypt x)) = f_2 (f_1 x) computed on the CPU at the plaintext rings."""
    import torch
    p, base, svar, B = 8, 2, 1.0, 3
    up = mr.chain_moduli()
    rs, rps = (8, 12, 30), (120, 60, 30)
    mk = lambda m, qs: gpu.Plan(lm.factor_pps(m), qs)
    Rp = [mk(m, up) for m in rps]                                       # R'_0, S'_0 = R'_1, S'_1 over the up list
    p_in, p_out = mk(120, up[1:]), mk(30, up[2:])
    eps = [math.gcd(rs[i], rs[i + 1]) * (rps[i] // rs[i]) for i in range(2)]       # e' = e (r' / r): 60, 30
    assert eps == [60, 30]
    Ep = [mk(e, up) for e in eps]
    exts_er = [gpu.Ext(Ep[i], Rp[i]) for i in range(2)]
    exts_es = [gpu.Ext(Ep[i], Rp[i + 1]) for i in range(2)]
    exts_f = [gpu.Ext(mk(12, up), Rp[1]), None]                         # S_i into S'_i
    rng = np.random.default_rng(2024)
    funcs = [rng.integers(0, p, size=(2, 4), dtype=np.int64), rng.integers(0, p, size=(2, 8), dtype=np.int64)]
    key = bytes(range(32))
    # the key of R'_0, over the up list (hints) and over the input moduli (encrypt)
    sk = Rp[0].errorRounded(svar, 1, key=key, ctr=1000)
    s_up = torch.remainder(sk.reshape(Rp[0].n, 1), torch.tensor(up, dtype=torch.int64, device="cuda")).contiguous()
    Rp[0].crt(Rp[0].l(s_up))
    hints, ys, s_last, ctr = gpu.TunnelChain.hints(exts_er, exts_es, exts_f, funcs, s_up, p, svar, base, key=key, ctr=0)
    assert ctr == sum(2 * S.decomposeLen(base) for S in Rp[1:])
    chain = gpu.TunnelChain(exts_er, exts_es, ys, hints, base, p_in, p_out)
    x = rng.integers(0, p, size=(B, 4), dtype=np.int64)
    x[0] = 0
    x[0, 1] = 1
    pp_in = mk(120, [p])
    ct = p_in.encrypt(torch.from_numpy(x).cuda(), s_up[:, 1:].contiguous(), pp_in, svar, key=key, ctr=5000,
                      ext=gpu.Ext(mk(8, [p]), pp_in))
    out, enc, l = chain(ct, p, "LSD", 1)
    got = p_out.decrypt(out, s_last[:, 2:].contiguous(), mk(30, [p]), enc=enc, k=0, l=l)
    torch.cuda.synchronize()
    want = mr.pt_tunnel(cpuref, rs, up[0], p, x, funcs)
    assert want.any()
    assert np.array_equal(got.cpu().numpy(), want)
