"""Nothing stores past lolhip_*_work_len (GPU): the four entries whose work-buffer layout nests another entry's
(ptRound, the tunnel chain, ptTunnel, tunnelHint) run through a raw ctypes call over one tensor of work_len + 4096 words;
the tail keeps its sentinel and the output equals the output of the Python wrapper's own call.  The buffer is always
large enough, so nothing here can fault.  Shapes: the smallest at which every region of the layout is non-empty."""
import ctypes as C
import math

import numpy as np
import pytest

import crtset_ref as cr
import modswitch_ref as mr
from oracle import lolmath as lm

pytestmark = pytest.mark.gpu
TAIL, SENT = 4096, 0x5A5A5A5A5A5A5A5A
KEY = bytes(range(32))


def _work(wl):
    import torch
    assert wl > 0
    return torch.full((wl + TAIL,), SENT, dtype=torch.int64, device="cuda")


def _tail_intact(work, wl):
    import torch
    torch.cuda.synchronize()
    return bool((work[wl:] == SENT).all()) and not bool((work[:wl] == SENT).all())


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _uniform(rng, shape, qs):
    import torch
    return torch.from_numpy(np.stack([rng.integers(0, q, size=shape, dtype=np.int64) for q in qs], axis=-1)).cuda()


def _key_over(plan, qs, ctr):
    """a rounded-Gaussian key of the plan's ring reduced into qs, CRT basis: [n][len(qs)]"""
    import torch
    sk = plan.errorRounded(1.0, 1, key=KEY, ctr=ctr)
    s = torch.remainder(sk.reshape(plan.n, 1), torch.tensor(qs, dtype=torch.int64, device="cuda")).contiguous()
    plan.crt(plan.l(s))                                           # in place
    return s


def test_ptround_stays_inside_work_len(gpu):
    """m' = 16 over m = 8 (the embed regions), p = 8 (level 1 fans out), base 2, five moduli, B = 3"""
    import torch
    L = gpu.lib()
    p, e, base, B = 8, 3, 2, 3
    g = lm.good_qs(16, 2 ** 29)
    qs = [next(g) for _ in range(5)]
    pps, pps_m = lm.factor_pps(16), lm.factor_pps(8)
    plans = [gpu.Plan(pps, qs[i + 1:]) for i in range(e)]
    ups = [gpu.Plan(pps, qs[i:]) for i in range(e - 1)]
    exts = tuple(gpu.Ext(gpu.Plan(pps_m, qs[i + 1:]), plans[i]) for i in range(2))
    s_up = _key_over(ups[0], qs, 1000)
    hints, _ = gpu.PTRound.hints(ups, [s_up[:, i:].contiguous() for i in range(e - 1)], 1.0, base, key=KEY, ctr=0)
    rnd = gpu.PTRound(plans, ups, hints, base, p, exts=exts)
    cs = _uniform(np.random.default_rng(1), (2, B, plans[0].n), qs[1:])
    want, _, k_want, l_want = rnd(cs, "MSD", 0, 1)
    wl = rnd.workLen(B)
    work, out = _work(wl), torch.zeros_like(want)
    ko, lo = C.c_int64(0), C.c_int64(0)
    rc = L.lolhip_ptround_batch(rnd._h, _stream(), cs.data_ptr(), 0, 1, 0, 1, out.data_ptr(), 0, C.byref(ko), C.byref(lo),
                                work.data_ptr(), B)
    assert rc == 0 and _tail_intact(work, wl)
    assert torch.equal(out, want) and (ko.value, lo.value) == (k_want, l_want)


def test_tunnel_chain_stays_inside_work_len(gpu):
    """8 -> 12 -> 30 over the up list of tests/modswitch_ref.py, p = 8, base 2, B = 2"""
    import torch
    L = gpu.lib()
    p, base, B = 8, 2, 2
    up, rs = mr.chain_moduli(), mr.CHAIN_MS
    mk = lambda m, qs: gpu.Plan(lm.factor_pps(m), qs)
    R = [mk(m, up) for m in rs]
    E = [mk(math.gcd(a, b), up) for a, b in zip(rs[:-1], rs[1:])]
    er, es = [gpu.Ext(E[i], R[i]) for i in range(2)], [gpu.Ext(E[i], R[i + 1]) for i in range(2)]
    p_in, p_out = mk(rs[0], up[1:]), mk(rs[-1], up[2:])
    rng = np.random.default_rng(2)
    funcs = [rng.integers(0, p, size=(R[i].n // E[i].n, R[i + 1].n), dtype=np.int64) for i in range(2)]
    hints, ys, _, _ = gpu.TunnelChain.hints(er, es, [None, None], funcs, _key_over(R[0], up, 1000), p, 1.0, base, key=KEY, ctr=0)
    chain = gpu.TunnelChain(er, es, ys, hints, base, p_in, p_out)
    cs = _uniform(rng, (2, B, p_in.n), up[1:])
    want, _, l_want = chain(cs, p, "LSD", 1)
    wl = chain.workLen(B)
    work, out = _work(wl), torch.zeros_like(want)
    lo = C.c_int64(0)
    rc = L.lolhip_tunnel_chain_batch(chain._h, _stream(), cs.data_ptr(), 0, 0, 1, p, out.data_ptr(), 0, C.byref(lo),
                                     work.data_ptr(), B)
    assert rc == 0 and _tail_intact(work, wl)
    assert torch.equal(out, want) and lo.value == l_want


def test_pt_tunnel_stays_inside_work_len(gpu):
    """8 -> 28 -> 182 mod 2^3, B = 3"""
    import torch
    L = gpu.lib()
    rings, p, e, B = [8, 28, 182], 2, 3, 3
    t = gpu.PTTunnel.for_rings(rings, p, e, funcs=cr.tunnel_funcs(rings, p, e))
    x = torch.from_numpy(np.random.default_rng(3).integers(0, p ** e, size=(B, 4), dtype=np.int64)).cuda()
    want = t(x)
    wl = t.workLen(B)
    work, out = _work(wl), torch.zeros_like(want)
    rc = L.lolhip_pt_tunnel_batch(t._h, _stream(), x.data_ptr(), out.data_ptr(), work.data_ptr(), B)
    assert rc == 0 and _tail_intact(work, wl)
    assert want.any() and torch.equal(out, want)


def test_tunnel_hint_stays_inside_work_len(gpu):
    """4 | 12 -> 4 | 20 over two moduli, base 2"""
    import torch
    L = gpu.lib()
    base, svar, ctr = 2, 1.0, 7
    g = lm.good_qs(60, 2 ** 29)
    qs = [next(g), next(g)]
    PE, PR, PS = (gpu.Plan.for_index(m, qs) for m in (4, 12, 20))
    XR, XS = gpu.Ext(PE, PR), gpu.Ext(PE, PS)
    rel = PR.n // PE.n
    ys = _uniform(np.random.default_rng(4), (rel, PS.n), qs)
    s_in, s_out = _key_over(PR, qs, 1000), _key_over(PS, qs, 1001)
    want = XR.tunnelHint(XS, ys, s_in, s_out, svar, base, key=KEY, ctr=ctr)
    wl = L.lolhip_tunnel_hint_work_len(XR._h, XS._h, base)
    work, out = _work(wl), torch.zeros_like(want)
    rc = L.lolhip_tunnel_hint_batch(XR._h, XS._h, _stream(), ys.data_ptr(), s_in.data_ptr(), s_out.data_ptr(), svar, base, KEY,
                                    ctr, out.data_ptr(), work.data_ptr())
    assert rc == 0 and _tail_intact(work, wl)
    assert want.any() and torch.equal(out, want)
