"""tunnelH with the functions the reference uses (TunnelChain.funcs: linearDec (take dim crtSet), HomomPRF.hs:400-411)
against the clear-text tunnel (PTTunnel) over the same functions: (r, r') = (8, 728) -> (28, 364) -> (182, 182), p = 8,
with the device's own errorRounded / encrypt / TunnelChain.hints / decrypt.
    decrypt (tunnelH hints (encrypt x)) = ptTunnel funcs x,  bit for bit,
the middle of the reference's PASS check (mulPublic before it and ptRound after it are not part of this test).
Moduli: the first three primes above 2^29 that are 1 mod 728 (the up list), the input over the last two, the output over
the last one, as tests/test_modswitch.py chooses them for its chain of the same pattern.  The list is kept because the
CPU model passes over it (`test_model_tunnel_passes_over_this_list`, no GPU): tests/modswitch_ref.Chain over the
ciphertext rings 728 -> 364 -> 182 (here e' = gcd(r'_h, r'_(h+1))) with every function value embedded from S into S',
the same gadget and plaintext modulus, B = 8 inputs.  The model draws its keys and errors from numpy's generator, the
device from its ChaCha20 streams: the two runs share the moduli, the functions and the shape of the inputs."""
import math

import numpy as np
import pytest

import crtset_ref as cr
from oracle import lolmath as lm

RS, RPS, BASE = (8, 28, 182), (728, 364, 182), 2
_g = lm.good_qs(728, 2 ** 29)
UP = [next(_g) for _ in range(3)]


def _inputs():
    x = np.random.default_rng(728).integers(0, 8, size=(8, 4), dtype=np.int64)
    x[0] = [0, 1, 0, 0]
    x[1] = 7
    return x


def test_model_tunnel_passes_over_this_list(cpuref):
    import modswitch_ref as mr
    from oracle import she_model as sm
    from oracle.oracle import Params
    mk = lambda pps, qs: sm.CpuEngine(cpuref, Params(pps, qs))
    mkt = lambda pe, pr, ps, qs: sm.CpuTunnelEngine(cpuref, Params(pe, qs), Params(pr, qs), Params(ps, qs))
    funcs = cr.tunnel_funcs(list(RS), 2, 3)
    ch = mr.Chain(mk, mkt, RPS, UP, UP[1:], UP[2:], 8, BASE, np.random.default_rng(3))
    ch.gen_hints([cr.embed_pow(RS[h + 1], RPS[h + 1], funcs[h]) for h in range(2)])
    x = _inputs()
    ct = ch.she_in.encrypt(cr.embed_pow(8, 728, x))
    got = mr.decrypt_lin(ch.she_out, ch.tunnel_h(ct))                  # [B][72]: O_182 = S = S'
    want = cr.pt_tunnel(list(RS), funcs, x, 8)
    assert want.any() and np.array_equal(got, want)


@pytest.mark.gpu
def test_tunnel_chain_with_crt_set_functions_decrypts_to_pt_tunnel(gpu):
    import torch
    p, e, base, svar, B = 2, 3, BASE, 1.0, 8
    pe = p ** e
    rs, rps, up = RS, RPS, UP
    mk = lambda m, qs: gpu.Plan(lm.factor_pps(m), qs)
    Rp = [mk(m, up) for m in rps]                                       # R'_0, S'_0 = R'_1, S'_1 over the up list
    p_in, p_out = mk(728, up[1:]), mk(182, up[2:])
    eps = [math.gcd(rs[i], rs[i + 1]) * (rps[i] // rs[i]) for i in range(2)]       # e' = e (r' / r)
    assert eps == [364, 182]
    Ep = [mk(m, up) for m in eps]
    exts_er = [gpu.Ext(Ep[i], Rp[i]) for i in range(2)]
    exts_es = [gpu.Ext(Ep[i], Rp[i + 1]) for i in range(2)]
    exts_f = [gpu.Ext(mk(28, up), Rp[1]), None]                         # S_i into S'_i
    funcs = gpu.TunnelChain.funcs(list(rs), p, e)
    assert all(np.array_equal(f.cpu().numpy(), w) for f, w in zip(funcs, cr.tunnel_funcs(list(rs), p, e)))
    key = bytes(range(32))
    sk = Rp[0].errorRounded(svar, 1, key=key, ctr=1000)
    s_up = torch.remainder(sk.reshape(Rp[0].n, 1), torch.tensor(up, dtype=torch.int64, device="cuda")).contiguous()
    Rp[0].crt(Rp[0].l(s_up))
    hints, ys, s_last, _ = gpu.TunnelChain.hints(exts_er, exts_es, exts_f, funcs, s_up, pe, svar, base, key=key, ctr=0)
    chain = gpu.TunnelChain(exts_er, exts_es, ys, hints, base, p_in, p_out)
    x = _inputs()
    pp_in = mk(728, [pe])
    ct = p_in.encrypt(torch.from_numpy(x).cuda(), s_up[:, 1:].contiguous(), pp_in, svar, key=key, ctr=5000,
                      ext=gpu.Ext(mk(8, [pe]), pp_in))
    out, enc, l = chain(ct, pe, "LSD", 1)
    got = p_out.decrypt(out, s_last[:, 2:].contiguous(), mk(182, [pe]), enc=enc, k=0, l=l)
    clear = gpu.PTTunnel.for_rings(list(rs), p, e, funcs=funcs)(torch.from_numpy(x).cuda())     # O_8: decoding = powerful basis
    torch.cuda.synchronize()
    want = cr.pt_tunnel(list(rs), cr.tunnel_funcs(list(rs), p, e), x, pe)
    assert want.any()
    assert np.array_equal(clear.cpu().numpy(), want)
    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
