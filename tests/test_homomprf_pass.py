"""The reference's PASS check (lol-apps Examples/HomomPRF.hs:125-133) over a small chain:
    decrypt decKey (homomPRF ct x) == ptTunnel ptTunnelFuncs (ringPRF s x)       for x = 0 .. 7
homomPRF = ptRound . tunnelH . mulPublic (head (head (columns A_T(x)))) (HomomPRF.hs:136-141), with
  (r, r') = (8, 728) -> (28, 364) -> (182, 182), plaintext modulus 8, the PRF family over R_8 mod 8 (KHPRF.lifted,
  BaseBGad 2, a balanced tree of 3 leaves) rounded to Z_2, the tunnel functions linearDec (take dim crtSet)
  (TunnelChain.funcs), ptRound with e = 3, the key-switch gadget TrivGad.

The CPU model (`test_model_passes_and_random_functions_fail`, no GPU) runs the same pipeline over oracle/she_model.py,
tests/modswitch_ref.py, tests/ptround_ref.py, tests/public_ref.py, tests/khprf_lifted_ref.py and tests/crtset_ref.py.  A
chain with r != r' is the model's Chain over the ciphertext rings r': here e' = e r'/r = gcd(r'_h, r'_(h+1)) for both
hops (364, 182), the number of relative basis elements is the same as over the plaintext rings, and the function of a
hop is the plaintext function with every value embedded from S into S' (extendLin, Linear.hs:113-119).

The moduli list (MODULI below) is chosen as tests/test_ptround.py chooses its ladder: w_0 and U_0 = q_0 .. q_3 are the
first five primes above 2^29 that are 1 mod 728.  The tunnel runs over w_0 : U_0 (roundCTUp adds w_0), its input is over
U_0, its output over Z_0 = q_1 .. q_3 (two roundCTDowns); ptRound's ladder is U_0.  The model passes over this list
for all 8 inputs (asserted in the non-GPU test, which takes a few seconds), and with the functions replaced by random
tables of the same shape the equality fails for it (asserted there as well, so the check is known to bite).  The model
draws its keys and errors from numpy's generator and the device from its ChaCha20 streams, so the two runs share the
moduli, the family, s and the inputs, not the SHE keys."""
import math

import numpy as np
import pytest

import crtset_ref as cr
import khprf_lifted_ref as klr
import modswitch_ref as mr
import ptround_ref as ptr
import public_ref as pr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle import she_ref as sr
from oracle.oracle import Params

RS, RPS = (8, 28, 182), (728, 364, 182)
P, E, B = 8, 3, 8
PRF_BASE, KS_BASE = 2, 0
TREE = [3, 2, 1, 1, 1]                                   # balancedTree 3
_g = lm.good_qs(728, 2 ** 29)
MODULI = [next(_g) for _ in range(5)]                    # w_0, q_0, q_1, q_2, q_3


def _family(rng):
    nL = sr.gadlen(PRF_BASE, P)                                          # the family's rows: L entries over R_8
    a0, a1 = (rng.integers(0, P, size=(nL, 4), dtype=np.int64) for _ in range(2))
    s = rng.integers(0, P, size=(4,), dtype=np.int64)
    return a0, a1, s


def _clear(cpuref, a0, a1, s, funcs):
    """ptTunnel (funcs mod 2) (head (ringPRF s x)) for x = 0 .. 7: [B][72] residues mod 2, powerful basis of O_182"""
    R = klr.LiftedRing(cpuref, 8, P)
    y = np.stack([klr.ring_prf(R, PRF_BASE, TREE, a0, a1, s, 2, x)[0] for x in range(B)])    # decoding basis of R_2
    return cr.pt_tunnel(list(RS), [np.asarray(f) % 2 for f in funcs], y, 2)


def _model(cpuref, a0, a1, s, funcs, seed):
    """decrypt (homomPRF ct x) on the CPU model for x = 0 .. 7"""
    rng = np.random.default_rng(seed)
    mk = lambda pps, qs: sm.CpuEngine(cpuref, Params(pps, qs))
    mkt = lambda pe, pr_, ps, qs: sm.CpuTunnelEngine(cpuref, Params(pe, qs), Params(pr_, qs), Params(ps, qs))
    assert [math.gcd(RS[i], RS[i + 1]) * (RPS[i] // RS[i]) for i in range(2)] == [math.gcd(RPS[i], RPS[i + 1]) for i in range(2)]
    ch = mr.Chain(mk, mkt, RPS, MODULI, MODULI[1:], MODULI[2:], P, KS_BASE, rng)
    ch.gen_hints([cr.embed_pow(RS[h + 1], RPS[h + 1], np.asarray(funcs[h]) % P) for h in range(2)])
    R = klr.LiftedRing(cpuref, 8, P)
    atx = np.stack([klr.eval_tree(R, PRF_BASE, TREE, a0, a1, x)[0] for x in range(B)])       # [B][4], powerful basis
    she = ch.she_in
    ct = she.encrypt(cr.embed_pow(8, 728, s[None]))                                          # one encryption of s
    P_hi, P_lo = Params(lm.factor_pps(728), MODULI[1:]), Params(lm.factor_pps(8), MODULI[1:])
    ct1 = pr.mul_public(cpuref, P_hi, P_lo, atx, dict(ct, c=np.stack([she.e.crt(c) for c in ct["c"]])), P, B)
    ct1 = dict(ct1, c=[she.e.crtInv(np.ascontiguousarray(c)) for c in ct1["c"]])
    ct2 = ch.tunnel_h(ct1)
    L = ptr.Ladder(mk, cpuref, 182, 182, MODULI[1:], P, KS_BASE, rng)
    L.s_all = np.ascontiguousarray(ch.she[-1].s[..., 1:])                                    # decKey: the last tunnel key
    out = ptr.pt_round(L, L.round_hints(), ct2)
    return ptr.decrypt(L, out)


def test_model_passes_and_random_functions_fail(cpuref):
    rng = np.random.default_rng(2912)
    a0, a1, s = _family(rng)
    funcs = cr.tunnel_funcs(list(RS), 2, E)
    want = _clear(cpuref, a0, a1, s, funcs)
    assert want.any() and len({tuple(w) for w in want}) > 1
    assert np.array_equal(_model(cpuref, a0, a1, s, funcs, seed=1), want)
    rnd = [rng.integers(0, P, size=f.shape, dtype=np.int64) for f in funcs]
    assert not np.array_equal(_model(cpuref, a0, a1, s, rnd, seed=1), _clear(cpuref, a0, a1, s, rnd))


@pytest.mark.gpu
def test_homomprf_matches_the_clear_prf_through_the_tunnel(gpu, cpuref):
    import torch
    svar, key = 1.0, bytes(range(32))
    a0, a1, s = _family(np.random.default_rng(2912))
    mk = lambda m, qs: gpu.Plan(lm.factor_pps(m), qs)
    up, U0 = MODULI, MODULI[1:]
    # the family and the clear side
    Q = lm.first_good_q(8, max(klr.bound(8, P, PRF_BASE) + 1, 2 ** 30))
    prf = gpu.KHPRF.lifted(mk(8, [P]), mk(8, [Q]), PRF_BASE, TREE, a0, a1)
    atx = prf.eval(0, B)                                                 # [B][L][4], powerful basis mod 8
    clear_prf = prf(s, 2, 0, B)[:, 0].contiguous()                       # head (ringPRF s x): [B][4], decoding basis of R_2
    funcs = gpu.TunnelChain.funcs(list(RS), 2, E)
    clear = gpu.PTTunnel.for_rings(list(RS), 2, 1, funcs=[f % 2 for f in funcs])(clear_prf)
    # keys and hints
    Rp = [mk(m, up) for m in RPS]
    p_in, p_out = mk(728, U0), mk(182, up[2:])
    Ep = [mk(math.gcd(RPS[i], RPS[i + 1]), up) for i in range(2)]
    exts_er = [gpu.Ext(Ep[i], Rp[i]) for i in range(2)]
    exts_es = [gpu.Ext(Ep[i], Rp[i + 1]) for i in range(2)]
    exts_f = [gpu.Ext(mk(28, up), Rp[1]), None]
    sk = Rp[0].errorRounded(svar, 1, key=key, ctr=1000)
    s_up = torch.remainder(sk.reshape(Rp[0].n, 1), torch.tensor(up, dtype=torch.int64, device="cuda")).contiguous()
    Rp[0].crt(Rp[0].l(s_up))
    thints, ys, s_last, ctr = gpu.TunnelChain.hints(exts_er, exts_es, exts_f, funcs, s_up, P, svar, KS_BASE, key=key, ctr=0)
    chain = gpu.TunnelChain(exts_er, exts_es, ys, thints, KS_BASE, p_in, p_out)
    plans = [mk(182, U0[i + 1:]) for i in range(E)]                      # Z_0, Z_1, Z_2
    ups = [mk(182, U0[i:]) for i in range(E - 1)]                        # U_0, U_1
    rhints, _ = gpu.PTRound.hints(ups, [s_last[:, 1 + i:].contiguous() for i in range(E - 1)], svar, KS_BASE, key=key, ctr=ctr)
    rnd = gpu.PTRound(plans, ups, rhints, KS_BASE, P)
    # homomPRF
    pp_in = mk(728, [P])
    ext_in = gpu.Ext(mk(8, U0), p_in)
    ct = p_in.encrypt(torch.from_numpy(s[None]).cuda(), s_up[:, 1:].contiguous(), pp_in, svar, key=key, ctr=5000,
                      ext=gpu.Ext(mk(8, [P]), pp_in), out_crt=True)    # one encryption of s, CRT basis
    ct1 = p_in.mulPublic(atx, ct, P, ext=ext_in, cs_shared=True, stride=atx.shape[1] * atx.shape[2], B=B)
    ct2, enc, l = chain(ct1, P, "LSD", 1, cs_crt=True)
    out, enc, k, l = rnd(ct2, enc, 0, l)
    got = plans[-1].decrypt(out, s_last[:, E + 1:].contiguous(), mk(182, [2]), enc=enc, k=k, l=l)
    torch.cuda.synchronize()
    want = _clear(cpuref, a0, a1, s, cr.tunnel_funcs(list(RS), 2, E))
    assert want.any()
    assert np.array_equal(clear.cpu().numpy(), want)
    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
