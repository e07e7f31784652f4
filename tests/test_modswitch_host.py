"""Host side of ciphertext modSwitch and multi-hop tunnelling (include/lolhip.h lolhip_modswitch_batch,
lolhip_tunnel_chain_*): no GPU needed.

 - the six entries are exported and declared, and lol_amd has Plan.modSwitch and TunnelChain;
 - every status of the entries on host-only plans, sentinel-filled out / l_out untouched;
 - work lengths: 0 at B = 0, a negative status for bad arguments, the formula of the header;
 - the restatement of tests/modswitch_ref.py: up then down is the identity, down by 1 is the oracle's
   rescale_drop_first, down by d is d applications of it, |q_0 out - c| <= q_0 / 2 on the centred lifts;
 - the chain property Dec (tunnelH ct) = evalLin f_2 (evalLin f_1 x) mod p on the CPU model, r = 8 -> 12 -> 30.
"""
import ctypes as C
import os
import re
from math import prod

import numpy as np
import pytest

import modswitch_ref as mr
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle import she_ref as sr
from oracle.oracle import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_modswitch_work_len", "lolhip_modswitch_batch", "lolhip_tunnel_chain_create", "lolhip_tunnel_chain_destroy",
       "lolhip_tunnel_chain_work_len", "lolhip_tunnel_chain_batch")
INVALID, MODULUS, NO_CRT, NO_DEVICE = -1, -2, -3, -5
SENT = 0x5A5A5A5A

CHAIN_MS, CHAIN_CASES, chain_moduli, run_chain = mr.CHAIN_MS, mr.CHAIN_CASES, mr.chain_moduli, mr.run_chain


def test_modswitch_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"
    assert callable(lolhip.Plan.modSwitch)
    for nm in ("__call__", "workLen", "hints"):
        assert callable(getattr(lolhip.TunnelChain, nm))


def _plans(lolhip, m=16, T=4, bits=30):
    g = lm.good_qs(m, 2 ** (bits - 1))
    qs = [next(g) for _ in range(T)]
    return qs, [lolhip.Plan.for_index(m, qs[i:], host_only=True) for i in range(T)]


def test_modswitch_statuses_on_host_only_plans(lolhip):
    L = lolhip.lib()
    qs, pl = _plans(lolhip)
    full, last2 = pl[0], pl[2]
    B, ncs = 2, 2
    cs = np.zeros((ncs, B, full.n, full.T), dtype=np.int64)
    out = np.full((ncs, B, full.n, 16), SENT, dtype=np.int64)
    work = np.zeros(cs.size, dtype=np.int64)
    lo = C.c_int64(SENT)
    P = lambda a: a.ctypes.data

    def call(f=full, t=last2, c=cs, ncs=ncs, crt=0, enc=0, l=1, p=257, o=out, ocrt=0, lout=True, w=work, Bn=B):
        return L.lolhip_modswitch_batch(None if f is None else f._h, None if t is None else t._h, None,
                                        None if c is None else P(c), ncs, crt, enc, l, p, None if o is None else P(o), ocrt,
                                        C.byref(lo) if lout else None, None if w is None else P(w), Bn)

    assert call() == NO_DEVICE                                   # everything valid: only the device is missing
    assert call(t=full) == NO_DEVICE and call(f=last2, t=full) == NO_DEVICE
    for kw in (dict(f=None), dict(t=None), dict(c=None), dict(o=None), dict(w=None), dict(lout=False)):
        assert call(**kw) == INVALID, kw
    assert call(ncs=0) == INVALID and call(Bn=-1) == INVALID
    assert call(enc=2) == INVALID and call(enc=-1) == INVALID
    other = lolhip.Plan.for_index(32, qs[2:], host_only=True)
    assert call(t=other) == INVALID                              # another index
    swapped = lolhip.Plan.for_index(16, [qs[3], qs[2]], host_only=True)
    assert call(t=swapped) == INVALID                            # not a suffix
    assert call(t=lolhip.Plan.for_index(16, qs[:2], host_only=True)) == INVALID        # a prefix is not a suffix
    g = lm.good_qs(16, 2 ** 20)
    many = [next(g) for _ in range(17)]
    assert call(f=lolhip.Plan.for_index(16, many[:7], host_only=True), t=lolhip.Plan.for_index(16, many[6:7], host_only=True)) == INVALID
    assert call(f=lolhip.Plan.for_index(16, many[6:7], host_only=True), t=lolhip.Plan.for_index(16, many[:7], host_only=True)) == INVALID
    assert call(f=lolhip.Plan.for_index(16, many, host_only=True), t=lolhip.Plan.for_index(16, many[1:], host_only=True)) == INVALID
    assert call(f=lolhip.Plan.for_index(16, many[1:], host_only=True), t=lolhip.Plan.for_index(16, many, host_only=True)) == INVALID
    for p in (1, 0, -3):
        assert call(p=p) == MODULUS
    assert call(p=qs[1]) == MODULUS                              # LSD input: p has no inverse mod q_1
    assert call(p=qs[1], enc=1) == NO_DEVICE                     # ... which an MSD input does not need
    dup = [qs[2], qs[2], qs[3]]
    assert call(f=lolhip.Plan.for_index(16, dup, host_only=True), t=lolhip.Plan.for_index(16, dup[1:], host_only=True)) == MODULUS
    nf, nt = (lolhip.Plan.for_index(16, q, host_only=True) for q in ([2 ** 20, 2 ** 21 + 1], [2 ** 21 + 1]))
    assert call(f=nf, t=nt, p=5) == NO_DEVICE and call(f=nf, t=nt, p=5, crt=1) == NO_CRT and call(f=nf, t=nt, p=5, ocrt=1) == NO_CRT
    assert (out == SENT).all() and lo.value == SENT
    assert call(Bn=0, c=None, o=None, w=None) == NO_DEVICE
    # the Python method raises the same codes before it stages anything
    for to, p, code in ((last2, 257, NO_DEVICE), (other, 257, INVALID), (last2, qs[1], MODULUS)):
        with pytest.raises(lolhip.LolHipError) as e:
            full.modSwitch(to, cs, p)
        assert e.value.code == code


def test_modswitch_work_len(lolhip):
    L = lolhip.lib()
    qs, pl = _plans(lolhip, m=45, T=4)
    for f, t in ((pl[0], pl[2]), (pl[2], pl[0]), (pl[1], pl[1])):
        assert L.lolhip_modswitch_work_len(f._h, t._h, 3, 0) == 0
        for ncs, B in ((1, 1), (2, 7), (3, 1001)):
            assert L.lolhip_modswitch_work_len(f._h, t._h, ncs, B) == ncs * B * f.n * f.T
    f, t = pl[0], pl[2]
    assert L.lolhip_modswitch_work_len(f._h, t._h, 0, 1) == INVALID
    assert L.lolhip_modswitch_work_len(f._h, t._h, 1, -1) == INVALID
    assert L.lolhip_modswitch_work_len(None, t._h, 1, 1) == INVALID
    assert L.lolhip_modswitch_work_len(f._h, lolhip.Plan.for_index(16, qs[2:], host_only=True)._h, 1, 1) == INVALID


def _chain_plans(lolhip, ms=CHAIN_MS):
    up = chain_moduli()
    mk = lambda m, qs: lolhip.Plan.for_index(m, qs, host_only=True)
    import math
    hops = []
    for r, s in zip(ms[:-1], ms[1:]):
        E, R, S = mk(math.gcd(r, s), up), mk(r, up), mk(s, up)
        hops.append((lolhip.Ext(E, R), lolhip.Ext(E, S), R, S))
    return up, mk, hops


def test_tunnel_chain_statuses_and_work_len(lolhip):
    L = lolhip.lib()
    up, mk, hops = _chain_plans(lolhip)
    p_in, p_out = mk(8, up[1:]), mk(30, up[2:])
    n = len(hops)
    vp = lambda vals: (C.c_void_p * max(len(vals), 1))(*vals)
    er, es = [h[0]._h for h in hops], [h[1]._h for h in hops]
    fake = [8, 8]                                                 # borrowed device pointers: only stored by create

    def create(n=n, er=er, es=es, ys=fake, hints=fake, base=2, pi=p_in, po=p_out):
        h = C.c_void_p()
        rc = L.lolhip_tunnel_chain_create(n, vp(er), vp(es), vp(ys), vp(hints), base, None if pi is None else pi._h,
                                          None if po is None else po._h, C.byref(h))
        assert (h.value is None) == (rc != 0)
        return rc, h

    rc, h = create()
    assert rc == 0
    T = 3
    for B in (1, 5):
        sub = max(2 * B * 4 * 2, *[L.lolhip_tunnel_work_len(a, b, 2, B) for a, b in zip(er, es)])
        assert L.lolhip_tunnel_chain_work_len(h, B) == 4 * B * 8 * T + sub           # n_max = phi(30) = 8
    assert L.lolhip_tunnel_chain_work_len(h, 0) == 0
    assert L.lolhip_tunnel_chain_work_len(h, -1) == INVALID and L.lolhip_tunnel_chain_work_len(None, 1) == INVALID
    B = 2
    cs = np.zeros((2, B, 4, 2), dtype=np.int64)
    out = np.full((2, B, 8, 1), SENT, dtype=np.int64)
    work = np.zeros(L.lolhip_tunnel_chain_work_len(h, B), dtype=np.int64)
    lo = C.c_int64(SENT)

    def batch(hh=h, c=cs, crt=0, enc=0, l=1, p=8, o=out, ocrt=0, lout=True, w=work, Bn=B):
        return L.lolhip_tunnel_chain_batch(hh, None, None if c is None else c.ctypes.data, crt, enc, l, p,
                                           None if o is None else o.ctypes.data, ocrt, C.byref(lo) if lout else None,
                                           None if w is None else w.ctypes.data, Bn)

    assert batch() == NO_DEVICE
    for kw in (dict(hh=None), dict(c=None), dict(o=None), dict(w=None), dict(lout=False), dict(Bn=-1), dict(enc=2)):
        assert batch(**kw) == INVALID, kw
    assert batch(p=1) == MODULUS and batch(p=up[1]) == MODULUS
    assert (out == SENT).all() and lo.value == SENT
    L.lolhip_tunnel_chain_destroy(h)
    # the Python class raises the same codes before it stages anything
    ch = lolhip.TunnelChain([x[0] for x in hops], [x[1] for x in hops], fake, fake, 2, p_in, p_out)
    for p, code in ((8, NO_DEVICE), (1, MODULUS)):
        with pytest.raises(lolhip.LolHipError) as e:
            ch(cs, p)
        assert e.value.code == code
    # create: hops that do not meet, plans not of the end rings or not over a suffix of the up list
    assert create(er=er[::-1], es=es[::-1])[0] == INVALID
    assert create(pi=mk(12, up[1:]))[0] == INVALID and create(po=mk(12, up[2:]))[0] == INVALID
    assert create(pi=mk(8, up[:2]))[0] == INVALID and create(po=mk(30, up[:1]))[0] == INVALID
    assert create(n=-1)[0] == INVALID and create(pi=None)[0] == INVALID and create(base=1)[0] == INVALID
    assert create(ys=[8, 0])[0] == INVALID
    g = lm.good_qs(120, 2 ** 40)
    alien = [next(g) for _ in range(3)]
    E2, S2 = lolhip.Plan.for_index(6, alien, host_only=True), lolhip.Plan.for_index(30, alien, host_only=True)
    R2 = lolhip.Plan.for_index(12, alien, host_only=True)
    x2 = (lolhip.Ext(E2, R2), lolhip.Ext(E2, S2))
    assert create(er=[er[0], x2[0]._h], es=[es[0], x2[1]._h])[0] == INVALID           # hop 1 over other moduli
    # nhops = 0: modSwitch between the two plans
    s_up, s_out = mk(30, up), mk(30, up[2:])                      # the chain borrows its plans: keep them alive
    rc, h0 = create(n=0, pi=s_up, po=s_out)
    assert rc == 0 and L.lolhip_tunnel_chain_work_len(h0, 3) == 2 * 3 * 8 * 3
    assert batch(hh=h0) == NO_DEVICE and batch(hh=h0, p=0) == MODULUS
    L.lolhip_tunnel_chain_destroy(h0)
    assert create(n=0, pi=mk(30, up), po=mk(12, up[2:]))[0] == INVALID
    L.lolhip_tunnel_chain_destroy(None)


# ---- the restatement ------------------------------------------------------------------------------------------------
def _mixed(m, T):
    """T good moduli of index m, widths cycling over 20, 31, 59 and 61 bits"""
    gens = [lm.good_qs(m, 2 ** (b - 1)) for b in (20, 31, 59, 61)]
    return [next(gens[t % 4]) for t in range(T)]


def _rows(rng, qs, rows):
    return np.stack([rng.integers(0, q, size=rows, dtype=np.int64) for q in qs], axis=-1)


@pytest.mark.parametrize("u", [1, 2, 5])
def test_up_then_down_is_the_identity(u):
    rng = np.random.default_rng(u)
    qs = _mixed(16, 3 + u)
    x = _rows(rng, qs[u:], 64)
    up = mr.rescale(x, qs[u:], qs)
    assert up.shape == (64, 3 + u) and not up[:, :u].any()
    assert np.array_equal(mr.rescale(up, qs, qs[u:]), x)


def test_down_equals_the_oracle_rescale_and_rounds_to_nearest():
    rng = np.random.default_rng(7)
    qs = _mixed(16, 6)
    P = Params(lm.factor_pps(16), qs)
    c = _rows(rng, qs, 5 * P.n)
    c[0] = 0
    c[1] = [q - 1 for q in qs]
    c[2] = [q // 2 for q in qs]
    c[3] = [q // 2 + 1 for q in qs]
    c3 = c.reshape(5, P.n, 6)
    one = mr.rescale(c3, qs, qs[1:])
    assert np.array_equal(one, sr.rescale_drop_first(P, c3))
    cur, moduli = c3, qs
    for d in range(1, 6):
        cur = sr.rescale_drop_first(Params(lm.factor_pps(16), moduli), cur)
        moduli = moduli[1:]
        assert np.array_equal(mr.rescale(c3, qs, qs[d:]), cur), d
    # |q_0 out - c| <= q_0 / 2 on the centred lifts over the product ring
    diff = qs[0] * mr.crt_lift(one, qs[1:]) - mr.crt_lift(c3, qs)
    Q = prod(qs)
    diff = (diff + Q // 2) % Q - Q // 2
    assert (2 * np.abs(diff) <= qs[0]).all()
    # negatives in (-q, 0) are the same residues
    neg = c3 - np.array(qs, dtype=np.int64) * (c3 > 0)
    assert np.array_equal(mr.rescale(neg, qs, qs[2:]), mr.rescale(c3, qs, qs[2:]))


@pytest.mark.parametrize("p,base", CHAIN_CASES)
def test_chain_property_holds_for_the_model_on_the_cpu_oracle(cpuref, p, base):
    ch, ct, funcs, x, want = run_chain(lambda pps, qs: sm.CpuEngine(cpuref, Params(pps, qs)),
                                       lambda pe, pr, ps, qs: sm.CpuTunnelEngine(cpuref, Params(pe, qs), Params(pr, qs), Params(ps, qs)),
                                       cpuref, p, base, seed=p + base)
    steps = []
    out = ch.tunnel_h(ct, steps)
    assert np.array_equal(mr.decrypt_lin(ch.she_out, out), want)
    # every hop decrypts exactly too: the parameters are inside the noise budget of the reference's own algorithm
    for i, (she, mid) in enumerate(steps):
        assert np.array_equal(mr.decrypt_lin(she, mid), mr.pt_tunnel(cpuref, CHAIN_MS, chain_moduli()[0], p, x, funcs[:i])), i
