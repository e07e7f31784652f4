"""crtSetDec, crtSet and powBasisPow on the host (lolhip_crtset_dec, lolhip_crtset_host, lolhip_ext_table 6), and the
statuses of lolhip_pt_tunnel_create over host-only plans.  No GPU.

 - counts against the closed form K = (phi(m')/ord_m'(p)) / (phi(m)/ord_m(p)), for the reference's five hops and for the
   small chain 8 -> 28 -> 182;
 - the ring identities of a CRT set over Z_(p^e), products taken with the CPU oracle mod a prime far above them;
 - crtSet mod p = embedPow (l crtSetDec);
 - every element evaluated at the roots of unity of crtset_ref's own field: 0 / 1, constant on cosets of <p>, supported
   on exactly one m'-coset above every m-coset;
 - equality with tests/crtset_ref.py under the stated rule for the root of unity, and determinism;
 - powBasisPow through sum_i embedPow(coeffs_i x) b_i = x on the host tables (the same identity through
   lolhip_ext_host runs in tests/test_crtset.py: that entry needs a device).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import crtset_ref as cr
from oracle import lolmath as lm
from oracle.oracle import Params

CASES = [(1, 7, 2, 1), (1, 7, 2, 2), (1, 7, 2, 3), (1, 91, 2, 3), (7, 91, 2, 3), (4, 28, 2, 3), (14, 182, 2, 3),
         (1, 13, 3, 2), (1, 35, 3, 2), (64, 448, 2, 3), (224, 2912, 2, 3)]
IDS = [f"{m}-{m2}-p{p}-e{e}" for m, m2, p, e in CASES]
REF_RINGS = [128, 448, 2912, 3640, 5460, 4095]              # H0 .. H5 of the reference's HomomPRF example
ERR_INVALID, ERR_MODULUS, ERR_NO_DEVICE = -1, -2, -5


def _strip(v, p):
    while v % p == 0:
        v //= p
    return v


def _pps(m):
    return lm.factor_pps(m) if m > 1 else []


@functools.lru_cache(maxsize=None)
def _set(lolhip, m, m2, p, e):
    return lolhip.crtSet(_pps(m), _pps(m2), p, e, host=True)


def _hops(rings):
    return [(math.gcd(r, s), r, s) for r, s in zip(rings[:-1], rings[1:])]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_match_the_closed_form(lolhip, case):
    m, m2, p, e = case
    mb, mb2 = _strip(m, p), _strip(m2, p)
    want = (lm.totient_pps(_pps(mb2)) // cr.order(p, mb2)) // ((lm.totient_pps(_pps(mb)) if mb > 1 else 1) // cr.order(p, mb))
    dec = lolhip.crtSetDec(_pps(mb), _pps(mb2), p)
    assert dec.shape == (want, lm.totient_pps(_pps(mb2)))
    assert _set(lolhip, m, m2, p, e).shape == (want, lm.totient_pps(_pps(m2)))
    assert dec.min() >= 0 and dec.max() < p
    assert _set(lolhip, m, m2, p, e).min() >= 0 and _set(lolhip, m, m2, p, e).max() < p ** e


@pytest.mark.parametrize("rings,sets,dims", [(REF_RINGS, [2, 3, 4, 2, 3], [2, 2, 4, 2, 2]), ([8, 28, 182], [2, 3], [2, 2])],
                         ids=["reference", "small"])
def test_hop_sets_cover_the_hop_dimensions(lolhip, rings, sets, dims):
    L = lolhip.lib()
    from lol_amd.tensor import _pps as arr
    got_sets, got_dims = [], []
    for eh, r, s in _hops(rings):
        (_, a, na), (_, b, nb) = arr(_pps(_strip(eh, 2))), arr(_pps(_strip(s, 2)))
        got_sets.append(L.lolhip_crtset_dec(a, na, b, nb, 2, None, 0))
        got_dims.append(lm.totient_pps(_pps(r)) // lm.totient_pps(_pps(eh)))
    assert got_sets == sets and got_dims == dims


def test_funcs_shapes_and_too_small_a_set(lolhip):
    fs = lolhip.TunnelChain.funcs([8, 28, 182], 2, 3, host=True)
    assert [f.shape for f in fs] == [(2, 12), (2, 72)]
    want = cr.tunnel_funcs([8, 28, 182], 2, 3)
    assert all(np.array_equal(f, w) for f, w in zip(fs, want))
    with pytest.raises(ValueError):
        lolhip.TunnelChain.funcs([8, 12], 2, 3, host=True)             # O_12/O_4 mod 2 has one CRT element, the hop needs two


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ring_identities_over_zpe(lolhip, cpuref, case):
    """c_i^2 = c_i, c_i c_j = 0, sum c_i = 1 in O_m' / p^e: the oracle multiplies the lifts mod a 40-bit prime (every
    coefficient of a product of two lifts is below C_m' p^2e < 2^39) and the centred result is reduced mod p^e"""
    m, m2, p, e = case
    cs, pe = _set(lolhip, m, m2, p, e), p ** e
    K, n = cs.shape
    P = Params(_pps(m2), [lm.first_good_q(m2, 2 ** 40)])
    Q = P.qs[0]
    a = np.repeat(cs, K, axis=0).reshape(K * K, n, 1)
    b = np.tile(cs, (K, 1)).reshape(K * K, n, 1)
    prod = cpuref.polymul(P, a, b).reshape(K, K, n)
    prod = np.where(2 * prod < Q, prod, prod - Q) % pe
    for i in range(K):
        for j in range(K):
            assert np.array_equal(prod[i, j], cs[i] if i == j else np.zeros(n, dtype=np.int64)), (i, j)
    one = np.zeros(n, dtype=np.int64)
    one[0] = 1
    assert np.array_equal(cs.sum(axis=0) % pe, one)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_set_mod_p_is_the_embedded_dec_set(lolhip, case):
    m, m2, p, e = case
    mb, mb2 = _strip(m, p), _strip(m2, p)
    dec = lolhip.crtSetDec(_pps(mb), _pps(mb2), p)
    assert np.array_equal(_set(lolhip, m, m2, p, e) % p, cr.embed_pow(mb2, m2, cr.l_pow(_pps(mb2), dec, p)))


@functools.lru_cache(maxsize=None)
def _roots(p, m2):
    F = cr.GF(p, cr.order(p, m2))
    w = F.pow(F.gen, (p ** F.d - 1) // m2)
    pows = [F.one]
    for _ in range(m2 - 1):
        pows.append(F.mul(pows[-1], w))
    return F, pows


@pytest.mark.parametrize("case", sorted({(_strip(m, p), _strip(m2, p), p) for m, m2, p, _ in CASES}), ids=str)
def test_evaluations_are_indicator_functions_of_coset_unions(lolhip, case):
    m, m2, p = case
    F, pows = _roots(p, m2)
    R = cr.ring(m2)
    elems = cr.l_pow(_pps(m2), lolhip.crtSetDec(_pps(m), _pps(m2), p), p)          # powerful basis mod p
    units = [i for i in range(1, m2 + 1) if math.gcd(i, m2) == 1]
    zero = tuple([0] * F.d)
    supports = []
    for c in elems:
        support = set()
        for i in units:
            v = zero
            for cj, ex in zip(c, R.expo):
                for _ in range(int(cj)):
                    v = F.add(v, pows[i * int(ex) % m2])
            assert v in (zero, F.one)
            if v == F.one:
                support.add(i % m2)
        supports.append(support)
    above = {}
    for co in cr.cosets(p, m2):
        above.setdefault(frozenset(x % m for x in co), []).append(frozenset(co))
    for s in supports:
        for lo, his in above.items():
            inside = [h for h in his if h <= s]
            assert len(inside) == 1 and all(h <= s or not (h & s) for h in his)     # whole cosets, one above each m-coset
    assert set().union(*supports) == {i % m2 for i in units} and sum(len(s) for s in supports) == len(units)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_equals_the_restatement_and_is_deterministic(lolhip, case):
    m, m2, p, e = case
    mb, mb2 = _strip(m, p), _strip(m2, p)
    dec = lolhip.crtSetDec(_pps(mb), _pps(mb2), p)
    assert np.array_equal(dec, np.array(cr.crtset_dec(mb, mb2, p), dtype=np.int64))
    assert np.array_equal(dec, lolhip.crtSetDec(_pps(mb), _pps(mb2), p))
    got = lolhip.crtSet(_pps(m), _pps(m2), p, e, host=True)
    assert np.array_equal(got, cr.crtset(m, m2, p, e))
    assert np.array_equal(got, _set(lolhip, m, m2, p, e))


@pytest.mark.parametrize("m,m2,p,e", [(1, 8, 2, 3), (4, 8, 2, 3), (1, 1, 2, 2), (3, 9, 3, 2)])
def test_a_p_power_index_has_the_set_one(lolhip, m, m2, p, e):
    """m' a power of p: the p-free part is the index 1, the CRT set is {1}"""
    got = lolhip.crtSet(_pps(m), _pps(m2), p, e, host=True)
    n = lm.totient_pps(_pps(m2)) if m2 > 1 else 1
    assert got.shape == (1, n) and got[0, 0] == 1 and not got[0, 1:].any()
    assert np.array_equal(got, cr.crtset(m, m2, p, e))
    (f,) = lolhip.TunnelChain.funcs([4, 8], 2, 3, host=True)           # a hop into a 2-power ring over O_4: the function 1
    assert f.tolist() == [[1, 0, 0, 0]]
    with pytest.raises(ValueError):
        lolhip.TunnelChain.funcs([12, 8], 2, 3, host=True)             # over O_4 from O_12: one element, two needed


def test_short_buffers_and_statuses(lolhip):
    from lol_amd.tensor import _pps as arr
    L = lolhip.lib()
    (_, a, na), (_, b, nb) = arr([]), arr(_pps(91))
    full = lolhip.crtSetDec([], _pps(91), 2)
    GUARD = 0x5A5A5A5A5A5A
    buf = np.full((2 + 3 * 72 + 2,), GUARD, dtype=np.int64)
    ptr = buf[2:].ctypes.data_as(C.POINTER(C.c_int64))
    assert L.lolhip_crtset_dec(a, na, b, nb, 2, ptr, 3) == 6               # cap rows are written, K is returned
    assert np.array_equal(buf[2:2 + 3 * 72].reshape(3, 72), full[:3]) and (buf[:2] == GUARD).all() and (buf[-2:] == GUARD).all()
    buf[:] = GUARD
    assert L.lolhip_crtset_host(a, na, b, nb, 2, 3, ptr, 3) == 6
    assert np.array_equal(buf[2:2 + 3 * 72].reshape(3, 72), lolhip.crtSet([], _pps(91), 2, 3, host=True)[:3])
    assert (buf[:2] == GUARD).all() and (buf[-2:] == GUARD).all()
    (_, b7, nb7) = arr(_pps(7))
    assert L.lolhip_crtset_host(a, na, b7, nb7, 2, 62, None, 0) == ERR_MODULUS          # 2^62: no prime below 2^61 certifies it
    assert L.lolhip_crtset_modulus(b7, nb7, 2, 62) == ERR_MODULUS
    assert L.lolhip_crtset_modulus(b7, nb7, 2, 30) == ERR_MODULUS                       # 2 C_7 (2^29)^2 = 22 2^58 >= 2^61
    q = L.lolhip_crtset_modulus(b7, nb7, 2, 3)
    assert q == lm.first_good_q(7, 2 * 11 * 16)                                        # C_7 = 11, (p^e/2)^2 = 16
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.crtSet([], _pps(7), 2, 62, host=True)
    assert ei.value.code == ERR_MODULUS
    assert L.lolhip_crtset_dec(a, na, b7, nb7, 7, None, 0) == ERR_INVALID               # p | m'
    assert L.lolhip_crtset_dec(a, na, b7, nb7, 4, None, 0) == ERR_INVALID               # p not prime
    (_, a3, na3) = arr(_pps(3))
    assert L.lolhip_crtset_dec(a3, na3, b7, nb7, 2, None, 0) == ERR_INVALID             # m does not divide m'
    assert L.lolhip_crtset_host(a3, na3, b7, nb7, 2, 3, None, 0) == ERR_INVALID
    assert L.lolhip_crtset_host(a, na, b7, nb7, 2, 0, None, 0) == ERR_INVALID           # e < 1


@pytest.mark.parametrize("m,m2", [(4, 28), (14, 182), (3, 45), (8, 8), (1, 35), (12, 180)])
def test_pow_basis_pow_rebuilds_every_element(lolhip, m, m2):
    """sum_i embedPow(coeffs_i x) b_i = x with b_i the powerful-basis unit vector at powBasisPow[i]"""
    q = 257
    lo, hi = lolhip.Plan(_pps(m), [q], host_only=True), lolhip.Plan(_pps(m2), [q], host_only=True)
    x = lolhip.Ext(lo, hi)
    pbp, co, emb = x.powBasisPow(), x.table(5).reshape(hi.n // lo.n, lo.n), x.table(2)
    assert pbp.shape == (hi.n // lo.n,) and np.array_equal(pbp, co[:, 0])
    R = cr.ring(m2)
    v = np.random.default_rng(m2).integers(0, q, size=hi.n)
    acc = np.zeros(hi.n, dtype=np.int64)
    for i in range(hi.n // lo.n):
        c = v[co[i]]                                                          # coeffs_i, an element of O_m
        up = np.where(emb >= 0, c[np.maximum(emb, 0)], 0)                      # embedPow
        b = np.zeros(hi.n, dtype=np.int64)
        b[pbp[i]] = 1
        acc = (acc + R.mul(up, b, q)) % q
    assert np.array_equal(acc, v)


def test_pt_tunnel_create_statuses(lolhip):
    L = lolhip.lib()
    rings, p, e = [8, 28, 182], 2, 3
    funcs = cr.tunnel_funcs(rings, p, e)
    t = lolhip.PTTunnel.for_rings(rings, p, e, funcs=funcs, host_only=True)    # validates, certifies, uploads nothing
    nmax = 72
    assert t.workLen(3) == 2 * 3 * nmax + max(2 * 3 * (2 + 12), 2 * 3 * (6 + 72))
    assert L.lolhip_pt_tunnel_batch(t._h, None, None, None, None, 0) == ERR_NO_DEVICE
    with pytest.raises(lolhip.LolHipError) as ei:                              # the method raises it before it stages anything
        t(np.zeros((3, 4), dtype=np.int64))
    assert ei.value.code == ERR_NO_DEVICE
    assert L.lolhip_pt_tunnel_work_len(t._h, -1) == ERR_INVALID
    # the bound of a hop: 2 rel C_S G_S D_R (p^e/2)^2
    b0 = lolhip.PTTunnel.modulus(8, 28, 2, True, p, e)
    b1 = lolhip.PTTunnel.modulus(28, 182, 2, False, p, e)
    assert b0 == 2 * 2 * (2 * 11) * 6 * 1 * 16 and b1 == 2 * 2 * (11 * 23) * (6 * 12) * 2 * 16   # C_4 = 2, C_7 = 11, C_13 = 23
    assert [x.hi.qs[0] > b for x, b in zip(t.exts_es, (b0, b1))] == [True, True]

    def build(q0, q1, e1_index=14):
        er, es = [], []
        for (eh, r, s), q in zip([(4, 8, 28), (e1_index, 28, 182)], (q0, q1)):
            E, R, S = (lolhip.Plan.for_index(m, [q], host_only=True) for m in (eh, r, s))
            er.append(lolhip.Ext(E, R))
            es.append(lolhip.Ext(E, S))
        return er, es

    q_ok0, q_ok1 = t.exts_es[0].hi.qs[0], t.exts_es[1].hi.qs[0]
    small = lm.first_good_q(182, 1000)                                         # a CRT basis, but far below the bound
    assert small < b1
    er, es = build(q_ok0, small)
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.PTTunnel(er, es, funcs, p, e)
    assert ei.value.code == ERR_MODULUS
    er, es = build(q_ok0, q_ok1)
    other_e = lolhip.Plan.for_index(2, [q_ok1], host_only=True)                # hop 1 with two different E plans
    es_bad = [es[0], lolhip.Ext(other_e, es[1].hi)]
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.PTTunnel(er, es_bad, funcs, p, e)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(lolhip.LolHipError) as ei:                              # S_0 = O_28 but hop 1 starts from O_8
        lolhip.PTTunnel([er[0], er[0]], [es[0], es[0]], [funcs[0], funcs[0]], p, e)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.PTTunnel([], [], [], p, e)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.PTTunnel(er, es, funcs, p, 62)
    assert ei.value.code == ERR_MODULUS
    nocrt = 2 ** 40 + 15                                                       # no CRT basis for O_182
    er, es = build(q_ok0, nocrt)
    with pytest.raises(lolhip.LolHipError) as ei:
        lolhip.PTTunnel(er, es, funcs, p, e)
    assert ei.value.code == -3
