"""Every lolhip_*_work_len entry over host-only handles against recorded values (tests/golden/work_len.json): no GPU
needed.  The entries measure the same layout functions the batch entries carve the caller's buffer with, so a length
that moves here is a buffer whose regions moved.

`table` tabulates every entry: plans of m = 16, 45 and 12 over one to three moduli, the exts 8 | 16, 9 | 45 and 4 | 12, the
tunnel chain 8 -> 12 -> 30 of tests/modswitch_ref.py, ptRound ladders with e = 1 .. 4 with and without an x_q, the ptTunnel
over the rings of tests/test_crtset_host.py, RingMul with K = 1 and K = 3, KHPRF left-spine and balanced trees, plain and
lifted; B in {0, 1, 3, 8}, ncs in {1, 2, 3}, base in {0, 2, 256}, every kind, and each entry's invalid arguments (null
handle, B < 0, an unrelated plan).  The golden file was recorded by running this module as a script
(python tests/test_work_len_host.py) against a build of the commit before the layouts moved into Work."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "work_len.json")
BS, NCS, BASES = (0, 1, 3, 8), (1, 2, 3), (0, 2, 256)
EXTS = ((8, 16), (9, 45), (4, 12))
CHAIN_BASES = (0, 2, 256)


def table(lolhip):
    import crtset_ref as cr
    import khprf_lifted_ref as klr
    import modswitch_ref as mr
    from oracle import lolmath as lm

    L = lolhip.lib()
    rows = {}
    keep = []                                                     # handles borrow their plans: alive until the end

    def put(key, v):
        assert key not in rows, key
        rows[key] = int(v)

    H = lambda x: None if x is None else x._h
    mk = lambda m, qs: lolhip.Plan.for_index(m, list(qs), host_only=True)
    vp = lambda vals: (C.c_void_p * max(len(vals), 1))(*vals)

    # ---- plans and exts: plan (m, T) is over the last T of the three moduli of its family's top index ------------------
    qs3, plans, exts = {}, {}, {}
    for lo, hi in EXTS:
        g = lm.good_qs(hi, 2 ** 29)
        qs3[hi] = [next(g) for _ in range(3)]
        for T in (1, 2, 3):
            plans[(hi, T)] = mk(hi, qs3[hi][3 - T:])
            exts[(lo, hi, T)] = lolhip.Ext(mk(lo, qs3[hi][3 - T:]), plans[(hi, T)])
    alien = plans[(45, 2)]                                        # unrelated to every m = 16 or m = 12 handle

    for (m, T), P in plans.items():
        tag = f"m{m}T{T}"
        for B in BS + (-1,):
            for ncs in NCS + (0,):
                put(f"decrypt {tag} ncs{ncs} B{B}", L.lolhip_decrypt_work_len(P._h, ncs, B))
            put(f"encrypt {tag} B{B}", L.lolhip_encrypt_work_len(P._h, B))
            for base in BASES + (1,):
                put(f"kshint {tag} base{base} B{B}", L.lolhip_kshint_work_len(P._h, base, B))
            for kind in (0, 1, 2, 3, -1):
                put(f"rlwe {tag} kind{kind} B{B}", L.lolhip_rlwe_work_len(P._h, kind, B))
            put(f"public {tag} B{B}", L.lolhip_public_work_len(P._h, None, B))
            for T2 in (1, 2, 3):
                for ncs in NCS + (0,):
                    put(f"modswitch {tag}->T{T2} ncs{ncs} B{B}", L.lolhip_modswitch_work_len(P._h, plans[(m, T2)]._h, ncs, B))
        put(f"modswitch {tag}->alien", L.lolhip_modswitch_work_len(P._h, (plans[(16, 2)] if m == 45 else alien)._h, 2, 1))
        put(f"modswitch {tag}->null", L.lolhip_modswitch_work_len(P._h, None, 2, 1))
    put("decrypt null", L.lolhip_decrypt_work_len(None, 1, 1))
    put("encrypt null", L.lolhip_encrypt_work_len(None, 1))
    put("kshint null", L.lolhip_kshint_work_len(None, 0, 1))
    put("rlwe null", L.lolhip_rlwe_work_len(None, 0, 1))
    put("public null", L.lolhip_public_work_len(None, None, 1))
    put("modswitch null", L.lolhip_modswitch_work_len(None, plans[(16, 1)]._h, 1, 1))

    for (lo, hi, T), X in exts.items():
        tag = f"{lo}|{hi}T{T}"
        for B in BS + (-1,):
            put(f"public {tag} B{B}", L.lolhip_public_work_len(plans[(hi, T)]._h, X._h, B))
            for base in BASES + (1,):
                put(f"tunnel {tag} base{base} B{B}", L.lolhip_tunnel_work_len(X._h, X._h, base, B))
        for base in BASES + (1,):
            put(f"tunnel_hint {tag} base{base}", L.lolhip_tunnel_hint_work_len(X._h, X._h, base))
        other = plans[(hi, 1 if T > 1 else 2)]                    # the ext does not end in this plan's moduli
        put(f"public {tag} unrelated", L.lolhip_public_work_len(other._h, X._h, 1))
        put(f"public {tag} alien", L.lolhip_public_work_len((plans[(16, T)] if hi == 45 else plans[(45, T)])._h, X._h, 1))
    X = exts[(4, 12, 2)]
    put("tunnel null er", L.lolhip_tunnel_work_len(None, X._h, 0, 1))
    put("tunnel null es", L.lolhip_tunnel_work_len(X._h, None, 0, 1))
    put("tunnel_hint null er", L.lolhip_tunnel_hint_work_len(None, X._h, 0))
    put("tunnel_hint null es", L.lolhip_tunnel_hint_work_len(X._h, None, 0))

    # ---- the tunnel chain 8 -> 12 -> 30 and its hops --------------------------------------------------------------------
    up = mr.chain_moduli()
    hops = []
    for r, s in zip(mr.CHAIN_MS[:-1], mr.CHAIN_MS[1:]):
        E, R, S = mk(math.gcd(r, s), up), mk(r, up), mk(s, up)
        hops.append((lolhip.Ext(E, R), lolhip.Ext(E, S)))
    p_in, p_out = mk(mr.CHAIN_MS[0], up[1:]), mk(mr.CHAIN_MS[-1], up[2:])
    er, es = [h[0]._h for h in hops], [h[1]._h for h in hops]
    fake = [8] * len(hops)                                        # borrowed device pointers: only stored by create
    for i, (xr, xs) in enumerate(hops):
        for base in BASES:
            put(f"tunnel_hint hop{i} base{base}", L.lolhip_tunnel_hint_work_len(xr._h, xs._h, base))
            for B in BS:
                put(f"tunnel hop{i} base{base} B{B}", L.lolhip_tunnel_work_len(xr._h, xs._h, base, B))
    put("tunnel_hint mismatched", L.lolhip_tunnel_hint_work_len(hops[0][0]._h, hops[1][1]._h, 2))
    put("tunnel mismatched", L.lolhip_tunnel_work_len(hops[0][0]._h, hops[1][1]._h, 2, 3))
    for base in CHAIN_BASES:
        h = C.c_void_p()
        assert L.lolhip_tunnel_chain_create(len(hops), vp(er), vp(es), vp(fake), vp(fake), base, p_in._h, p_out._h, C.byref(h)) == 0
        for B in BS + (-1,):
            put(f"chain base{base} B{B}", L.lolhip_tunnel_chain_work_len(h, B))
        L.lolhip_tunnel_chain_destroy(h)
    s_up, s_out = mk(30, up), mk(30, up[2:])
    h = C.c_void_p()
    assert L.lolhip_tunnel_chain_create(0, vp([]), vp([]), vp([]), vp([]), 2, s_up._h, s_out._h, C.byref(h)) == 0
    for B in BS + (-1,):
        put(f"chain nhops0 B{B}", L.lolhip_tunnel_chain_work_len(h, B))
    L.lolhip_tunnel_chain_destroy(h)
    put("chain null", L.lolhip_tunnel_chain_work_len(None, 1))

    # ---- ptRound ladders, m' = 16 with and without m = 8 under it -------------------------------------------------------
    for e in (1, 2, 3, 4):
        g = lm.good_qs(16, 2 ** 29)
        qs = [next(g) for _ in range(e + 1)]
        lv, ups = [mk(16, qs[i + 1:]) for i in range(e)], [mk(16, qs[i:]) for i in range(e - 1)]
        for with_x in (False, True):
            m_lo = 8 if with_x else 16
            pp = mk(m_lo, [2 ** e]) if e > 1 else None
            xq = [lolhip.Ext(mk(8, qs[i + 1:]), lv[i]) for i in range(min(e, 2))] if with_x else []
            keep.append((lv, ups, pp, xq))
            for base in BASES:
                h = C.c_void_p()
                rc = L.lolhip_ptround_create(e, 2 ** e, vp([p._h for p in lv]), vp([p._h for p in ups]), vp([8] * (e - 1)), base,
                                             H(pp), H(xq[0]) if xq else None, H(xq[1]) if len(xq) > 1 else None, C.byref(h))
                assert rc == 0, (e, with_x, base, rc)
                for B in BS + (-1,):
                    put(f"ptround e{e} x{int(with_x)} base{base} B{B}", L.lolhip_ptround_work_len(h, B))
                L.lolhip_ptround_destroy(h)
    put("ptround null", L.lolhip_ptround_work_len(None, 1))

    # ---- ptTunnel over 8 -> 28 -> 182 mod 2^3 ---------------------------------------------------------------------------
    rings, p, e = [8, 28, 182], 2, 3
    t = lolhip.PTTunnel.for_rings(rings, p, e, funcs=cr.tunnel_funcs(rings, p, e), host_only=True)
    for B in BS + (-1,):
        put(f"pt_tunnel B{B}", L.lolhip_pt_tunnel_work_len(t._h, B))
    put("pt_tunnel null", L.lolhip_pt_tunnel_work_len(None, 1))

    # ---- RingMul, K = 1 and K = 3 -----------------------------------------------------------------------------------------
    Ks = set()
    for m, qs in ((16, [256]), (45, [2 ** 40]), (64, [2 ** 16, 12289, 15]), (16, [2 ** 61 + 1])):
        rm = lolhip.RingMul(mk(m, qs))
        Ks.add(rm.K)
        for B in BS + (-1, 2 ** 31):
            put(f"ringmul m{m} T{rm.T} K{rm.K} B{B}", L.lolhip_ringmul_work_len(rm._h, B))
    assert {1, 3} <= Ks
    put("ringmul null", L.lolhip_ringmul_work_len(None, 1))

    # ---- KHPRF, plain and lifted ------------------------------------------------------------------------------------------
    trees = {"left": lolhip.left_spine_tree(5), "balanced": lolhip.balanced_tree(5)}
    for base in (2, 16):
        Pq = mk(32, [257])
        ell = Pq.decomposeLen(base)
        z = np.zeros((ell, Pq.n), dtype=np.int64)
        P8 = mk(32, [8])
        PQ = mk(32, [lm.first_good_q(32, klr.bound(32, 8, 2) + 1)])
        z8 = np.zeros((P8.decomposeLen(2), P8.n), dtype=np.int64)
        for name, tree in trees.items():
            fams = {"plain": lolhip.KHPRF(Pq, base, tree, z, z)}
            if base == 2:
                fams["lifted"] = lolhip.KHPRF.lifted(P8, PQ, 2, tree, z8, z8)
            for kind, f in fams.items():
                for x0 in (0, 5, 31):
                    for B in BS + (-1,):
                        put(f"khprf {kind} {name} base{base} x0={x0} B{B}", L.lolhip_khprf_work_len(f._h, x0, B))
                put(f"khprf {kind} {name} base{base} x0=-1", L.lolhip_khprf_work_len(f._h, -1, 1))
    put("khprf null", L.lolhip_khprf_work_len(None, 0, 1))
    return rows


def test_every_work_len_equals_the_recorded_value(lolhip):
    got = table(lolhip)
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff
    assert sum(v > 0 for v in got.values()) > 500 and sum(v < 0 for v in got.values()) > 100


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import lol_amd
    with open(GOLDEN, "w") as fh:
        json.dump(table(lol_amd), fh, indent=0, sort_keys=True)
        fh.write("\n")
