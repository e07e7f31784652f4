"""Every handle gives its device memory back (lol_amd/csrc/devmem.h: each table is a DevBuf of its handle, destroy is
delete).  Per handle kind: build and drop once as a warm-up, read the free HBM, build and drop 16 more times, and the
free figure is the same word for word — the precedent of test_short_lived_host_threads_leave_nothing_behind.

What one cycle builds is what a caller builds: the handle with the plans and exts under it, so every cycle allocates
and frees well over 1 MiB (a PTRound or RingMul handle alone owns a few KiB or nothing).  The parameter sets are those
of the feature tests: the moduli come from lm.good_qs / lm.first_good_q exactly as there.

What the figure can see, measured once on an MI355X (profiles/devmem_refactor_evidence.txt): it moves in steps of
2 MiB.  Sixteen handles kept alive lower it by 2 MiB (the ext without device tables: its `lo` plans) up to 118 MiB (the
m = 2^14 plan), every kind by at least 2 MiB; sixteen 48 KiB tables alone (PTRound handles over shared plans) do not
move it.  So a leaked table shows once 16 copies of it take the runtime into another 2 MiB block, which the tables of
1 MiB and more do at once and the small ones need not.  The figures are equal on the commit before devmem.h too, whose
hand-written frees did not leak on these paths.

No create can fail after its first upload other than by a HIP error (every validation comes first), and none is
provoked: there is no failed-create case.  lolhip_ext_create over a device `lo` and a host-only `hi` returns OK with
no device table; it is cycled like the others.
"""
import numpy as np
import pytest

import crtset_ref as cr
import khprf_lifted_ref as klr
from oracle import lolmath as lm

pytestmark = pytest.mark.gpu

CYCLES = 16


def _qs(m, lower, T):
    g = lm.good_qs(m, lower)
    return [next(g) for _ in range(T)]


def _plan_pow2(gpu):
    """m = 2^14, T = 4, moduli below 2^27: the consts and the 2-power tables in both widths"""
    qs = _qs(2 ** 14, 2 ** 20, 4)
    assert max(qs) < 2 ** 27
    return lambda: gpu.Plan.for_index(2 ** 14, qs)


def _plan_fused(gpu):
    """m = 64 * 27, T = 2: the fused, merged and big programs, the Montgomery pool and its 32-bit copy"""
    qs = _qs(64 * 27, 2 ** 20, 2)
    return lambda: gpu.Plan.for_index(64 * 27, qs)


def _plan_float(gpu):
    """m = 2^13 * 3 (n = 8192): the constant pools of the CRT over C and of gaussianDec"""
    m = 2 ** 13 * 3
    qs = [lm.first_good_q(m, 1000)]
    return lambda: gpu.Plan.for_index(m, qs)


def _ext(gpu):
    """2^6 | 64 * 27 with a CRT basis on both sides: the six index tables and twaceCRT's tweak vector"""
    qs = _qs(64 * 27, 2 ** 20, 2)

    def make():
        x = gpu.Ext(gpu.Plan.for_index(64, qs), gpu.Plan.for_index(64 * 27, qs))
        assert x.lo.has_crt and x.hi.has_crt
        return x
    return make


def _ext_mixed_residency(gpu):
    """a device `lo` under a host-only `hi`: a handle without device tables"""
    qs = _qs(64 * 27, 2 ** 20, 2)
    return lambda: gpu.Ext(gpu.Plan.for_index(64, qs), gpu.Plan.for_index(64 * 27, qs, host_only=True))


def _khprf(gpu):
    """m = 256, q ~ 2^29, BaseBGad 2, k = 3 leaves: the leaves and their L-fold digit table (1.8 MiB)"""
    m, base = 256, 2
    q = lm.first_good_q(m, 2 ** 29)
    rng = np.random.default_rng(0)

    def make():
        P = gpu.Plan.for_index(m, [q])
        a0, a1 = (rng.integers(0, q, size=(P.decomposeLen(base), P.n), dtype=np.int64) for _ in range(2))
        return gpu.KHPRF(P, base, gpu.balanced_tree(3), a0, a1)
    return make


def _khprf_lifted(gpu):
    """m = 8*5*7*13, q = 8, BaseBGad 2, k = 3 leaves: the three leaf tables of the lifted family"""
    m, q, base = 8 * 5 * 7 * 13, 8, 2
    Q = lm.first_good_q(m, max(klr.bound(m, q, base) + 1, 2 ** 30))
    rng = np.random.default_rng(1)

    def make():
        Pq, PQ = gpu.Plan.for_index(m, [q]), gpu.Plan.for_index(m, [Q])
        a0, a1 = (rng.integers(0, q, size=(Pq.decomposeLen(base), Pq.n), dtype=np.int64) for _ in range(2))
        return gpu.KHPRF.lifted(Pq, PQ, base, gpu.balanced_tree(3), a0, a1)
    return make


def _pt_tunnel(gpu):
    """16 -> 56 -> 364 over Z_8: two hops, one function table each"""
    rings, p, e = [16, 56, 364], 2, 3
    funcs = cr.tunnel_funcs(rings, p, e)
    return lambda: gpu.PTTunnel.for_rings(rings, p, e, funcs=funcs)


def _ptround(gpu):
    """m = m' = 2048, p = 8 (e = 3): the constants' source table; creation keeps the hints' addresses and reads nothing"""
    import torch
    m, p, base = 2048, 8, 0
    e = p.bit_length() - 1
    moduli = _qs(m, 2 ** 29, e + 1)
    pps = lm.factor_pps(m)
    hints = []

    def make():
        plans = [gpu.Plan(pps, moduli[i + 1:]) for i in range(e)]
        ups = [gpu.Plan(pps, moduli[i:]) for i in range(e - 1)]
        if not hints:                                    # made once: torch's allocator stays out of the cycles
            hints.extend(torch.zeros((U.decomposeLen(base), 2, U.n, U.T), dtype=torch.int64, device="cuda") for U in ups)
        return gpu.PTRound(plans, ups, hints, base, p)
    return make


def _ringmul(gpu):
    """m = 16384 over q = 2^32: the handle owns no table, its two plans do"""
    pps = lm.factor_pps(16384)
    return lambda: gpu.RingMul(gpu.Plan(pps, [2 ** 32]))


KINDS = [_plan_pow2, _plan_fused, _plan_float, _ext, _ext_mixed_residency, _khprf, _khprf_lifted, _pt_tunnel, _ptround,
         _ringmul]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__.lstrip("_"))
def test_create_destroy_cycles_leave_free_memory_unchanged(gpu, kind):
    import torch
    make = kind(gpu)

    def cycle():
        h = make()
        del h
        torch.cuda.synchronize()

    cycle()                                              # warm-up: what the runtime keeps per first use is kept now
    free = torch.cuda.mem_get_info()[0]
    for _ in range(CYCLES):
        cycle()
    print(f"{kind.__name__}: free {free} -> {torch.cuda.mem_get_info()[0]}")
    assert torch.cuda.mem_get_info()[0] == free
