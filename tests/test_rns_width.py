"""Wide and mixed-width RNS tuples, and batches that outlast the grid, on the GPU (-m gpu).

Every expected value comes from the oracle (oracle.CpuRef, oracle/she_ref.py, oracle/she_model.py, tests/enc_ref.py)
or from a bit-exact equality between two device routes; none from the kernel under test.

    wide tuples          T = 5, 8, 16 and one plan at T = 64 through every transform, at m = 2^6, 2^11 and the mixed
                         indices 45, 1575, 15015; B = 1 and 5 (ragged last workgroup), B = 8 for the component remap
    mixed widths         tuples with a modulus from every arithmetic class (below 2^27, either side of 13 (q-1)^2 = 2^64,
                         below 2^31 and 2^32, either side of 2^61), largest first and smallest first; extreme residues
    pipelines            ctMulCRT, decompose / gadget, knapsack, keySwitch (fused m = 2^k, fused mixed-radix, three
                         launches), rescaleDropFirst, evalLin, tunnel, encrypt / errorTerm / decrypt at T = 5, 8, 16;
                         every pipeline refuses T = 17 before it launches
    grid-stride loops    k_mixed, k_generic, k_mixed_keyswitch and the encrypt samplers at batches whose work items
                         exceed the grid cap by more than one sweep: the rows at the sweep boundaries against the
                         oracle, a size-independent property over the whole batch
"""
import math

import numpy as np
import pytest

import enc_ref as er
from oracle import lolmath as lm
from oracle import she_model as sm
from oracle import she_ref as sr
from oracle.oracle import Params
from params import PLAN_NAME, PRIME_OPS
from test_decrypt import _gpu_checks
from test_encrypt import _rep, _restated_e, _small_key
from test_rns_width_host import good_below, mixed16, mixed_moduli

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
GRID_CAP = 65536                     # workgroups of k_mixed / k_generic / k_mixed_keyswitch
GRID_Y_CAP = 65535                   # grid.y of the encrypt samplers


def _qs(m, lower, T):
    g = lm.good_qs(m, lower)
    return [next(g) for _ in range(T)]


def _extreme(R, rng, B):
    """[B][n][T] with q - 1 everywhere (row 0), alternating 0 / q - 1 (row 1), random rows after"""
    qv = np.array(R.qs, dtype=np.int64)
    y = R.random(rng, B)
    y[0] = qv - 1
    if B > 1:
        y[1] = 0
        y[1, ::2] = qv - 1
    return y


def _neg(y, qs):
    """the same residues as representatives in (-q, 0]"""
    return np.where(y > 0, y - np.asarray(qs, dtype=np.int64), 0)


def _transforms(P, R, cpuref, y, z, tag):
    for op in ("crt", "crtinv") + PRIME_OPS:
        got, want = getattr(P, PLAN_NAME[op])(y), getattr(cpuref, op)(R, y)
        assert (got is None) == (want is None), (op, tag)
        if want is not None:
            assert np.array_equal(got, want), (op, tag)
    assert np.array_equal(P.mul(y, z), cpuref.mul(R, y, z)), tag
    assert np.array_equal(P.polymul(y, z), cpuref.polymul(R, y, z)), tag
    assert np.array_equal(P.polymul(y, y), cpuref.polymul(R, y, y)), (tag, "square")
    assert np.array_equal(P.mulGCRT(y), cpuref.crt(R, cpuref.gpow(R, cpuref.crtinv(R, y)))), tag
    assert np.array_equal(P.divGCRT(P.mulGCRT(y)), y), tag


# ---------------------------------------------------------------------------------------------
# 1. wide tuples through the transforms
# ---------------------------------------------------------------------------------------------
WIDE = [(64, 5, 2 ** 59), (64, 16, 2 ** 20), (2048, 5, 2 ** 26), (2048, 8, 2 ** 29), (2048, 16, 2 ** 60),
        (45, 5, 2 ** 30), (45, 8, 2 ** 26), (45, 16, 2 ** 60), (1575, 8, 2 ** 29), (1575, 16, 2 ** 20),
        (15015, 5, 2 ** 45), (15015, 16, 2 ** 29)]


@pytest.mark.parametrize("m,T,lower", WIDE)
def test_wide_tuple_transforms(gpu, cpuref, m, T, lower):
    pps, qs = lm.factor_pps(m), _qs(m, lower, T)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    rng = np.random.default_rng(m * 100 + T)
    batches = (1, 5, 8) if m == 2048 and T >= 8 else (1, 5)     # B % 8 == 0: the XCD component remap of k_pow2
    for B in batches:
        y, z = _extreme(R, rng, B), R.random(rng, B)
        _transforms(P, R, cpuref, y, z, (m, T, B))
        assert np.array_equal(P.crt(_neg(y, qs)), cpuref.crt(R, y)), (m, T, B, "negative")


@pytest.mark.parametrize("m,lower", [(64, 2 ** 40), (45, 2 ** 29)])
def test_plan_at_64_moduli(gpu, cpuref, m, lower):
    """the plan limit: 64 moduli at a small n"""
    pps, qs = lm.factor_pps(m), _qs(m, lower, 64)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    rng = np.random.default_rng(64 + m)
    for B in (1, 3):
        _transforms(P, R, cpuref, _extreme(R, rng, B), R.random(rng, B), (m, 64, B))


# ---------------------------------------------------------------------------------------------
# 2. mixed-width tuples through the transforms
# ---------------------------------------------------------------------------------------------
def _mixed(m, kind):
    if kind == "ascending":
        return mixed_moduli(m)
    if kind == "descending":
        return sorted(mixed_moduli(m), reverse=True)
    return mixed16(m)


@pytest.mark.parametrize("m", [64, 2048, 45, 1575, 15015])
@pytest.mark.parametrize("kind", ["ascending", "descending", "mixed16"])
def test_mixed_width_transforms(gpu, cpuref, m, kind):
    pps, qs = lm.factor_pps(m), _mixed(m, kind)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    rng = np.random.default_rng(m + len(kind))
    for B in (1, 5):
        y, z = _extreme(R, rng, B), _extreme(R, rng, B)[::-1].copy()
        _transforms(P, R, cpuref, y, z, (m, kind, B))
        assert np.array_equal(P.crt(_neg(y, qs)), cpuref.crt(R, y)), (m, kind, B, "negative")
        assert np.array_equal(P.polymul(_neg(y, qs), _neg(z, qs)), cpuref.polymul(R, y, z)), (m, kind, B, "negative")


# ---------------------------------------------------------------------------------------------
# 3. every SymmSHE pipeline at T = 5, 8, 16 and at mixed widths
# ---------------------------------------------------------------------------------------------
# (m, name, moduli): the fused m = 2^k key switch needs every q < 2^30, the fused mixed-radix one class 2 (u16 at 45) or
# class 4 (u8 at 45); decompose runs its Q32 kernel below 2^31, knapsack its Q32 kernel below 2^29
PIPE = [(64, "u5", lambda m: _qs(m, 2 ** 20, 5)), (64, "u8", lambda m: _qs(m, 2 ** 29, 8)),
        (64, "u16", lambda m: _qs(m, 2 ** 26, 16)), (45, "u8", lambda m: _qs(m, 2 ** 20, 8)),
        (45, "u16", lambda m: _qs(m, 2 ** 29, 16)), (45, "u5_59", lambda m: _qs(m, 2 ** 59, 5)),
        (64, "ascending", mixed_moduli), (45, "descending", lambda m: sorted(mixed_moduli(m), reverse=True)),
        (64, "mixed16", mixed16)]
PIPE_IDS = [f"{m}-{nm}" for m, nm, _ in PIPE]


def _pipe(gpu, m, mk):
    pps, qs = lm.factor_pps(m), mk(m)
    return gpu.Plan(pps, qs), Params(pps, qs), qs


@pytest.mark.parametrize("m,name,mk", PIPE, ids=PIPE_IDS)
def test_wide_ctmul(gpu, cpuref, m, name, mk):
    P, R, qs = _pipe(gpu, m, mk)
    rng = np.random.default_rng(m + 1)
    for B in (1, 5):
        ops = [_extreme(R, rng, B) for _ in range(4)]
        want = sr.ctmul_crt(cpuref, R, *ops)
        for g_, w in zip(P.ctMulCRT(*ops), want):
            assert np.array_equal(g_, w), (name, B)
        for g_, w in zip(P.ctMulCRT(*[_neg(o, qs) for o in ops]), want):
            assert np.array_equal(g_, w), (name, B, "negative")


@pytest.mark.parametrize("m,name,mk", PIPE, ids=PIPE_IDS)
@pytest.mark.parametrize("base", [0, 2, 3, 256, 2 ** 20])
def test_wide_decompose_and_gadget(gpu, m, name, mk, base):
    P, R, qs = _pipe(gpu, m, mk)
    rng = np.random.default_rng(base % 97 + m)
    c = _extreme(R, rng, 3)
    qv = np.array(qs, dtype=np.int64)
    c[2, 0], c[2, 1] = qv // 2, qv // 2 - 1                      # the lift's break point
    assert P.decomposeLen(base) == sum(sr.digit_counts(R, base))
    assert np.array_equal(P.gadget(base), sr.gadget(R, base))
    want = sr.decompose(R, c, base)
    assert np.array_equal(P.decompose(c, base), want), (name, base)
    assert np.array_equal(P.decompose(_neg(c, qs), base), want), (name, base, "negative")


@pytest.mark.parametrize("qs", [[1017857, 1032193], [good_below(16, 2 ** 31), good_below(16, 2 ** 27)],
                                [good_below(16, 2 ** 61), 1032193], [lm.first_good_q(16, 2 ** 61), good_below(16, 2 ** 32)]])
def test_decompose_t2_with_an_8_byte_aligned_digit_slab(gpu, qs):
    """T = 2 stores each digit row as one 16-byte pair only when the digit slab is 16-byte aligned: at an 8-byte-aligned
    slab the general store runs, in the Q32 kernel and the general one; nothing lands outside the slab"""
    import torch
    pps = [(2, 4)]
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    rng = np.random.default_rng(qs[0] % 1000)
    B = 3
    c = _extreme(R, rng, B)
    for base in (0, 2, 256):
        L = P.decomposeLen(base)
        want = sr.decompose(R, c, base)
        dc = torch.from_numpy(c).cuda()
        SENT = 0x5A5A5A5A
        pad = torch.full((L * B * R.n * 2 + 2,), SENT, dtype=torch.int64, device="cuda")
        out = pad[1:-1]
        assert out.data_ptr() % 16 == 8
        assert gpu.lib().lolhip_decompose_batch(P._h, None, dc.data_ptr(), base, out.data_ptr(), B) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.view(L, B, R.n, 2).cpu().numpy(), want), (qs, base)
        assert int(pad[0]) == SENT and int(pad[-1]) == SENT
        assert np.array_equal(P.decompose(c, base), want), (qs, base, "aligned")


@pytest.mark.parametrize("m,name,mk", PIPE, ids=PIPE_IDS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_wide_knapsack(gpu, cpuref, m, name, mk, K):
    P, R, qs = _pipe(gpu, m, mk)
    rng = np.random.default_rng(K * 7 + m)
    B, L = 3, 4
    qv = np.array(qs, dtype=np.int64)
    xs = np.stack([_extreme(R, rng, B) for _ in range(L)])
    hint = np.stack([np.stack([R.random(rng, 1)[0] for _ in range(K)]) for _ in range(L)])
    hint[0, 0] = qv - 1
    add = np.stack([R.random(rng, B) for _ in range(K)])
    want = sr.knapsack(cpuref, R, xs, hint)
    assert np.array_equal(P.knapsack(xs, hint), want), name
    wadd = ((want.astype(object) + add) % np.array(qs, dtype=object)).astype(np.int64)
    assert np.array_equal(P.knapsack(_neg(xs, qs), _neg(hint, qs), addend=add), wadd), (name, "negative")


@pytest.mark.parametrize("m,name,mk", PIPE, ids=PIPE_IDS)
@pytest.mark.parametrize("base", [0, 2, 256])
def test_wide_keyswitch(gpu, cpuref, m, name, mk, base):
    """against the restatement and against the three-launch route (KEYSWITCH_UNFUSED)"""
    P, R, qs = _pipe(gpu, m, mk)
    rng = np.random.default_rng(base + m)
    B, Ld = 2, sum(sr.digit_counts(R, base))
    qv = np.array(qs, dtype=np.int64)
    c2 = _extreme(R, rng, B)
    c2[1, 0] = qv // 2
    hint = np.stack([np.stack([R.random(rng, 1)[0] for _ in range(2)]) for _ in range(Ld)])
    add = np.stack([R.random(rng, B) for _ in range(2)])
    want = sr.keyswitch(cpuref, R, c2, base, hint)
    wadd = ((want.astype(object) + add) % np.array(qs, dtype=object)).astype(np.int64)
    assert np.array_equal(P.keySwitch(c2, base, hint), want), (name, base)
    fused = P.keySwitch(_neg(c2, qs), base, _neg(hint, qs), addend=_neg(add, qs))
    assert np.array_equal(fused, wadd), (name, base, "addend, negative")
    gpu.debug_set("KEYSWITCH_UNFUSED", True)
    try:
        assert np.array_equal(P.keySwitch(c2, base, hint, addend=add), wadd), (name, base, "three launches")
    finally:
        gpu.debug_set("KEYSWITCH_UNFUSED", False)


def _rescale_tuples(m):
    return [("q0 >> qs", [lm.first_good_q(m, 2 ** 61)] + _qs(m, 2 ** 20, 4)),   # |lift q_0| far beyond every other q_s
            ("q0 >> qs, mixed", sorted(mixed_moduli(m), reverse=True)),
            ("q0 << qs", [good_below(m, 2 ** 27)] + _qs(m, 2 ** 59, 4)),
            ("q0 << qs, mixed", mixed_moduli(m)),
            ("T = 16", _qs(m, 2 ** 40, 16)),
            ("T = 16, mixed", mixed16(m))]


@pytest.mark.parametrize("m", [64, 45])
@pytest.mark.parametrize("i", range(6))
def test_wide_rescale(gpu, m, i):
    name, qs = _rescale_tuples(m)[i]
    pps = lm.factor_pps(m)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    rng = np.random.default_rng(i + m)
    c = _extreme(R, rng, 5)
    qv = np.array(qs, dtype=np.int64)
    c[2, 0], c[2, 1] = qv // 2, qv // 2 - 1
    c[3, :, 0] = qv[0] // 2 + rng.integers(0, 2, size=R.n)      # |lift a| at its largest
    want = sr.rescale_drop_first(R, c)
    assert np.array_equal(P.rescaleDropFirst(c), want), name
    assert np.array_equal(P.rescaleDropFirst(_neg(c, qs)), want), (name, "negative")


EXT_WIDE = [(4, 12, 12, 13, 4), (3, 21, 21, 43, 4), (4, 12, 20, 61, 5), (8, 16, 40, 241, 3), (4, 12, 12, 13, 16)]


def _ext_setup(gpu, e, r, s, q, T):
    qs = [q] + _qs(r * s // math.gcd(r, s), q, T - 1)
    pe, pr, ps = (lm.factor_pps(x) for x in (e, r, s))
    PE, PR, PS = (Params(p_, qs) for p_ in (pe, pr, ps))
    GE, GR, GS = (gpu.Plan(p_, qs) for p_ in (pe, pr, ps))
    return qs, (PE, PR, PS), (gpu.Ext(GE, GR), gpu.Ext(GE, GS))


@pytest.mark.parametrize("e,r,s,q,T", EXT_WIDE)
def test_wide_evallin(gpu, cpuref, e, r, s, q, T):
    qs, (PE, PR, PS), (XR, XS) = _ext_setup(gpu, e, r, s, q, T)
    rng = np.random.default_rng(r + s + T)
    x = _extreme(PR, rng, 3)
    ys = np.stack([PS.random(rng, 1)[0] for _ in range(PR.n // PE.n)])
    assert np.array_equal(XR.evalLin(XS, x, ys), sr.evallin(cpuref, PE, PR, PS, x, ys))


@pytest.mark.parametrize("e,r,s,q,T", EXT_WIDE)
@pytest.mark.parametrize("base", [0, 16])
def test_wide_tunnel(gpu, cpuref, e, r, s, q, T, base):
    qs, (PE, PR, PS), (XR, XS) = _ext_setup(gpu, e, r, s, q, T)
    rng = np.random.default_rng(r + s + T + base)
    B, rel, L = 2, PR.n // PE.n, sum(sr.digit_counts(PS, base))
    c0, c1 = _extreme(PR, rng, B), PR.random(rng, B)
    ys = np.stack([PS.random(rng, 1)[0] for _ in range(rel)])
    hints = np.stack([np.stack([np.stack([PS.random(rng, 1)[0] for _ in range(2)]) for _ in range(L)]) for _ in range(rel)])
    got = XR.tunnel(XS, c0, c1, ys, hints, base)
    assert np.array_equal(got, sr.tunnel(cpuref, PE, PR, PS, c0, c1, ys, hints, base))


# (m, m', p, moduli)
ENC_WIDE = [(64, 64, 257, _qs(64, 2 ** 29, 8)), (2048, 2048, 16, _qs(2048, 2 ** 20, 16)),
            (45, 45, 7, _qs(45, 2 ** 29, 16)), (16, 1024, 8, _qs(1024, 2 ** 59, 8)), (64, 64, 5, mixed16(64))]


@pytest.mark.parametrize("m,m2,p,qs", ENC_WIDE)
def test_wide_encrypt_matches_restatement_and_decrypts(gpu, cpuref, m, m2, p, qs):
    pq, pp = gpu.Plan.for_index(m2, qs), gpu.Plan.for_index(m2, [p])
    x_p = None if m == m2 else gpu.Ext(gpu.Plan.for_index(m, [p]), pp)
    n_m = pp.n if x_p is None else x_p.lo.n
    n, T = pq.n, len(qs)
    rng = np.random.default_rng(m2 + T)
    B, svar, ctr = 3, 1.5, 77 + m2
    key = rng.bytes(32)
    pt = rng.integers(-p + 1, p, size=(B, n_m), dtype=np.int64)
    s_crt = _small_key(cpuref, m2, qs, rng)
    out_crt = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, ext=x_p, out_crt=True)
    out_pow = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, ext=x_p)
    assert np.array_equal(out_crt[1], er.uniform_crt(key, ctr, B, n, qs))
    P = Params(lm.factor_pps(m2), qs)
    for i in range(2):
        assert np.array_equal(out_pow[i], cpuref.crtinv(P, out_crt[i]).reshape(B, n, T)), i
    rep = _rep(cpuref, m, m2, p, pt)
    e_want, near = _restated_e(m2, p, svar, key, ctr, B, rep)
    e_pow = pq.errorTerm(out_pow, s_crt, p)
    assert np.array_equal(e_pow, pq.errorTerm(out_crt, s_crt, p, cs_crt=True))
    bad = e_pow != e_want
    assert bad.sum() <= 4 and near[bad].all(), (int(bad.sum()), int(near.sum()))
    want = pt % p
    assert np.array_equal(pq.decrypt(out_pow, s_crt, pp, ext=x_p), want)
    assert np.array_equal(pq.decrypt(out_crt, s_crt, pp, ext=x_p, cs_crt=True), want)


# every T in 1 .. 16 at m = 64, p = 257 (each k_lift<T, PMODE> instantiation decrypts once), with the smaller of
# 2^20 / 2^29 as the moduli's lower bound at which the model itself decrypts every step it runs (checked on the host:
# 2^20 from T = 2 on, 2^29 for the product at T = 1)
WIDE_DEC = [(64, 257, 2 ** 29, 8), (64, 257, 2 ** 20, 16), (45, 181, 2 ** 30, 8), (45, 181, 2 ** 59, 16),
            (64, 257, 2 ** 29, 1)] + [(64, 257, 2 ** 20, T) for T in range(2, 16) if T != 8]


@pytest.mark.parametrize("m,p,lower,T", WIDE_DEC)
def test_wide_decrypt_matches_model(gpu, cpuref, m, p, lower, T):
    """the flow of test_decrypt_matches_model: fresh, MSD, ct x ct, keySwitchQuadCirc, modSwitch.  One modulus ends
    after ct x ct: its only (TrivGad) hint digit carries noise of the size of q, which the model cannot decrypt at
    2^20 or at 2^29 either, and modSwitch needs a second modulus to drop."""
    pps = lm.factor_pps(m)
    qs = _qs(m, lower, T)
    rng = np.random.default_rng(5000 + m + T)
    eng = lambda qs_: sm.CpuEngine(cpuref, Params(pps, qs_))
    she = sm.SHE(eng(qs), eng([p]), qs, p, rng)
    she.keygen()
    pq, pp = gpu.Plan(pps, qs), gpu.Plan(pps, [p])
    B = 2
    pt1 = rng.integers(0, p, size=(B, she.n), dtype=np.int64)
    pt2 = rng.integers(0, p, size=(B, she.n), dtype=np.int64)
    ct1, ct2 = she.encrypt(pt1), she.encrypt(pt2)
    _gpu_checks(she, pq, pp, ct1, pt1)
    _gpu_checks(she, pq, pp, she.toMSD(ct1), pt1)
    prod_ = she.mul(ct1, ct2)
    want = cpuref.polymul(Params(pps, [p]), pt1[..., None], pt2[..., None]).reshape(pt1.shape)
    _gpu_checks(she, pq, pp, prod_, want)
    if T == 1:
        return
    _gpu_checks(she, pq, pp, she.key_switch_quad(she.ks_quad_hint(0), 0, prod_), want)
    small, she2 = she.mod_switch_drop_first(ct1, eng(qs[1:]))
    _gpu_checks(she2, gpu.Plan(pps, qs[1:]), pp, small, pt1)


def test_every_pipeline_refuses_17_moduli(gpu):
    """PIPE_MAX_T = 16: every pipeline entry point refuses T = 17 with LOLHIP_ERR_INVALID before it launches, so its
    output stays untouched (test_every_pipeline_runs_at_16_moduli: the same calls at T = 16 run)"""
    import torch
    L = gpu.lib()
    SENT = 0x5A5A5A5A
    T, B = 17, 2
    qs = _qs(48, 2 ** 20, T)                                      # = 1 (mod 48): the extensions 4 -> 16, 4 -> 48 as well
    pq, pp = gpu.Plan.for_index(16, qs), gpu.Plan.for_index(16, [5])
    GE, GR, GS = (gpu.Plan.for_index(x, qs) for x in (4, 16, 48))
    XR, XS = gpu.Ext(GE, GR), gpu.Ext(GE, GS)
    n, rel = pq.n, GR.n // GE.n
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    sent = lambda *shape: torch.full(shape, SENT, dtype=torch.int64, device="cuda")
    work = z(1 << 16)
    a = [z(B, n, T) for _ in range(4)]
    s_crt, hint = z(n, T), z(T, 2, n, T)
    out = {"ctmul": sent(3, B, n, T), "decompose": sent(T, B, n, T), "knapsack": sent(1, B, n, T),
           "keyswitch": sent(2, B, n, T), "rescale": sent(B, n, T - 1), "errorterm": sent(B, n), "decrypt": sent(B, n),
           "encrypt": sent(2, B, n, T), "evallin": sent(B, GS.n, T), "tunnel": sent(2, B, GS.n, T)}
    e = out["ctmul"]
    rc = {
        "ctmul": L.lolhip_ctmul_crt_batch(pq._h, None, *[x.data_ptr() for x in a], e[0].data_ptr(), e[1].data_ptr(),
                                          e[2].data_ptr(), B),
        "decompose": L.lolhip_decompose_batch(pq._h, None, a[0].data_ptr(), 0, out["decompose"].data_ptr(), B),
        "knapsack": L.lolhip_knapsack_batch(pq._h, None, a[0].data_ptr(), 1, hint.data_ptr(), 1, None,
                                            out["knapsack"].data_ptr(), B),
        "keyswitch": L.lolhip_keyswitch_batch(pq._h, None, a[0].data_ptr(), 0, hint.data_ptr(), 2, None,
                                              out["keyswitch"].data_ptr(), work.data_ptr(), B),
        "rescale": L.lolhip_rescale_drop_batch(pq._h, None, a[0].data_ptr(), out["rescale"].data_ptr(), B),
        "errorterm": L.lolhip_error_term_batch(pq._h, None, a[0].data_ptr(), 2, 0, s_crt.data_ptr(), 0, 5,
                                               out["errorterm"].data_ptr(), work.data_ptr(), B),
        "decrypt": L.lolhip_decrypt_batch(pq._h, pp._h, None, None, a[0].data_ptr(), 2, 0, s_crt.data_ptr(), 0, 0, 1,
                                          out["decrypt"].data_ptr(), work.data_ptr(), B),
        "encrypt": L.lolhip_encrypt_batch(pq._h, pp._h, None, None, z(B, n).data_ptr(), s_crt.data_ptr(), 1.0, bytes(32), 0,
                                          0, out["encrypt"].data_ptr(), work.data_ptr(), B),
        "evallin": L.lolhip_evallin_batch(XR._h, XS._h, None, z(B, GR.n, T).data_ptr(), z(rel, GS.n, T).data_ptr(),
                                          out["evallin"].data_ptr(), work.data_ptr(), B),
        "tunnel": L.lolhip_tunnel_batch(XR._h, XS._h, None, z(B, GR.n, T).data_ptr(), z(B, GR.n, T).data_ptr(),
                                        z(rel, GS.n, T).data_ptr(), z(rel, T, 2, GS.n, T).data_ptr(), 0,
                                        out["tunnel"].data_ptr(), work.data_ptr(), B),
    }
    torch.cuda.synchronize()
    for k, v in out.items():
        assert rc[k] == ERR_INVALID, (k, rc[k])
        assert bool((v == SENT).all()), k
    for f in (pq.decomposeLen, pq.gadget):
        with pytest.raises(gpu.LolHipError) as ei:
            f(0)
        assert ei.value.code == ERR_INVALID


def test_every_pipeline_runs_at_16_moduli(gpu):
    """the counterpart of the refusals: the same entry points accept T = 16"""
    import torch
    L = gpu.lib()
    qs = _qs(48, 2 ** 20, 16)
    pq, pp = gpu.Plan.for_index(16, qs), gpu.Plan.for_index(16, [5])
    n, B, T = pq.n, 2, 16
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    work = z(max(1 << 16, L.lolhip_decrypt_work_len(pq._h, 2, B)))
    a, s_crt = z(B, n, T), z(n, T)
    e = z(3, B, n, T)
    assert L.lolhip_ctmul_crt_batch(pq._h, None, a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), e[0].data_ptr(),
                                    e[1].data_ptr(), e[2].data_ptr(), B) == 0
    assert L.lolhip_knapsack_batch(pq._h, None, a.data_ptr(), 1, z(1, 1, n, T).data_ptr(), 1, None, e.data_ptr(), B) == 0
    assert L.lolhip_rescale_drop_batch(pq._h, None, a.data_ptr(), z(B, n, T - 1).data_ptr(), B) == 0
    assert L.lolhip_error_term_batch(pq._h, None, z(2, B, n, T).data_ptr(), 2, 0, s_crt.data_ptr(), 0, 5, z(B, n).data_ptr(),
                                     work.data_ptr(), B) == 0
    GE, GR, GS = (gpu.Plan.for_index(x, qs) for x in (4, 16, 48))
    XR, XS = gpu.Ext(GE, GR), gpu.Ext(GE, GS)
    rel = GR.n // GE.n
    assert L.lolhip_evallin_batch(XR._h, XS._h, None, z(B, GR.n, T).data_ptr(), z(rel, GS.n, T).data_ptr(),
                                  z(B, GS.n, T).data_ptr(), work.data_ptr(), B) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 4. grid-stride loops: a second and a third sweep
# ---------------------------------------------------------------------------------------------
def _need_hbm(gb):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 1e9:
        pytest.skip(f"needs {gb} GB of free HBM")


def _boundary_items(items):
    return sorted({i for i in (0, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, 2 * GRID_CAP, items - 1) if i < items})


def _rows_of_items(items_idx, T, ppw, B):
    """the polynomials work item i = group * T + t touches: group i // T, polynomials group * ppw ..."""
    rows = set()
    for i in items_idx:
        g = i // T
        rows.update(range(g * ppw, min((g + 1) * ppw, B)))
    return sorted(rows)


def _ppw(n, B):
    ppw = 1
    while ppw * 2 * n <= 2048 and ppw * 2 <= B:
        ppw *= 2
    return ppw


# (m, T, lower, polynomials per workgroup, groups): k_mixed at n = 2048 (one polynomial per workgroup) and at m = 45
# (64 packed polynomials per group, a ragged last group); k_generic at m = 89 (16 per group)
GRID = [(6144, 2, 2 ** 29, 70000), (45, 2, 2 ** 29, 64 * 70000 + 17), (89, 2, 2 ** 29, 16 * 70000 + 5)]


@pytest.mark.parametrize("m,T,lower,B", GRID)
def test_grid_stride_transforms(gpu, cpuref, m, T, lower, B):
    import torch
    pps, qs = lm.factor_pps(m), _qs(m, lower, T)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    ppw = _ppw(R.n, B)
    items = -(-B // ppw) * T
    assert items > 2 * GRID_CAP
    _need_hbm(3.3 * B * R.n * T * 8 / 1e9 + 1)
    rows = _rows_of_items(_boundary_items(items), T, ppw, B)
    g = torch.Generator(device="cuda"); g.manual_seed(m)
    qv = torch.tensor(qs, dtype=torch.int64, device="cuda")
    a = torch.stack([torch.randint(0, q, (B, R.n), dtype=torch.int64, device="cuda", generator=g) for q in qs], dim=-1)
    a[-1] = qv - 1
    a_rows = a[rows].cpu().numpy()
    x = a.clone()
    P.crt(x)
    assert np.array_equal(x[rows].cpu().numpy(), cpuref.crt(R, a_rows).reshape(len(rows), R.n, T)), "crt"
    P.crtInv(x)
    assert torch.equal(x, a), "crtInv . crt"
    del x
    # polymul: the unit at every position, and sampled rows of a product against the oracle
    one = torch.zeros_like(a); one[:, 0, :] = 1
    c = torch.empty_like(a)
    P.polymul(a, one, out=c)
    assert torch.equal(c, a), "a * 1"
    b = one
    del one
    for t, q in enumerate(qs):
        b[..., t].random_(0, q, generator=g)
    P.polymul(a, b, out=c)
    want = cpuref.polymul(R, a_rows, b[rows].cpu().numpy()).reshape(len(rows), R.n, T)
    assert np.array_equal(c[rows].cpu().numpy(), want), "polymul"
    del a, b, c
    torch.cuda.empty_cache()


def test_grid_stride_mixed_keyswitch(gpu, cpuref):
    """k_mixed_keyswitch with B * T = 140,000 items"""
    import torch
    m, T, B = 45, 2, 70000
    pps, qs = lm.factor_pps(m), _qs(m, 2 ** 29, T)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    _need_hbm(2)
    items = B * T
    rows = _rows_of_items(_boundary_items(items), T, 1, B)
    g = torch.Generator(device="cuda"); g.manual_seed(45)
    rnd = lambda *shape: torch.stack([torch.randint(0, q, shape, dtype=torch.int64, device="cuda", generator=g) for q in qs], dim=-1)
    for base in (0, 256):
        Ld = P.decomposeLen(base)
        c2, hint, add = rnd(B, R.n), rnd(Ld, 2, R.n), rnd(2, B, R.n)
        fused = P.keySwitch(c2, base, hint, addend=add)
        gpu.debug_set("KEYSWITCH_UNFUSED", True)
        try:
            unfused = P.keySwitch(c2, base, hint, addend=add)
        finally:
            gpu.debug_set("KEYSWITCH_UNFUSED", False)
        assert torch.equal(fused, unfused), base
        want = sr.keyswitch(cpuref, R, c2[rows].cpu().numpy(), base, hint.cpu().numpy())
        want = (want.astype(object) + add[:, rows].cpu().numpy()) % np.array(qs, dtype=object)
        assert np.array_equal(fused[:, rows].cpu().numpy(), want.astype(np.int64)), base


def _enc_rows(B):
    return sorted({b for b in (0, GRID_Y_CAP - 1, GRID_Y_CAP, GRID_Y_CAP + 1, 2 * GRID_Y_CAP - 1, 2 * GRID_Y_CAP,
                               2 * GRID_Y_CAP + 2, B - 1) if b < B})


@pytest.mark.parametrize("ctr", [5, 2 ** 32 - 70000])            # the second: ctr + b crosses 2^32 inside the second sweep
def test_grid_stride_encrypt(gpu, cpuref, ctr):
    import torch
    m, p, T, B, svar = 16, 5, 2, 140000, 1.5
    qs = _qs(m, 2 ** 29, T)
    pq, pp = gpu.Plan.for_index(m, qs), gpu.Plan.for_index(m, [p])
    n = pq.n
    rng = np.random.default_rng(ctr % 1000)
    key = rng.bytes(32)
    pt_h = rng.integers(-p + 1, p, size=(B, n), dtype=np.int64)
    pt = torch.from_numpy(pt_h).cuda()
    s_crt = torch.from_numpy(_small_key(cpuref, m, qs, rng)).cuda()
    rows = _enc_rows(B)
    if ctr > 2 ** 31:
        rows = sorted(set(rows) | {2 ** 32 - ctr - 1, 2 ** 32 - ctr})
        assert GRID_Y_CAP <= 2 ** 32 - ctr < 2 * GRID_Y_CAP
    for out_crt in (True, False):
        whole = pq.encrypt(pt, s_crt, pp, svar, key=key, ctr=ctr, out_crt=out_crt)
        for cut in (GRID_Y_CAP, GRID_Y_CAP + 1):
            parts = torch.cat([pq.encrypt(pt[:cut].contiguous(), s_crt, pp, svar, key=key, ctr=ctr, out_crt=out_crt),
                               pq.encrypt(pt[cut:].contiguous(), s_crt, pp, svar, key=key, ctr=ctr + cut, out_crt=out_crt)],
                              dim=1)
            assert torch.equal(whole, parts), (out_crt, cut)
        if out_crt:
            c1 = whole[1].cpu().numpy()
            for b in rows:
                assert np.array_equal(c1[b], er.uniform_crt(key, ctr + b, 1, n, qs)[0]), b
        e = pq.errorTerm(whole, s_crt, p, cs_crt=out_crt).cpu().numpy()
        rep = _rep(cpuref, m, m, p, pt_h[rows])
        for i, b in enumerate(rows):
            e_want, near = _restated_e(m, p, svar, key, ctr + b, 1, rep[i:i + 1])
            bad = e[b] != e_want[0]
            assert bad.sum() <= 1 and near[0][bad].all(), (b, out_crt)
        assert torch.equal(pq.decrypt(whole, s_crt, pp, cs_crt=out_crt), pt % p), out_crt


@pytest.mark.parametrize("ctr", [5, 2 ** 32 - 70000])
def test_grid_stride_error_rounded(gpu, ctr):
    import torch
    m, B, svar = 16, 140000, 3.0
    pq = gpu.Plan.for_index(m, _qs(m, 2 ** 29, 2))
    key = bytes(range(5, 37))
    z = pq.errorRounded(svar, B=B, key=key, ctr=ctr)
    for cut in (GRID_Y_CAP, GRID_Y_CAP + 1):
        assert torch.equal(z, torch.cat([pq.errorRounded(svar, B=cut, key=key, ctr=ctr),
                                         pq.errorRounded(svar, B=B - cut, key=key, ctr=ctr + cut)])), cut
    zh = z.cpu().numpy()
    rows = _enc_rows(B)
    if ctr > 2 ** 31:
        rows = sorted(set(rows) | {2 ** 32 - ctr - 1, 2 ** 32 - ctr})
    sig = er.sigma(lm.factor_pps(m), svar)
    for b in rows:
        x = er.gaussians(key, er.DOM_ERR_ROUNDED, ctr + b, 1, pq.n, sig)
        want, near = er.round_coset(x, np.zeros((1, pq.n), dtype=np.int64), 1)
        bad = zh[b] != want[0]
        assert bad.sum() <= 1 and near[0][bad].all(), b
