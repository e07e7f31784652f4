"""Whole RLWE / RLWR challenges on the GPU (lolhip_chall_*, lol_amd.RLWE.instances / validInstances): I instances of
L samples generated in one call and verified in one call, bit-exact throughout.

    1 generate     equals I single-secret calls at the stated counters (secret i at ctr_s + i, the samples of instance
                   i at ctr + i L), taken to the decoding basis with crtInv and lInv; s, a and the RLWR b also equal the
                   CPU model of tests/challenge_ref.py; Cont doubles compared as bits
    2 verify       fails and worst equal the model and a host reduction of the per-sample errorGSqNorm* / mismatchRLWR
                   outputs; the strict bound; one corrupted coefficient; permuted secrets; a saturated norm
    3 status       decided on the host, outputs untouched
    4 end to end   generate -> files -> verify from a temporary directory on one plan-route and one ring-route shape,
                   the suppressed variant with I - 1 secrets, regen, and regen after one flipped byte of a

Every raw call has guard words around every output and a poisoned work buffer.  Shapes, plan route (lolhip_chall_*):
m = 32 / q = 97 (2-power), m = 21 / q = 337 (vector interpreter), m = 23 / q = 47 (scalar interpreter: the samplers of
Disc and Cont refuse a prime above 13, so generate is RLWR there and the Disc / Cont data is made by the model), m = 32
over (97, 193) (T = 2, Disc).  Ring route (lolhip_chall_ring_*): m = 32 / q = 512 (fused tails), m = 12 / q = 500
(unfused).  RLWR with p = 2 and p = q - 1.  (I, L): (1, 1) and (3, 2) the degenerate and the small grouping, (3, 5) where
b / L differs from b % I, run with every slab one word off a 16-byte boundary (the one-word-per-access kernels),
(33, 3): 99 items, instance boundaries inside a workgroup of four items.

Permuted secrets, svar = 0.5, eps = 2^-25, (I, L) = (3, 5), key / counters below: the model gives
    m = 32 q = 97    Disc bound 197,      honest max 44,      permuted min 8129
                     Cont bound 96.0998,  honest max 42.9658, permuted min 8144.38
    m = 21 q = 337   Disc bound 414,      honest max 60,      permuted min 68536
                     Cont bound 112.564,  honest max 43.9416, permuted min 67973.3
    m = 32 (97,193)  Disc bound 197,      honest max 44,      permuted min 361730048
    m = 32 q = 512   Disc bound 197,      honest max 44,      permuted min 247410
                     Cont bound 96.0998,  honest max 42.9658, permuted min 247446
    m = 12 q = 500   Disc bound 74,       honest max 8,       permuted min 8960
                     Cont bound 23.2291,  honest max 7.69374, permuted min 9012.76
and the test asserts honest max < bound < permuted min on the model before it looks at the device."""
import functools

import numpy as np
import pytest

import challenge_ref as cf
import rlwe_ref as rr

DISC, CONT, RLWR = cf.DISC, cf.CONT, cf.RLWR
# (m, moduli, route): "plan" = lolhip_chall_* (a CRT basis), "ring" = lolhip_chall_ring_* (fused tails at m = 32, unfused at 12)
CASES = [(32, (97,), "plan"), (21, (337,), "plan"), (23, (47,), "plan"), (32, (97, 193), "plan"), (32, (512,), "ring"),
         (12, (500,), "ring")]
IL = [(1, 1), (3, 2), (3, 5), (33, 3)]
KEY, CTR_S, CTR, SVAR, EPS = bytes(range(32)), 100, 1000, 0.5, 2.0 ** -25
SENT, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
INT64_MAX = rr.INT64_MAX
ERR_INVALID, ERR_NO_CRT = -1, -3


def _kinds(case):
    """(kind, p) the device can generate at this case"""
    m, qs, _ = CASES[case]
    if len(qs) > 1:
        return [(DISC, 0)]
    rl = [(RLWR, 2), (RLWR, qs[0] - 1)]
    return rl if m == 23 else [(DISC, 0), (CONT, 0)] + rl


def _all_kinds(case):
    """(kind, p) that verify takes at this case"""
    return [(DISC, 0)] if len(CASES[case][1]) > 1 else [(DISC, 0), (CONT, 0), (RLWR, 2), (RLWR, CASES[case][1][0] - 1)]


@functools.lru_cache(maxsize=None)
def _plan(case):
    import lol_amd
    m, qs, _ = CASES[case]
    return lol_amd.Plan.for_index(m, list(qs))


def _ring(case):
    return CASES[case][2] == "ring"


@functools.lru_cache(maxsize=None)
def _rl(case):
    """the single-secret class of the case's route"""
    import lol_amd
    return (lol_amd.RingRLWE if _ring(case) else lol_amd.RLWE)(_plan(case))


def _model(cpuref, case):
    m, qs, _ = CASES[case]
    return cf.RingModel(m, qs[0]) if _ring(case) else cf.Model(cpuref, m, qs)


def _entry(gpu, case, name):
    """the C entry of the case's route with its leading handles bound"""
    L = gpu.lib()
    if _ring(case):
        return functools.partial(getattr(L, f"lolhip_chall_ring_{name}"), _rl(case).ring._h, _plan(case)._h)
    return functools.partial(getattr(L, f"lolhip_chall_{name}"), _plan(case)._h)


def _bits(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _bound(case, kind):
    m = CASES[case][0]
    return rr.error_bound_disc(m, SVAR, EPS) if kind == DISC else rr.error_bound_cont(m, SVAR, EPS) if kind == CONT else 0


# ---- buffers with guard words ---------------------------------------------------------------------------------------------
class Guarded:
    """`count` elements with `guard` sentinel words on either side; guard odd: the slab is one word off 16 bytes"""

    def __init__(self, count, dtype="int64", guard=8):
        import torch
        self.int32 = dtype == "int32"
        g = 2 * guard if self.int32 else guard                    # int32: the same bytes of guard
        self.buf = torch.full((count + 2 * g,), SENT32 if self.int32 else SENT, dtype=torch.int32 if self.int32 else torch.int64,
                              device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.g, self.count, self.dtype = g, count, dtype
        self.t = self.buf[g:g + count]

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        s = SENT32 if self.int32 else SENT
        return bool((self.buf[:self.g] == s).all()) and bool((self.buf[self.g + self.count:] == s).all())

    def untouched(self):
        return bool((self.buf == (SENT32 if self.int32 else SENT)).all())

    def value(self, *shape):
        import torch
        t = self.t.clone()
        return (t.view(torch.float64) if self.dtype == "float64" else t).reshape(shape)


def _work(gpu, case, kind, I, L, guard):
    guard = 8 if _ring(case) else guard                            # the ring route asks for a 16-byte-aligned work buffer
    wl = _entry(gpu, case, "work_len")(kind, I, L)
    assert wl > 0
    return Guarded(wl, guard=guard)


def raw_generate(gpu, case, kind, p, I, L, svar=SVAR, guard=8, key=KEY):
    """(rc, s, a, b, buffers) of the C entry on guarded buffers and poisoned work; s [I][n][T], a [I L][n][T]"""
    import torch
    plan = _plan(case)
    n, T, B = plan.n, plan.T, I * L
    s = Guarded(I * n * T, guard=guard)
    a = Guarded(B * n * T, guard=guard)
    b = Guarded(B * n * (T if kind == DISC else 1), "float64" if kind == CONT else "int64", guard=guard)
    w = _work(gpu, case, kind, I, L, guard)
    rc = _entry(gpu, case, "generate_batch")(None, kind, p, svar, key, CTR_S, CTR, I, L, s.ptr(), a.ptr(), b.ptr(), w.ptr())
    torch.cuda.synchronize()
    assert all(x.intact() for x in (s, a, b, w))
    return rc, s.value(I, n, T), a.value(B, n, T), b.value(*((B, n, T) if kind == DISC else (B, n))), (s, a, b)


def raw_verify(gpu, case, kind, p, L, s_dec, a_dec, b, bound, guard=8):
    """(rc, fails, worst, buffers) of the C entry; inputs numpy or tensors, checked unwritten"""
    import torch
    plan = _plan(case)
    dev = lambda x, dt: (torch.from_numpy(np.ascontiguousarray(x, dtype=dt)) if isinstance(x, np.ndarray) else x).cuda().contiguous()
    s_d, a_d, b_d = dev(s_dec, np.int64), dev(a_dec, np.int64), dev(b, np.float64 if kind == CONT else np.int64)
    before = [t.clone() for t in (s_d, a_d, b_d)]
    I = s_d.numel() // (plan.n * plan.T)
    fails = Guarded(I, "int32", guard=guard)
    worst = Guarded(I, "float64" if kind == CONT else "int64", guard=guard)
    w = _work(gpu, case, kind, I, L, guard)
    bd, bc = (int(bound), 0.0) if kind == DISC else (0, float(bound))
    rc = _entry(gpu, case, "verify_batch")(None, kind, p, bd, bc, I, L, s_d.data_ptr(), a_d.data_ptr(), b_d.data_ptr(),
                                            fails.ptr(), worst.ptr(), w.ptr())
    torch.cuda.synchronize()
    assert all(x.intact() for x in (fails, worst, w))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip((s_d, a_d, b_d), before))
    return rc, fails.value(I).cpu().numpy(), worst.value(I).cpu().numpy(), (fails, worst)


# ---- the same work as I single-secret calls ---------------------------------------------------------------------------------
def _to_dec(case, x):
    """the stream's basis (CRT, or powerful on the ring route) -> decoding basis with the existing passes, on a copy"""
    plan, y = _plan(case), x.clone()
    if not _ring(case):
        plan.crtInv(y)
    plan.lInv(y)
    return y


def _from_dec(case, x):
    plan, y = _plan(case), x.clone()
    plan.l(y)
    if not _ring(case):
        plan.crt(y)
    return y


def singles(gpu, case, kind, p, I, L):
    """(s_dec [I][n][T], a_dec [B][n][T], b) from I calls of secret() and sample*()"""
    import torch
    plan, r = _plan(case), _rl(case)
    n, T = plan.n, plan.T
    ss, aa, bb = [], [], []
    for i in range(I):
        s = r.secret(key=KEY, ctr=CTR_S + i)
        s, sec = (s[0], s[1]) if _ring(case) else (s, s)           # the ring route samples against the prepared secret
        c = CTR + i * L
        a, b = (r.sampleDisc(sec, L, SVAR, key=KEY, ctr=c) if kind == DISC else
                r.sampleCont(sec, L, SVAR, key=KEY, ctr=c) if kind == CONT else r.sampleRLWR(sec, L, p, key=KEY, ctr=c))
        ss.append(_to_dec(case, s).reshape(n, T))
        aa.append(_to_dec(case, a).reshape(L, n, T))
        bb.append(_to_dec(case, b).reshape(L, n, T) if kind == DISC else b)
    return torch.stack(ss), torch.cat(aa), torch.cat(bb)


def per_sample(gpu, case, kind, p, L, s_dec, a_dec, b):
    """the existing per-sample outputs under secret b / L, as numpy: Disc / Cont norms, RLWR mismatch counts"""
    import torch
    plan, r = _plan(case), _rl(case)
    n, T = plan.n, plan.T
    dev = lambda x, dt: (torch.from_numpy(np.ascontiguousarray(x, dtype=dt)) if isinstance(x, np.ndarray) else x).cuda()
    s_c, a_c = _from_dec(case, dev(s_dec, np.int64)).reshape(-1, n, T), _from_dec(case, dev(a_dec, np.int64)).reshape(-1, n, T)
    b = dev(b, np.float64 if kind == CONT else np.int64)
    b = _from_dec(case, b).reshape(-1, n, T) if kind == DISC else b
    if _ring(case):
        s_c, a_c, b = s_c.reshape(-1, n), a_c.reshape(-1, n), b.reshape(-1, n)
    out = []
    for i in range(s_c.shape[0]):
        sl = slice(i * L, (i + 1) * L)
        sec = r.prepare(s_c[i].contiguous()) if _ring(case) else s_c[i]
        out.append(r.errorGSqNormDisc(sec, a_c[sl], b[sl]) if kind == DISC else
                   r.errorGSqNormCont(sec, a_c[sl], b[sl]) if kind == CONT else r.mismatchRLWR(sec, a_c[sl], b[sl], p))
    return torch.cat(out).cpu().numpy()


def data(gpu, M, case, kind, p, I, L):
    """challenge data (numpy, decoding basis) of this case: from the device where it can sample, else honest data made
    by the model with small hand-made errors"""
    if (kind, p) in _kinds(case):
        rc, s, a, b, _ = raw_generate(gpu, case, kind, p, I, L)
        assert rc == 0
        return s.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()
    rng = np.random.default_rng(1000 * case + 10 * I + L)
    q, B = M.qs[0], I * L
    s = rng.integers(0, q, size=(I, M.n, 1), dtype=np.int64)
    a = rng.integers(0, q, size=(B, M.n, 1), dtype=np.int64)
    x = M.x_grouped(a, s, L)
    if kind == DISC:
        return s, a, (x + rng.integers(-1, 2, size=(B, M.n, 1))) % q
    return s, a, rr.cont_sample(x[..., 0], rng.normal(size=(B, M.n)) * 0.5, q)


# ---------------------------------------------------------------------------------------------
# 1. generate
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("I,L", IL)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_generate_equals_single_secret_calls(gpu, cpuref, case, I, L):
    import torch
    M = _model(cpuref, case)
    guard = 7 if (I, L) == (3, 5) else 8
    for kind, p in _kinds(case):
        rc, s, a, b, _ = raw_generate(gpu, case, kind, p, I, L, guard=guard)
        assert rc == 0
        s1, a1, b1 = singles(gpu, case, kind, p, I, L)
        assert torch.equal(s, s1) and torch.equal(a, a1), (kind, p)
        assert b.dtype == b1.dtype and torch.equal(_bits(b), _bits(b1)), (kind, p)
        want = cf.generate(M, kind, I, L, SVAR, p, KEY, CTR_S, CTR)
        assert np.array_equal(s.cpu().numpy(), want["s"]) and np.array_equal(a.cpu().numpy(), want["a"])
        if kind == RLWR:
            assert np.array_equal(b.cpu().numpy(), want["b"]) and int(b.max()) < p
        # the Python layer gives the same tensors
        s2, a2, b2 = _rl(case).instances(kind, I, L, svar=SVAR, p=p, key=KEY, ctr_s=CTR_S, ctr=CTR)
        assert torch.equal(s2.reshape(s.shape), s) and torch.equal(a2.reshape(a.shape), a)
        assert torch.equal(_bits(b2).reshape(b.shape), _bits(b))


# ---------------------------------------------------------------------------------------------
# 2. verify
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("I,L", IL)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_verify_equals_model_and_per_sample_reduction(gpu, cpuref, case, I, L):
    M = _model(cpuref, case)
    guard = 7 if (I, L) == (3, 5) else 8
    mid = I // 2
    for kind, p in _all_kinds(case):
        s, a, b = data(gpu, M, case, kind, p, I, L)
        vals = cf.sample_values(M, kind, L, s, a, b, p)
        dvals = per_sample(gpu, case, kind, p, L, s, a, b)
        if kind == CONT:
            assert (np.abs(dvals - vals) <= 1e-12 * np.abs(vals)).all()
        else:
            assert np.array_equal(dvals, vals)
        bound = _bound(case, kind) if (kind, p) in _kinds(case) else (int(vals.max()) + 1 if kind == DISC else 1.5 * vals.max() + 1)
        if kind != RLWR:
            assert vals.max() < bound, (kind, vals.max(), bound)               # honest data passes on the model

        def check(s_, a_, b_, bound_, why):
            rc, fails, worst, _ = raw_verify(gpu, case, kind, p, L, s_, a_, b_, bound_, guard=guard)
            assert rc == 0
            dv = per_sample(gpu, case, kind, p, L, s_, a_, b_)
            f_dev, w_dev = cf.verdict(kind, dv, L, bound_)
            assert np.array_equal(fails, f_dev), why
            assert np.array_equal(worst.view(np.int64), np.ascontiguousarray(w_dev).view(np.int64)), why
            f_mod, w_mod = cf.verify(M, kind, L, s_, a_, b_, bound_, p)
            assert np.array_equal(fails, f_mod), why
            if kind == CONT:
                assert (np.abs(worst - w_mod) <= 1e-12 * np.abs(w_mod)).all(), why
            else:
                assert np.array_equal(worst, w_mod), why
            return fails, worst

        fails, worst = check(s, a, b, bound, "honest")
        assert not fails.any()
        if kind == DISC:
            # the strict bound: the largest norm itself fails exactly the instances that reach it, one more passes all
            top = int(vals.max())
            fails, _ = check(s, a, b, top, "bound = a sample's own norm")
            assert list(fails > 0) == list(vals.reshape(I, L).max(axis=1) == top) and fails.any()
            fails, _ = check(s, a, b, top + 1, "bound = norm + 1")
            assert not fails.any()
        # one coefficient of the last sample of the middle instance
        b2 = b.copy()
        at = ((mid + 1) * L - 1, M.n // 2) + ((0,) if kind == DISC else ())
        q = M.qs[0]
        b2[at] = (b2[at] + 1) % p if kind == RLWR else (b2[at] + q // 2) % q if kind == DISC else (b2[at] + q / 2) % q
        vals2 = cf.sample_values(M, kind, L, s, a, b2, p)                         # the model: only that sample fails
        bad = (vals2 != 0) if kind == RLWR else ~(bound > vals2)
        assert list(np.flatnonzero(bad)) == [at[0]]
        fails, worst = check(s, a, b2, bound, "one corruption")
        assert [int(f) for f in fails] == [1 if i == mid else 0 for i in range(I)]
        # the Python layer
        f2, w2 = _rl(case).validInstances(kind, s, a, b2, bound=bound, p=p)
        assert np.array_equal(f2, fails) and np.array_equal(np.ascontiguousarray(w2).view(np.int64), worst.view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 3, 4, 5])
def test_permuted_secrets_fail_every_instance(gpu, cpuref, case):
    I, L = 3, 5
    M = _model(cpuref, case)
    one = len(CASES[case][1]) == 1
    for kind in ((DISC, CONT) if one else (DISC,)):
        bound = _bound(case, kind)
        g = cf.generate(M, kind, I, L, SVAR, 0, KEY, CTR_S, CTR)
        honest = cf.sample_values(M, kind, L, g["s"], g["a"], g["b"])
        permuted = cf.sample_values(M, kind, L, np.roll(g["s"], 1, axis=0), g["a"], g["b"])
        assert honest.max() < bound < permuted.min(), (honest.max(), bound, permuted.min())   # the docstring's table
        s, a, b = data(gpu, M, case, kind, 0, I, L)
        rc, fails, _, _ = raw_verify(gpu, case, kind, 0, L, s, a, b, bound)
        assert rc == 0 and not fails.any()
        sp = np.roll(s, 1, axis=0)
        rc, fails, worst, _ = raw_verify(gpu, case, kind, 0, L, sp, a, b, bound)
        f_mod, w_mod = cf.verify(M, kind, L, sp, a, b, bound)
        assert rc == 0 and list(fails) == [L] * I and np.array_equal(fails, f_mod)
        assert np.array_equal(worst, w_mod) if kind == DISC else (np.abs(worst - w_mod) <= 1e-12 * w_mod).all()
    # RLWR: every sample of every instance mismatches somewhere under another secret
    if one:
        q = CASES[case][1][0]
        s, a, b = data(gpu, M, case, RLWR, q - 1, I, L)
        sp = np.roll(s, 1, axis=0)
        rc, fails, worst, _ = raw_verify(gpu, case, RLWR, q - 1, L, sp, a, b, 0)
        f_mod, w_mod = cf.verify(M, RLWR, L, sp, a, b, 0, q - 1)
        assert rc == 0 and np.array_equal(fails, f_mod) and np.array_equal(worst, w_mod) and list(fails) == [L] * I


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["plan", "ring"])
def test_saturated_norm_fails_under_every_bound(gpu, cpuref, route):
    """a 61-bit modulus: the lifted error q // 2 has a square beyond int64, the norm saturates and the sample fails even
    under bound = INT64_MAX; the instance beside it passes"""
    from oracle import lolmath as lm
    m, I, L = 32, 2, 2
    q = next(lm.good_qs(m, 2 ** 60)) if route == "plan" else 2 ** 61
    plan = gpu.Plan.for_index(m, [q])
    r = gpu.RLWE(plan) if route == "plan" else gpu.RingRLWE(plan)
    M = cf.Model(cpuref, m, [q]) if route == "plan" else cf.RingModel(m, q)
    n = M.n
    s = np.zeros((I, n, 1), dtype=np.int64)
    a = np.random.default_rng(5).integers(0, q, size=(I * L, n, 1), dtype=np.int64)
    b = np.ones((I * L, n, 1), dtype=np.int64)
    b[1, 3, 0] = q // 2 - 1
    fails, worst = r.validInstances("disc", s, a, b, bound=INT64_MAX)
    assert list(fails) == [1, 0] and list(worst) == [INT64_MAX, n]
    f_mod, w_mod = cf.verify(M, DISC, L, s, a, b, INT64_MAX)
    assert np.array_equal(fails, f_mod) and np.array_equal(worst, w_mod)
    # the Python layer clamps a bound beyond int64: still only the saturated sample fails
    f2, w2 = r.validInstances("disc", s, a, b, bound=2 ** 70)
    assert list(f2) == [1, 0] and list(w2) == [INT64_MAX, n]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 4])
def test_nan_norm_fails_cont(gpu, case):
    n, I, L = _plan(case).n, 2, 3
    s = np.zeros((I, n, 1), dtype=np.int64)
    a = np.zeros((I * L, n, 1), dtype=np.int64)
    b = np.zeros((I * L, n))
    b[4, 2] = np.nan
    rc, fails, worst, _ = raw_verify(gpu, case, CONT, 0, L, s, a, b, 1e300)
    assert rc == 0 and list(fails) == [0, 1] and worst[0] == 0 and np.isnan(worst[1])


# ---------------------------------------------------------------------------------------------
# 3. status codes on a device plan: decided on the host, outputs untouched
# ---------------------------------------------------------------------------------------------
def _gen_status(gpu, entry_of, plan, kind, p=4, svar=1.0, I=2, L=2):
    import torch
    Ib, Lb = I if 0 < I < 100 else 1, L if 0 < L < 100 else 1            # the buffers of a small valid call
    n, T, B = plan.n, plan.T, Ib * Lb
    s, a, b = Guarded(Ib * n * T), Guarded(B * n * T), Guarded(B * n * T)
    w = Guarded(max(entry_of("work_len")(0, Ib, Lb), 1))
    rc = entry_of("generate_batch")(None, kind, p, svar, KEY, 0, 0, I, L, s.ptr(), a.ptr(), b.ptr(), w.ptr())
    torch.cuda.synchronize()
    return rc, all(x.untouched() for x in (s, a, b))


def _ver_status(gpu, entry_of, plan, kind, p=4, I=2, L=2):
    import torch
    Ib, Lb = I if 0 < I < 100 else 1, L if 0 < L < 100 else 1
    n, T, B = plan.n, plan.T, Ib * Lb
    z = torch.zeros((B * n * T,), dtype=torch.int64, device="cuda")
    f, wo = Guarded(Ib, "int32"), Guarded(Ib)
    w = Guarded(max(entry_of("work_len")(0, Ib, Lb), 1))
    rc = entry_of("verify_batch")(None, kind, p, 1, 1.0, I, L, z.data_ptr(), z.data_ptr(), z.data_ptr(), f.ptr(), wo.ptr(),
                                  w.ptr())
    torch.cuda.synchronize()
    return rc, f.untouched() and wo.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 4])
def test_errors_leave_outputs_untouched(gpu, case):
    p1, q = _plan(case), CASES[case][1][0]
    gen = lambda kind, **kw: _gen_status(gpu, lambda nm: _entry(gpu, case, nm), p1, kind, **kw)
    ver = lambda kind, **kw: _ver_status(gpu, lambda nm: _entry(gpu, case, nm), p1, kind, **kw)
    for kind in (0, 1, 2):
        assert gen(kind) == (0, False) and ver(kind) == (0, False), kind
        assert gen(kind, I=-1) == ver(kind, I=-1) == (ERR_INVALID, True)
        assert gen(kind, L=0) == ver(kind, L=0) == (ERR_INVALID, True)
        assert gen(kind, I=2 ** 31, L=1) == ver(kind, I=2 ** 16, L=2 ** 15) == (ERR_INVALID, True)
        assert gen(kind, I=0) == ver(kind, I=0) == (0, True)
    assert gen(3) == gen(-1) == ver(3) == (ERR_INVALID, True)
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        assert gen(0, svar=sv) == gen(1, svar=sv) == (ERR_INVALID, True)
        assert gen(2, svar=sv) == (0, False)
    for p in (q, q + 1, 1, 0, -5):
        assert gen(2, p=p) == ver(2, p=p) == (ERR_INVALID, True), p
    assert gen(2, p=q - 1) == ver(2, p=q - 1) == (0, False)
    # the Python layer raises with the code before it stages anything
    with pytest.raises(gpu.LolHipError) as ei:
        _rl(case).instances("disc", 2, 2, svar=-1.0)
    assert ei.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        _rl(case).validInstances("rlwr", np.zeros((2, p1.n, 1), dtype=np.int64), np.zeros((3, p1.n, 1), dtype=np.int64),
                                 np.zeros((3, p1.n), dtype=np.int64), p=4)


@pytest.mark.gpu
def test_errors_of_each_route(gpu):
    from oracle import lolmath as lm
    L = gpu.lib()
    plan_entry = lambda pl: (lambda nm: functools.partial(getattr(L, f"lolhip_chall_{nm}"), pl._h))
    p2, p23 = _plan(3), _plan(2)
    gen = lambda pl, kind: _gen_status(gpu, plan_entry(pl), pl, kind)
    ver = lambda pl, kind: _ver_status(gpu, plan_entry(pl), pl, kind)
    # one modulus only for Cont and RLWR
    assert gen(p2, 0) == ver(p2, 0) == (0, False)
    assert gen(p2, 1) == gen(p2, 2) == ver(p2, 1) == ver(p2, 2) == (ERR_INVALID, True)
    # the sampler's index limits, as the single-secret entries: generate only
    assert gen(p23, 0) == gen(p23, 1) == (ERR_INVALID, True)
    assert gen(p23, 2) == ver(p23, 0) == ver(p23, 1) == ver(p23, 2) == (0, False)
    # no CRT basis
    no_crt = [v for v in range(1000003, 1001000, 2) if lm.is_prime(v) and (v - 1) % 64][0]
    pn = gpu.Plan.for_index(64, [no_crt])
    assert not pn.has_crt
    for kind in (0, 1, 2):
        assert gen(pn, kind) == ver(pn, kind) == (ERR_NO_CRT, True)
    # the ring route: pq must be the plan the handle was made from
    ring, other = _rl(4), _plan(5)
    ring_entry = lambda pl: (lambda nm: functools.partial(getattr(L, f"lolhip_chall_ring_{nm}"), ring.ring._h, pl._h))
    for kind in (0, 1, 2):
        assert L.lolhip_chall_ring_work_len(ring.ring._h, other._h, kind, 2, 2) == ERR_INVALID
        assert L.lolhip_chall_ring_work_len(None, _plan(4)._h, kind, 2, 2) == ERR_INVALID
    assert _gen_status(gpu, lambda nm: (lambda *a: 1) if nm == "work_len" else ring_entry(other)(nm), other, 2) == (ERR_INVALID, True)
    assert _ver_status(gpu, lambda nm: (lambda *a: 1) if nm == "work_len" else ring_entry(other)(nm), other, 2) == (ERR_INVALID, True)


# ---------------------------------------------------------------------------------------------
# 4. end to end: generate -> files -> verify from a directory, on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,q,route", [(32, 97, "plan"), (12, 500, "ring")])
def test_tree_end_to_end_on_the_device(gpu, cpuref, tmp_path, m, q, route):
    import os
    from lol_amd import challenges as ch
    root = str(tmp_path)
    lines = f'0 Cont {m} {q} 0.5 3 "toy" 1 Disc {m} {q} 0.5 3 "toy" 2 RLWR {m} {q} {q - 1} 3 "toy"'
    M = cf.Model(cpuref, m, [q]) if route == "plan" else cf.RingModel(m, q)
    for cp in ch.parse_params(lines, num_instances=5):
        assert ch.route(cp)[0] == route
        name = ch.generate(cp, root, KEY, beacon=(1478822400, 63), ctr_s=CTR_S, ctr=CTR)
        # the files hold what one grouped call gives, and the model agrees on what is exact
        kind = {"Disc": DISC, "Cont": CONT, "RLWR": RLWR}[cp.kind]
        _, ids, s, a, b, seeds = ch.read_tree(root, name)
        s1, a1, b1 = (t.cpu().numpy().reshape(-1, M.n) for t in
                      ch.generate_arrays(cp, KEY, ctr_s=CTR_S, ctr=CTR))
        assert ids == list(range(5)) and np.array_equal(s, s1) and np.array_equal(a, a1)
        assert np.array_equal(np.ascontiguousarray(b).view(np.int64), np.ascontiguousarray(b1).view(np.int64))
        want = cf.generate(M, kind, 5, 3, 0.5, cp.p or 0, KEY, CTR_S, CTR)
        assert np.array_equal(s, want["s"][..., 0]) and np.array_equal(a, want["a"][..., 0])
        assert seeds[4] == KEY + (CTR_S + 4).to_bytes(8, "little") + (CTR + 12).to_bytes(8, "little")
        res = ch.verify(root, name)
        assert sorted(res) == list(range(5)) and all(ok and f == 0 for ok, f, _ in res.values())
        f_mod, w_mod = cf.verify(M, kind, 3, s, a, b, ch.error_bound(cp) or 0, cp.p or 0)
        assert not f_mod.any() and (kind == CONT or [w for _, _, w in res.values()] == list(w_mod))
        assert ch.regen(root, name)
        # the suppressed variant: I - 1 secrets
        with pytest.raises(ch.ChallengeError, match="Secret 2 should not exist, but it does!"):
            ch.verify(root, name, beacon_byte=0xE8)
        assert ch.suppress(root, name, 0xE8) == 2
        res = ch.verify(root, name, beacon_byte=0xE8)
        assert sorted(res) == [0, 1, 3, 4] and all(ok for ok, _, _ in res.values())
        assert ch.regen(root, name, beacon_byte=0xE8)
        # one flipped byte of a: the last sint64 of a of the first sample of instance 1
        ipath = ch.instance_path(root, name, 1)
        inst = ch.instance_read(open(ipath, "rb").read(), cp.kind)
        blob = open(ipath, "rb").read()
        for j in range(M.n):                                       # a coefficient whose change is one byte of the file
            a2 = inst["a"].copy()
            a2[0, j] ^= 1
            blob2 = ch.instance_write(cp.challID, 1, inst["params"], a2, inst["b"])
            if len(blob) == len(blob2) and sum(x != y for x, y in zip(blob, blob2)) == 1:
                break
        assert len(blob) == len(blob2) and sum(x != y for x, y in zip(blob, blob2)) == 1
        open(ipath, "wb").write(blob2)
        assert not ch.regen(root, name, beacon_byte=0xE8)
        res = ch.verify(root, name, beacon_byte=0xE8)
        assert [i for i, (ok, _, _) in res.items() if not ok] == [1]
        assert os.path.exists(ch.secret_path(root, name, 1))
