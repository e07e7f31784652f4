"""The SymmSHE pipeline kernels with saturated lazy accumulators (-m gpu): the largest modulus of every arithmetic
class, residues of q - 1, and digit counts on both sides of every reduction interval.

Every check is bit-exact: against oracle/she_ref.py and tests/khprf_ref.py over the CPU oracle, against a Python-integer
CRT lift, and against the closed forms of tests/saturate.py (a key switch of saturating_c2 under the all-(q - 1) hint
is L mod q at every slot).  tests/test_saturation_host.py proves on the CPU that these inputs reach
interval * (q-1)^2 + carry in every window of every kernel's schedule.

    k_knapsack          Q32 form (every q < 2^29) at L = 31 ... 65, 128-bit form at L = 7 ... 17, K = 1, 2, 3
    k_keyswitch         m = 2^k just below 2^30 and 2^27, fewer and more than 64 threads per polynomial, n = 2^14, TrivGad
                        at T = 16; fused and three launches (k_decompose<true, .> and k_knapsack at the same moduli)
    k_mixed_keyswitch   just below 13 (q-1)^2 = 2^64 and 2^27 at m = 45, 1728, 11648; one modulus above the limit
    k_decompose         either side of the Q32 form's limits: moduli below 2^31 with bases around 2^31, moduli in [2^31, 2^32)
    KHPRF               q just below 2^29, 2^30, 2^31, 2^32, 2^61 and 2^62, the first above 2^32
    k_ctmul, k_sk_eval, k_lift      T = 2 and T = 16 moduli just below 2^62, plaintext modulus just below 2^62
"""
from math import prod

import numpy as np
import pytest

import khprf_ref as kr
import saturate as sat
from oracle import lolmath as lm
from oracle import she_ref as sr
from oracle.oracle import Params
from test_decrypt import INT64_MIN, _boundary_values, _centred, xs_rows

pytestmark = pytest.mark.gpu


def _plan(gpu, m, qs):
    pps = lm.factor_pps(m)
    return gpu.Plan(pps, qs), Params(pps, qs)


def _addq(a, b, qs):
    return ((a.astype(object) + b) % np.array(qs, dtype=object)).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# 1. k_knapsack directly
# ---------------------------------------------------------------------------------------------
KNAPSACK = [(m, "q32", 0) for m in (32, 45)] + [(m, "wide", i) for m in (32, 45) for i in range(4)]


@pytest.mark.parametrize("m,form,i", KNAPSACK)
def test_knapsack_saturated(gpu, cpuref, m, form, i):
    """row 0: xs, hint and addend all q - 1; row 1: the same as representatives in (-q, 0]; row 2: random.  Rows 0 and 1
    are (L - 1) mod q in closed form (L mod q without the addend); every row equals the restatement."""
    qs, Ls = (sat.class_top(m, "29", 3), (31, 32, 33, 64, 65)) if form == "q32" else (sat.knapsack_wide(m)[i], (7, 8, 9, 16, 17))
    P, R = _plan(gpu, m, qs)
    qv = np.array(qs, dtype=np.int64)
    rng = np.random.default_rng(m + i)
    B = 3
    for L in Ls:
        for K in (1, 2, 3):
            xs = np.stack([R.random(rng, B) for _ in range(L)])
            add = np.stack([R.random(rng, B) for _ in range(K)])
            xs[:, :2], add[:, :2] = qv - 1, qv - 1
            hint = sat.full_q1((L, K, R.n), qs)
            want = sr.knapsack(cpuref, R, xs, hint)
            wadd = _addq(want, add, qs)
            assert (want[:, :2] == L % qv).all() and (wadd[:, :2] == (L - 1) % qv).all(), (L, K)
            xs_in, add_in = xs.copy(), add.copy()
            xs_in[:, 1], add_in[:, 1] = -1, -1                                    # q - 1 in (-q, 0]
            assert np.array_equal(P.knapsack(xs_in, hint), want), (qs, L, K)
            assert np.array_equal(P.knapsack(xs_in, hint, addend=add_in), wadd), (qs, L, K, "addend")
            assert np.array_equal(P.knapsack(xs_in, sat.neg_rep(hint, qs), addend=add_in), wadd), (qs, L, K, "negative hint")
            hint_r = np.stack([np.stack([R.random(rng, 1)[0] for _ in range(K)]) for _ in range(L)])
            hint_r[::2, 0] = qv - 1
            want_r = _addq(sr.knapsack(cpuref, R, xs, hint_r), add, qs)
            assert np.array_equal(P.knapsack(xs_in, hint_r, addend=add_in), want_r), (qs, L, K, "random hint")


# ---------------------------------------------------------------------------------------------
# 2. / 3. the fused key switches
# ---------------------------------------------------------------------------------------------
def _routes(gpu, P, base, c2, hint, add, want, wadd, tag):
    """fused (where the plan takes it) and three launches, with and without the addend"""
    for unfused in (False, True):
        gpu.debug_set("KEYSWITCH_UNFUSED", unfused)
        try:
            assert np.array_equal(P.keySwitch(c2, base, hint), want), (tag, "unfused" if unfused else "fused")
            assert np.array_equal(P.keySwitch(c2, base, hint, addend=add), wadd), (tag, "unfused" if unfused else "fused", "addend")
        finally:
            gpu.debug_set("KEYSWITCH_UNFUSED", False)


def _keyswitch_four_items(gpu, cpuref, m, qs, base):
    """item 0 saturating; item 1 the same through negative representatives; items 2 and 3 random with q - 1 and q // 2
    planted.  Under the all-(q - 1) hint, as canonical and as negative residues, and under a random hint."""
    P, R = _plan(gpu, m, qs)
    qv = np.array(qs, dtype=np.int64)
    rng = np.random.default_rng(m + base + len(qs))
    B, L = 4, P.decomposeLen(base)
    assert L == sum(sr.digit_counts(R, base))
    c2 = R.random(rng, B)
    c2[0] = c2[1] = sat.saturating_c2(R, base)
    c2[2, 0], c2[2, 1], c2[3, 0], c2[3, 1] = qv - 1, qv // 2, qv // 2 - 1, qv - 1
    add = np.stack([R.random(rng, B) for _ in range(2)])
    add[:, :2] = qv - 1
    c2_in, add_in = c2.copy(), add.copy()
    c2_in[1], add_in[:, 1] = sat.neg_rep(c2[1], qs), -1
    hint = sat.full_q1((L, 2, R.n), qs)
    want = sr.keyswitch(cpuref, R, c2, base, hint)
    wadd = _addq(want, add, qs)
    assert (want[:, :2] == L % qv).all() and (wadd[:, :2] == (L - 1) % qv).all()
    _routes(gpu, P, base, c2_in, hint, add_in, want, wadd, (m, qs, base, "saturating hint"))
    _routes(gpu, P, base, sat.neg_rep(c2, qs), sat.neg_rep(hint, qs), sat.neg_rep(add, qs), want, wadd, (m, qs, base, "all negative"))
    hint_r = np.stack([np.stack([R.random(rng, 1)[0] for _ in range(2)]) for _ in range(L)])
    hint_r[::3, 1] = qv - 1
    want_r = sr.keyswitch(cpuref, R, c2, base, hint_r)
    _routes(gpu, P, base, c2_in, hint_r, add_in, want_r, _addq(want_r, add, qs), (m, qs, base, "random hint"))


def _keyswitch_closed_form(gpu, m, qs, base):
    """B = 1, the saturating item only: L mod q everywhere (L - 1 with the addend), fused and three launches"""
    P = gpu.Plan(lm.factor_pps(m), qs)
    qv = np.array(qs, dtype=np.int64)
    L = P.decomposeLen(base)
    c2 = sat.saturating_c2(P, base)[None]
    hint, add = sat.full_q1((L, 2, P.n), qs), sat.full_q1((2, 1, P.n), qs)
    want = np.ascontiguousarray(np.broadcast_to(L % qv, (2, 1, P.n, P.T)))
    wadd = np.ascontiguousarray(np.broadcast_to((L - 1) % qv, (2, 1, P.n, P.T)))
    _routes(gpu, P, base, c2, hint, add, want, wadd, (m, qs, base, "closed form"))
    return P, c2, hint, add


@pytest.mark.parametrize("m,kind,T", sat.KEYSWITCH_POW2)
def test_keyswitch_pow2_saturated(gpu, cpuref, m, kind, T):
    """k_keyswitch<L, 2> just below 2^30 and <L, 4> just below 2^27: n = 16 (one thread per polynomial, 256 polynomials
    per workgroup), n = 1024 (64 threads: s and b broadcast with readfirstlane), n = 2^14 by closed form"""
    qs = sat.class_top(m, kind, T)
    base = sat.pick_base(qs)
    if m <= 2048:
        _keyswitch_four_items(gpu, cpuref, m, qs, base)
    else:
        _keyswitch_closed_form(gpu, m, qs, base)


@pytest.mark.parametrize("m", [32, 2048])
def test_keyswitch_pow2_trivgad_one_full_window(gpu, cpuref, m):
    """TrivGad at T = 16 moduli just below 2^30, c2[., 0, t] = q_t - 1: sixteen digits of -1, one full window"""
    qs = sat.class_top(m, "30", 16)
    assert (sat.saturating_c2(Params([(2, 1)], qs[:1]), 0) == qs[0] - 1).all()
    _keyswitch_four_items(gpu, cpuref, m, qs, 0)


@pytest.mark.parametrize("m,kind,T", sat.KEYSWITCH_MIXED)
def test_keyswitch_mixed_saturated(gpu, cpuref, m, kind, T):
    """k_mixed_keyswitch just below 13 (q-1)^2 = 2^64 (class 2) and just below 2^27 (class 4); m = 11648 is the
    12-coefficients-per-thread instantiation (n = 5760): closed form, and the fused route = the three-launch route on
    random items"""
    qs = sat.class_top(m, kind, T)
    base = sat.pick_base(qs)
    if m != 11648:
        _keyswitch_four_items(gpu, cpuref, m, qs, base)
        return
    P, c2, hint, add = _keyswitch_closed_form(gpu, m, qs, base)
    rng = np.random.default_rng(m)
    c2r = np.stack([rng.integers(0, q, size=(2, P.n), dtype=np.int64) for q in qs], axis=-1)
    c2r[0, 0], c2r[0, 1] = np.array(qs) - 1, np.array(qs) // 2
    hint_r = np.stack([rng.integers(0, q, size=hint.shape[:-1], dtype=np.int64) for q in qs], axis=-1)
    add2 = sat.full_q1((2, 2, P.n), qs)
    fused = P.keySwitch(c2r, base, hint_r, addend=add2)
    gpu.debug_set("KEYSWITCH_UNFUSED", True)
    try:
        assert np.array_equal(P.keySwitch(c2r, base, hint_r, addend=add2), fused)
    finally:
        gpu.debug_set("KEYSWITCH_UNFUSED", False)


@pytest.mark.parametrize("m", [45, 1728])
def test_keyswitch_mixed_one_modulus_above_the_class_limit(gpu, cpuref, m):
    """a tuple with one modulus just above 13 (q-1)^2 = 2^64 leaves class 2, so the fused kernel must not take it: the
    answers are the restatement's and the closed form's on either route"""
    qs = [sat.class_top(m, "B13")[0], lm.first_good_q(m, sat.B13)]
    assert 13 * (qs[0] - 1) ** 2 < 2 ** 64 <= 13 * (qs[1] - 1) ** 2
    _keyswitch_four_items(gpu, cpuref, m, qs, sat.pick_base(qs))


# ---------------------------------------------------------------------------------------------
# 4. k_decompose at its own boundary
# ---------------------------------------------------------------------------------------------
def _decompose_inputs(R, rng):
    qv = np.array(R.qs, dtype=np.int64)
    c = R.random(rng, 3)
    c[0, 0], c[0, 1], c[0, 2], c[0, 3] = qv - 1, qv // 2, qv // 2 - 1, 0
    c[1] = qv - 1
    c[2, ::2] = qv // 2
    return c


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("kind", ["below31", "31to32"])
def test_decompose_at_the_q32_boundary(gpu, kind, T):
    """the Q32 form (every q < 2^31, base <= 2^31) and the general one next to it; T = 2 is the paired store.  Moduli
    just below 2^31 with bases 2^30 ... 2^31 + 1, and the whole of [2^31, 2^32) with base 256 and TrivGad."""
    m = 32
    if kind == "below31":
        qs, bases = sat.class_top(m, "31", T), (2 ** 30, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1)
    else:
        qs, bases = ([sat.class_top(m, "32")[0], lm.first_good_q(m, 2 ** 31)] + sat.class_top(m, "31", 1))[:T], (256, 0)
        assert all(q >= 2 ** 31 for q in qs[:2])
    P, R = _plan(gpu, m, qs)
    rng = np.random.default_rng(T)
    c = _decompose_inputs(R, rng)
    for base in bases:
        want = sr.decompose(R, c, base)
        assert P.decomposeLen(base) == want.shape[0]
        assert np.array_equal(P.decompose(c, base), want), (qs, base)
        assert np.array_equal(P.decompose(sat.neg_rep(c, qs), base), want), (qs, base, "negative")


# ---------------------------------------------------------------------------------------------
# 5. the key-homomorphic PRF
# ---------------------------------------------------------------------------------------------
KHPRF_QS = sat.khprf_moduli() + sat.class_top(sat.KHPRF_M, "62")
KHPRF_IDS = ["below2^29", "below2^30", "below2^31", "below2^32", "above2^32", "below2^61", "below2^62"]


@pytest.mark.parametrize("q", KHPRF_QS, ids=KHPRF_IDS)
def test_khprf_saturated(gpu, cpuref, q):
    """tree [2, 1, 1], a0 = q - 1, a1 = crt of the constant whose digits are all -1: every product of the root at x = 1
    is (q-1)^2, A_T(1) = ell mod q; every input against the restatement"""
    plan, R = _plan(gpu, sat.KHPRF_M, [q])
    base = sat.pick_base([q])
    ell = plan.decomposeLen(base)
    a0 = np.full((ell, R.n), q - 1, dtype=np.int64)
    a1 = np.full((ell, R.n), sat.all_minus_one(q, base) % q, dtype=np.int64)
    got = gpu.KHPRF(plan, base, [2, 1, 1], a0, a1).eval(0, 4).cpu().numpy()
    assert (got[1] == ell % q).all()
    for x in range(4):
        assert np.array_equal(got[x], kr.eval_tree(cpuref, R, base, [2, 1, 1], a0, a1, x)), x


def test_khprf_sixteen_digits_per_sum(gpu, cpuref):
    """just below 2^30 fold_for allows 16 digits per sum and no all-(-1) base has that many: base 2 (ell = 30) with the
    constant -(2^17 - 1), seventeen digits of -1 and thirteen of 0, fills the first sum and starts the second with
    (q-1)^2 (a seventeenth term in the first would overflow): A_T(1) = 17"""
    q = sat.class_top(sat.KHPRF_M, "30")[0]
    plan, R = _plan(gpu, sat.KHPRF_M, [q])
    ell = plan.decomposeLen(2)
    assert ell == 30 and sat.fold_for(q, ell) == 16
    a0 = np.full((ell, R.n), q - 1, dtype=np.int64)
    a1 = np.full((ell, R.n), q - (2 ** 17 - 1), dtype=np.int64)
    got = gpu.KHPRF(plan, 2, [2, 1, 1], a0, a1).eval(0, 4).cpu().numpy()
    assert (got[1] == 17).all()
    for x in range(4):
        assert np.array_equal(got[x], kr.eval_tree(cpuref, R, 2, [2, 1, 1], a0, a1, x)), x


@pytest.mark.parametrize("q", KHPRF_QS, ids=KHPRF_IDS)
def test_khprf_random_at_the_class_tops(gpu, cpuref, q):
    """random a0, a1 at the same moduli: every input of [2, 1, 1] and of the left spine of three leaves, and the full PRF
    with p = 2"""
    plan, R = _plan(gpu, sat.KHPRF_M, [q])
    base = sat.pick_base([q])
    ell = plan.decomposeLen(base)
    rng = np.random.default_rng(q % 1000)
    a0, a1 = (rng.integers(0, q, size=(ell, R.n), dtype=np.int64) for _ in range(2))
    a0[0], a1[0] = q - 1, q - 1
    s = rng.integers(0, q, size=(R.n,), dtype=np.int64)
    for tree in ([2, 1, 1], gpu.left_spine_tree(3)):
        f = gpu.KHPRF(plan, base, tree, a0, a1)
        dom = 2 ** tree[0]
        got = f.eval(0, dom).cpu().numpy()
        for x in range(dom):
            assert np.array_equal(got[x], kr.eval_tree(cpuref, R, base, tree, a0, a1, x)), (tree, x)
        if tree[0] == 2:
            prf = f(s, 2, 0, dom).cpu().numpy()
            for x in range(dom):
                assert np.array_equal(prf[x], kr.ring_prf(cpuref, R, base, tree, a0, a1, s, 2, x)), (tree, x, "prf")


# ---------------------------------------------------------------------------------------------
# 6. k_ctmul, k_sk_eval, k_lift at the top of the range
# ---------------------------------------------------------------------------------------------
def test_ctmul_just_below_2_62(gpu, cpuref):
    """row 0: all four operands q - 1 (the cross term is 2 (q-1)^2); row 1: the same as -1; row 2: random"""
    qs = sat.class_top(64, "62", 2)
    P, R = _plan(gpu, 64, qs)
    rng = np.random.default_rng(62)
    ops = [R.random(rng, 3) for _ in range(4)]
    for o in ops:
        o[:2] = np.array(qs) - 1
    want = sr.ctmul_crt(cpuref, R, *ops)
    ins = [o.copy() for o in ops]
    for o in ins:
        o[1] = -1
    for g_, w in zip(P.ctMulCRT(*ins), want):
        assert np.array_equal(g_, w)
    for g_, w in zip(P.ctMulCRT(*[sat.neg_rep(o, qs) for o in ops]), want):
        assert np.array_equal(g_, w)


def _lift_setup(gpu, cpuref):
    """m = 64, the plaintext modulus p = the largest good prime below 2^62 and the 16 next ones as ciphertext moduli;
    decoding-basis integers [B][n]: -1 (every residue q_i - 1), 0, either side of the sign break, then the boundary
    values of tests/test_decrypt.py"""
    m = 64
    tops = sat.class_top(m, "62", 17)
    p, qs = tops[0], tops[1:]
    pq, R = _plan(gpu, m, qs)
    Q = prod(qs)
    H = (Q - 1) // 2
    rng = np.random.default_rng(16)
    B, n = 2, pq.n
    xs = [-1, 0, H, -H] + _boundary_values(Q, rng, B * n - 4)
    assert _centred(H + 1, Q) == -H
    x = np.array(xs, dtype=object).reshape(B, n)
    res = np.ascontiguousarray(np.stack([(x % q).astype(np.int64) for q in qs], axis=-1))      # decoding basis, [0, q)
    assert (res[0, 0] == np.array(qs) - 1).all() and not res[0, 1].any()
    e_pow = cpuref.l(R, res).reshape(res.shape)                                                # powerful basis
    return p, qs, pq, R, Q, x, e_pow


def _int64_or_min(rows):
    return np.array([[v if -(2 ** 63) < v < 2 ** 63 else INT64_MIN for v in row] for row in rows], dtype=np.int64)


def test_error_term_and_decrypt_at_16_moduli_just_below_2_62(gpu, cpuref):
    p, qs, pq, R, Q, x, e_pow = _lift_setup(gpu, cpuref)
    qv = np.array(qs, dtype=np.int64)
    n = pq.n
    rng = np.random.default_rng(17)
    s_rand = np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=-1)
    want_e = _int64_or_min(xs_rows(x))
    want_msd = _int64_or_min([[_centred(3 * v, Q) for v in row] for row in xs_rows(x)])
    pp = gpu.Plan(lm.factor_pps(64), [p])
    Rp = Params(lm.factor_pps(64), [p])
    dec = (x % p).astype(np.int64)[..., None]
    want_pt = cpuref.l(Rp, np.ascontiguousarray(dec)).reshape(x.shape)                         # powerful basis of R_p
    e_crt = cpuref.crt(R, e_pow).reshape(e_pow.shape)
    # one component: the lift alone (k_lift<16, .>), powerful-basis and CRT-basis input, some residues in (-q, 0)
    neg = sat.neg_rep(e_pow, qs)
    for c0, crt_in in ((e_pow, False), (neg, False), (e_crt, True)):
        assert np.array_equal(pq.errorTerm([c0], s_rand, 2, cs_crt=crt_in), want_e), crt_in
        assert np.array_equal(pq.errorTerm([c0], s_rand, 3, enc="MSD", cs_crt=crt_in), want_msd), crt_in
        assert np.array_equal(pq.decrypt([c0], s_rand, pp, cs_crt=crt_in), want_pt), crt_in
    # two components in the CRT basis with c1 = s = q - 1 everywhere (c1 s = 1): k_sk_eval's Horner step is
    # (q-1)^2 + c0.  c0 = q - 1 everywhere makes it the largest there is, and the value 0 ...
    s_top = sat.full_q1((n,), qs)
    top = sat.full_q1((2, n), qs)
    assert not pq.errorTerm([top, top], s_top, 2, cs_crt=True).any()
    assert not pq.decrypt([top, top], s_top, pp, cs_crt=True).any()
    assert not pq.errorTerm([sat.neg_rep(top, qs), sat.neg_rep(top, qs)], sat.neg_rep(s_top, qs), 2, cs_crt=True).any()
    # ... and c0 = crt(e) - 1 makes it the planted values
    c0 = ((e_crt.astype(object) - 1) % np.array(qs, dtype=object)).astype(np.int64)
    assert np.array_equal(pq.errorTerm([c0, top], s_top, 2, cs_crt=True), want_e)
    assert np.array_equal(pq.decrypt([c0, top], s_top, pp, cs_crt=True), want_pt)
    # powerful-basis components: c1 = the constant -1 (crt: q - 1 everywhere), times s, plus c0 inside the lift
    c1_pow = np.zeros_like(e_pow)
    c1_pow[:, 0] = qv - 1
    c0_pow = e_pow.copy()
    c0_pow[:, 0] = (c0_pow[:, 0].astype(object) - 1) % np.array(qs, dtype=object)
    assert np.array_equal(pq.errorTerm([c0_pow, c1_pow], s_top, 2), want_e)
    assert np.array_equal(pq.decrypt([c0_pow, c1_pow], s_top, pp), want_pt)
