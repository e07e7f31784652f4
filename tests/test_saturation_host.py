"""The saturating inputs of tests/saturate.py, proved on the CPU (no GPU): the evidence that tests/test_saturation.py
drives every lazy accumulator of the SymmSHE pipeline kernels to the bound its reduction interval relies on.

    construction    sr.decompose of saturating_c2 is q - 1 at coefficient 0 and 0 elsewhere in every digit and component,
                    and sr.keyswitch with the all-(q - 1) hint is L mod q everywhere; the chosen bases are pinned
    the inputs bite the accumulate-and-reduce schedule of every kernel, replayed in Python integers over the raw terms
                    those inputs produce: the largest pre-reduction sum is interval * (q-1)^2 + carry, below the
                    accumulator's capacity (headroom printed; DESIGN.md 3.4d holds the table), while the random inputs of
                    test_wide_knapsack stay below half of it
    fold_for        the KHPRF's digits-per-sum rule restated: maximal, 1 at the top of [2^31, 2^32), 4 just below 2^31

The intervals are read off the kernel sources and stated here as constants: a change there has to change this file.
"""
from fractions import Fraction
from math import log, log2, prod

import numpy as np
import pytest

import khprf_ref as kr
import saturate as sat
from oracle import lolmath as lm
from oracle import she_ref as sr
from oracle.oracle import Params
from test_rns_width import PIPE, PIPE_IDS, _extreme

# raw terms between reductions and accumulator width, as the sources have them
KS_POW2 = ("k_keyswitch<L,AR>", 16, 64)              # kernels.hip: (j & 15) == 15
KS_MIXED = ("k_mixed_keyswitch", 8, 64)              # mixed_ks.hip: (j & 7) == 7
KN_Q32 = ("k_knapsack<K,true>", 32, 64)              # pipeline.hip: (j & 31) == 31, every q < 2^29
KN_WIDE = ("k_knapsack<K,false>", 8, 128)            # pipeline.hip: (j & 7) == 7
KHPRF_WIDE = 8                                       # khprf.hip launch_khprf_node: 128-bit sums, q >= 2^32

# one row per class top: (m, class bound, T) -> (base pick_base must choose, L, the kernels whose window these L terms fill)
ROWS = [
    (32, "27", 3, 5, 36, [KS_POW2, KN_Q32]),          # arith32 == 4; unfused: the Q32 knapsack
    (32, "29", 3, 8, 30, [KS_POW2]),                  # L < 32: the Q32 knapsack's window is filled by the direct test
    (32, "30", 3, 4, 45, [KS_POW2, KN_WIDE]),         # the top of the fused key switch; unfused: 128-bit knapsack
    (32, "31", 2, 6, 24, [KN_WIDE]),
    (32, "32", 1, 4, 16, [KN_WIDE]),
    (45, "B13", 2, 5, 26, [KS_MIXED, KN_WIDE]),       # the class-2 limit of the vector interpreter
    (45, "27", 2, 5, 24, [KS_MIXED]),                 # class 4
    (32, "61", 2, 6, 48, [KN_WIDE]),
    (32, "62", 2, 4, 62, [KN_WIDE]),
]
# every (tuple, base) of the GPU tests' key switches: a silent change of pick_base shows up here
PINNED_BASES = {(32, "30", 3): 4, (32, "27", 3): 5, (2048, "30", 3): 4, (2048, "27", 3): 5, (2 ** 15, "30", 3): 4,
                (2 ** 15, "27", 3): 5, (45, "B13", 2): 5, (45, "27", 2): 5, (1728, "B13", 2): 5, (1728, "27", 2): 5,
                (11648, "B13", 2): 5, (11648, "27", 2): 5}
PINNED_KHPRF = [(8, 10), (4, 15), (6, 12), (4, 16), (5, 14), (6, 24)]      # (base, ell) per sat.khprf_moduli()


def replay(terms, interval, q):
    """acc += term_j; after every `interval`-th term acc = acc mod q (the kernels' schedule, j counted over all
    digits).  Returns (largest sum handed to a reduction or left at the end, its carry-in, terms in its window)."""
    acc = carry = cnt = 0
    best = (0, 0, 0)
    for j, t in enumerate(terms):
        acc += int(t)
        cnt += 1
        if acc > best[0]:
            best = (acc, carry, cnt)
        if j % interval == interval - 1:
            acc %= q
            carry, cnt = acc, 0
    return best


def headroom(cap_bits, value):
    """log2(2^cap / value), also where the gap is far below a double's resolution"""
    gap = Fraction(2 ** cap_bits - value, 2 ** cap_bits)
    return cap_bits - log2(value) if gap > Fraction(1, 2 ** 20) else float(gap) / log(2)


def _report(lines):
    print()
    for ln in lines:
        print("    " + ln)


# ---------------------------------------------------------------------------------------------
# 0. the helpers themselves
# ---------------------------------------------------------------------------------------------
def test_class_tops_are_the_largest_good_primes_below_their_bounds():
    for m in (32, 45, 64):
        for kind, bound in sat.BOUNDS.items():
            qs = sat.class_top(m, kind, 3)
            assert qs == sorted(qs, reverse=True) and len(set(qs)) == 3 and qs[0] < bound
            assert all(lm.is_prime(q) and q % m == 1 for q in qs)
            between = [q for q in range(qs[2], bound, m) if lm.is_prime(q)]     # q = 1 mod m
            assert between == qs[::-1], (m, kind)
    q = sat.class_top(45, "B13")[0]
    assert 13 * (q - 1) ** 2 < 2 ** 64 <= 13 * (lm.first_good_q(45, sat.B13) - 1) ** 2
    assert sat.good_below(32, 2 ** 30) == sat.good_below(32, 2 ** 30, 1)[0]


def test_edge_of_the_construction():
    """where there is no all-(-1) value: base 2 and 3 always; base 4 below 2^27, 2^29 and 2^31; just above 2^30 every
    power of two but 16"""
    for kind in sat.BOUNDS:
        for m in (32, 45):
            q = sat.class_top(m, kind)[0]
            assert sat.all_minus_one(q, 2) is None and sat.all_minus_one(q, 3) is None
            assert sat.all_minus_one(q, 0) == -1
            for b in range(2, 65):                            # the rule, against the digits peeled one by one
                k = sr.gadlen(b, q)
                v = -((b ** k - 1) // (b - 1))
                assert (sat.all_minus_one(q, b) == v) == (2 * -v <= q - 1 and b > 2), (q, b)
    for kind, ok in (("27", False), ("29", False), ("30", True), ("31", False), ("32", True)):
        assert (sat.all_minus_one(sat.class_top(32, kind)[0], 4) is not None) == ok, kind
    above = lm.first_good_q(32, 2 ** 30)
    assert [b for b in (2, 4, 8, 16, 32, 64) if sat.all_minus_one(above, b) is not None] == [16]
    assert sat.pick_base([above], lo=2, hi=4) is None


# ---------------------------------------------------------------------------------------------
# 1. construction
# ---------------------------------------------------------------------------------------------
def _check_construction(cpuref, m, qs, base):
    R = Params(lm.factor_pps(m), qs)
    qv = np.array(qs, dtype=np.int64)
    c2 = sat.saturating_c2(R, base)[None]
    d = sr.decompose(R, c2, base)
    L = d.shape[0]
    assert (d[:, 0, 0, :] == qv - 1).all() and not d[:, 0, 1:, :].any(), (m, qs, base)
    hint = sat.full_q1((L, 2, R.n), qs)
    got = sr.keyswitch(cpuref, R, c2, base, hint)
    assert (got == L % qv).all(), (m, qs, base)
    return L


@pytest.mark.parametrize("m,kind,T", sat.KEYSWITCH_POW2 + sat.KEYSWITCH_MIXED)
def test_construction_at_every_gpu_tuple(cpuref, m, kind, T):
    qs = sat.class_top(m, kind, T)
    base = sat.pick_base(qs)
    assert base == PINNED_BASES[(m, kind, T)]
    for q in qs:                                             # the digits of the scalar, peeled one by one
        v = sat.all_minus_one(q, base)
        assert v is not None and sr.lift_centered(np.array([v % q]), q)[0] == v
    if lm.totient_pps(lm.factor_pps(m)) <= 1024:             # the larger indices run the closed form only on the GPU
        assert _check_construction(cpuref, m, qs, base) == sum(sr.gadlen(base, q) for q in qs)


@pytest.mark.parametrize("m,kind,T,base,L,kernels", ROWS)
def test_construction_at_every_row_of_the_table(cpuref, m, kind, T, base, L, kernels):
    qs = sat.class_top(m, kind, T)
    assert sat.pick_base(qs) == base
    assert _check_construction(cpuref, m, qs, base) == L


def test_construction_trivgad_fills_one_window(cpuref):
    """TrivGad at T = 16 moduli just below 2^30: 16 digits of -1, one full window of k_keyswitch"""
    qs = sat.class_top(32, "30", 16)
    assert _check_construction(cpuref, 32, qs, 0) == 16 == KS_POW2[1]


def test_construction_khprf(cpuref):
    """tree [2, 1, 1], a0 = q - 1, a1 = crt of the constant v, x = 1: A_T(1) = ell mod q everywhere"""
    picked = []
    for q in sat.khprf_moduli():
        R = Params(lm.factor_pps(sat.KHPRF_M), [q])
        base = sat.pick_base([q])
        ell = sr.gadlen(base, q)
        picked.append((base, ell))
        a0 = np.full((ell, R.n), q - 1, dtype=np.int64)
        a1 = np.full((ell, R.n), sat.all_minus_one(q, base) % q, dtype=np.int64)
        assert (cpuref.crtinv(R, a1.reshape(ell, R.n, 1)).reshape(ell, R.n)[:, 1:] == 0).all()     # crt of a constant
        assert (kr.eval_tree(cpuref, R, base, [2, 1, 1], a0, a1, 1) == ell % q).all(), q
    assert picked == PINNED_KHPRF


# ---------------------------------------------------------------------------------------------
# 2. the inputs bite
# ---------------------------------------------------------------------------------------------
def _saturating_terms(cpuref, m, qs, base):
    """raw products per (digit j, slot x, target s) of the saturating key switch: crt(digit_j) * hint, Python integers"""
    R = Params(lm.factor_pps(m), qs)
    d = sr.decompose(R, sat.saturating_c2(R, base)[None], base)
    L = d.shape[0]
    d_crt = cpuref.crt(R, np.ascontiguousarray(d.reshape(L, R.n, R.T))).reshape(L, R.n, R.T)
    hint = sat.full_q1((L, R.n), qs)
    return d_crt.astype(object) * hint.astype(object)


@pytest.mark.parametrize("m,kind,T,base,L,kernels", ROWS)
def test_saturating_key_switch_fills_every_window(cpuref, m, kind, T, base, L, kernels):
    qs = sat.class_top(m, kind, T)
    terms = _saturating_terms(cpuref, m, qs, base)
    assert terms.shape[0] == L
    lines = []
    for name, interval, cap in kernels:
        assert L >= interval, "a row lists only the kernels whose window it fills"
        for s, q in enumerate(qs):
            seen = {replay(terms[:, x, s], interval, q) for x in range(terms.shape[1])}
            assert len(seen) == 1                             # every slot carries the same sums
            top, carry, cnt = seen.pop()
            assert cnt == interval and top == interval * (q - 1) ** 2 + carry and 0 <= carry < q
            assert carry == (L // interval - 1) * interval % q        # (q-1)^2 = 1 (mod q): the last full window carries most
            assert top < 2 ** cap
            assert interval * (q - 1) ** 2 + (q - 1) < 2 ** cap          # the bound relied on, whatever is carried
            if s == 0:
                lines.append(f"{name:22s} m={m:<3d} q={q:<20d} base {base} L={L:<3d} {interval:2d} terms: "
                             f"{headroom(cap, top):.3g} bits below 2^{cap}")
    _report(lines)


@pytest.mark.parametrize("m", [32, 45])
def test_saturating_knapsack_fills_every_window(m):
    """the direct knapsack test's rows 0 and 1 (xs, hint = q - 1): the Q32 form at L = 31 ... 65, the 128-bit form at
    L = 7 ... 17; one term short of the interval does not reach the bound, the interval itself does"""
    lines = []
    for (name, interval, cap), tuples, Ls in ((KN_Q32, [sat.class_top(m, "29", 3)], (31, 32, 33, 64, 65)),
                                              (KN_WIDE, sat.knapsack_wide(m), (7, 8, 9, 16, 17))):
        for qs in tuples:
            if name == KN_Q32[0]:
                assert max(qs) < 2 ** 29 <= lm.first_good_q(m, 2 ** 29)
            else:
                assert max(qs) >= 2 ** 29                     # the widest modulus moves the plan off Q32
            for q in qs:
                for L in Ls:
                    top, carry, cnt = replay([(q - 1) ** 2] * L, interval, q)
                    assert top < 2 ** cap
                    if L < interval:
                        assert top == L * (q - 1) ** 2 < interval * (q - 1) ** 2
                    else:
                        assert cnt == interval and top == interval * (q - 1) ** 2 + carry
                        assert carry == (L // interval - 1) * interval % q
                assert interval * (q - 1) ** 2 + (q - 1) < 2 ** cap
                lines.append(f"{name:22s} m={m:<3d} q={q:<20d} {interval:2d} terms: {headroom(cap, top):.3g} bits below 2^{cap}")
    _report(lines)
    # the dispatch threshold: with one more bit, 17 terms (the direct test's largest L off Q32) would not fit 64 bits
    q30 = sat.class_top(m, "30")[0]
    assert [q30 in qs for qs in sat.knapsack_wide(m)].count(True) == 1 and 17 * (q30 - 1) ** 2 >= 2 ** 64


def test_saturating_khprf_fills_every_window():
    lines = []
    cases = [(q, sat.pick_base([q])) for q in sat.khprf_moduli() + [sat.class_top(sat.KHPRF_M, "62")[0]]]
    for q, base in cases:
        ell = sr.gadlen(base, q)
        fold, cap = (sat.fold_for(q, ell), 64) if q < 2 ** 32 else (KHPRF_WIDE, 128)
        top, carry, cnt = replay([(q - 1) ** 2] * ell, fold, q)
        assert cnt == fold and top == fold * (q - 1) ** 2 + carry and top < 2 ** cap
        assert carry == (ell // fold - 1) * fold % q
        assert (q - 1) + fold * (q - 1) ** 2 < 2 ** cap
        lines.append(f"k_khprf_node<{'true' if cap == 64 else 'false'}>  q={q:<20d} base {base} ell={ell:<3d} "
                     f"{fold:2d} terms: {headroom(cap, top):.3g} bits below 2^{cap}")
    # just below 2^30 the rule allows 16 digits, and no all-(-1) base has that many: base 2 with v = -(2^17 - 1) has
    # seventeen digits of -1 and thirteen of 0: the first window full, and one more term in it would overflow
    q = sat.class_top(sat.KHPRF_M, "30")[0]
    v, ell = -(2 ** 17 - 1), sr.gadlen(2, q)
    digits = sr.decompose(Params([(2, 1)], [q]), np.array([[[v % q]]]), 2)[:, 0, 0, 0]
    assert ell == 30 and sat.fold_for(q, ell) == 16 and list(digits) == [q - 1] * 17 + [0] * 13
    top, carry, cnt = replay([int(d) * (q - 1) for d in digits], 16, q)
    assert (top, carry, cnt) == (16 * (q - 1) ** 2, 0, 16) and top < 2 ** 64 <= 17 * (q - 1) ** 2
    lines.append(f"k_khprf_node<true>   q={q:<20d} base 2 ell=30  16 terms: {headroom(64, top):.3g} bits below 2^64")
    _report(lines)


def test_two_term_sums_and_the_lift_at_the_top_of_the_range():
    """k_ctmul's cross term and k_sk_eval's Horner step hand rem128 a value whose high word must stay below q; k_lift
    adds up to 16 products v_i (P_i mod p) in one 128-bit sum"""
    tops = sat.class_top(64, "62", 17)
    p, qs = tops[0], tops[1:]                                  # decrypt's plaintext modulus: the largest of the class
    lines = []
    for q in tops[:2]:
        cross = 2 * (q - 1) ** 2                              # a0 b1 + a1 b0, every operand q - 1
        horner = (q - 1) ** 2 + (q - 1)                       # acc * s + c
        assert (cross >> 64) < q and (horner >> 64) < q and cross < 2 ** 128
        lines.append(f"k_ctmul / k_sk_eval    q={q:<20d} high word of 2 (q-1)^2: {log2(q) - log2(cross >> 64):.3g} bits below q")
    Ps = [prod(qs[:i]) for i in range(16)]
    total = sum((q - 1) * (P % p) for q, P in zip(qs, Ps))     # the row "all q_i - 1": every mixed-radix digit is q_i - 1
    assert sum((q - 1) * P for q, P in zip(qs, Ps)) == prod(qs) - 1
    assert total < 16 * (qs[0] - 1) * (p - 1) < 2 ** 128
    lines.append(f"k_lift<16,true>        p={p:<20d} 16 terms: {headroom(128, total):.3g} bits below 2^128 "
                 f"(worst case {headroom(128, 16 * (qs[0] - 1) * (p - 1)):.3g})")
    _report(lines)


@pytest.mark.parametrize("m,name,mk", PIPE, ids=PIPE_IDS)
def test_random_inputs_of_the_wide_knapsack_stay_below_half_the_capacity(m, name, mk):
    """the gap: test_wide_knapsack (tests/test_rns_width.py) at L = 4 leaves at least one bit of every accumulator unused"""
    qs = mk(m)
    R = Params(lm.factor_pps(m), qs)
    interval, cap = (KN_Q32[1:] if max(qs) < 2 ** 29 else KN_WIDE[1:])
    for K in (1, 2, 3):
        rng = np.random.default_rng(K * 7 + m)                # that test's inputs
        xs = np.stack([_extreme(R, rng, 3) for _ in range(4)])
        hint = np.stack([np.stack([R.random(rng, 1)[0] for _ in range(K)]) for _ in range(4)])
        hint[0, 0] = np.array(qs, dtype=np.int64) - 1
        terms = xs.astype(object)[:, None] * hint.astype(object)[:, :, None]          # [L][K][B][n][T]
        assert 4 < interval
        assert int(terms.sum(axis=0).max()) < 2 ** (cap - 1)


# ---------------------------------------------------------------------------------------------
# 3. fold_for
# ---------------------------------------------------------------------------------------------
def test_fold_for_is_the_largest_interval_that_fits():
    m = sat.KHPRF_M
    qs = [sat.class_top(m, k)[0] for k in ("27", "29", "30", "B13", "31", "32")]
    qs += [lm.first_good_q(m, 2 ** b) for b in (20, 29, 30, 31)] + [257, 3]
    for q in qs:
        for ell in (1, 2, 3, 4, 5, 15, 16, 17, 30, 64):
            f = sat.fold_for(q, ell)
            assert 1 <= f <= ell
            assert (q - 1) + f * (q - 1) ** 2 < 2 ** 64
            if f < ell:                                       # not capped at ell: one more digit would overflow
                assert 2 ** 64 <= (q - 1) + (f + 1) * (q - 1) ** 2
    assert sat.fold_for(sat.class_top(m, "32")[0], 64) == 1
    assert sat.fold_for(lm.first_good_q(m, 2 ** 31), 64) == 3
    assert sat.fold_for(sat.class_top(m, "31")[0], 64) == 4
    assert sat.fold_for(sat.class_top(m, "30")[0], 64) == 16
    assert sat.fold_for(sat.class_top(m, "29")[0], 64) == 64
    assert sat.fold_for(lm.first_good_q(m, 2 ** 32), 64) == KHPRF_WIDE == sat.fold_for(sat.class_top(m, "61")[0], 3)
