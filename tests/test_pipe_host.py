"""What tests/test_pipe.py relies on, checked without a GPU (-m "not gpu").

  coverage   the case table of pipe_cases.py reaches all twelve k_pow2_pipe<L, AR, SQ> instantiations, and every
             arithmetic class with a modulus at the very top of its range
  rows       the closed-form products of the structured operand rows, against the oracle
  model      the 32-bit classes' fused poly-mul as the pipelined kernel enters it, replayed on numpy uint64 with every
             intermediate held to the range that the comments of pow2_impl.h state:

    entry                (low dword of x) + q mod 2^32, in (0, 2q) for every representative x in (-q, q)
    forward  AR = 2      Harvey's [0, 4q): X trimmed to [0, 2q), Shoup product in [0, 2q)
             AR = 3      [0, 2q): X and the product trimmed to [0, q)
             AR = 4      no trim: below 2q + 2kq after level k, and below 2^32 as an integer (no wrap)
    park_fwd             Shoup product by 2^32 mod q, trimmed: canonical
    pmul                 x = a b < q 2^32; REDC exact, below 2q (AR = 3: trimmed, canonical)
    inverse  AR = 2, 4   [0, 2q);  AR = 3 canonical;  last level scaled by n^-1
    canon_inv            canonical, and equal to the oracle's poly-mul

The butterflies run in the plain in-place order (level s pairs x and x + 2^(s-1)); the ranges do not depend on which
register holds which coefficient.  shoup32 is modelled with its exact integer value w y - floor(wp y / 2^32) q, asserted
inside [0, 2q): below 2^32 for q < 2^31, so the kernel's arithmetic mod 2^32 returns the same word.
"""
import numpy as np
import pytest

from oracle.oracle import Params

import pipe_cases as pc

U = np.uint64
M32 = U(0xFFFFFFFF)
TWO32 = 1 << 32


def test_case_table_reaches_all_twelve_instantiations():
    got = {(L, pc.arith_class(q), sq) for L, q, sq in pc.ROUTE_CASES}
    assert got == {(L, ar, sq) for L in (12, 13) for ar in (2, 3, 4) for sq in (False, True)} and len(got) == 12
    for q in pc.MODULI:
        assert q % 2 ** 14 == 1 and pc.lm.is_prime(q), q
    # both ends of every class; the top one within 64 steps of 2^14 of the class bound
    for ar, bound in pc.CLASS_BOUND.items():
        qs = [q for q in pc.MODULI if pc.arith_class(q) == ar]
        assert qs == [pc.BOTTOM[ar], pc.TOP[ar]], ar
        assert 0 < bound - pc.TOP[ar] <= 2 ** 14 * 64, (ar, pc.TOP[ar])
    assert pc.BOTTOM[2] >= 2 ** 27 and pc.BOTTOM[3] >= 2 ** 30 and pc.BOTTOM[2] - 2 ** 27 <= 2 ** 14 * 64
    # every (L, class) of the round shapes and of the real grid is among the routes
    assert {(L, pc.arith_class(q)) for L, q in pc.ROUND_PLANS} == {(13, 4), (13, 2), (13, 3), (12, 3)}
    assert pc.arith_class(pc.REAL_Q) == 2 and pc.REAL_Q == pc.TOP[2] and pc.REAL_L == 13


def test_round_shapes_give_one_two_and_three_iterations():
    assert max(B for G in pc.ROUND_GRIDS for B in pc.round_batches(G)) == pc.ROUND_BMAX == 14
    seen = set()
    for G in pc.ROUND_GRIDS:
        Bs = pc.round_batches(G)
        assert Bs == sorted(set(Bs)) and Bs[0] == 1
        for B in Bs:
            g = min(G, B)                                      # the launcher clamps the grid to B
            iters = [len(range(w, B, g)) for w in range(g)]
            seen.add((min(iters), max(iters)))
    # even rounds of 1, 2, 3 and ragged last rounds (some workgroups one iteration short) after 1 and 2
    assert {(1, 1), (2, 2), (3, 3), (1, 2), (2, 3)} <= seen


@pytest.mark.parametrize("L", pc.LS)
@pytest.mark.parametrize("q", pc.MODULI)
def test_closed_forms_against_oracle(cpuref, q, L):
    R = Params([(2, L + 1)], [q])
    a, b = pc.rows(q, L)
    assert a.shape == (9, 1 << L, 1) and np.abs(a).max() == q - 1 and a.min() == -(q - 1) and b.min() < 0
    for square in (False, True):
        want = cpuref.polymul(R, a, a if square else b).reshape(len(pc.ROW_NAMES), -1)
        cf = pc.closed_forms(q, L, a, b, square)
        assert set(cf) == set(pc.ROW_NAMES) - {"random", "random_signed"}
        for nm, v in cf.items():
            assert np.array_equal(want[pc.ROW[nm]], v), (nm, square)


# ---- the integer model --------------------------------------------------------------------------------------------
class Model:
    def __init__(self, L, q, entry_add=True):
        self.L, self.q, self.n, self.ar = L, q, 1 << L, pc.arith_class(q)
        self.entry_add = entry_add                             # False: the kernel without its `+ qk.q` (sensitivity check)
        self.R = Params([(2, L + 1)], [q])
        n, ru, rui = self.n, self.R.ru[0], self.R.ruinv[0]
        fw, iw = np.zeros(n, dtype=U), np.zeros(n, dtype=U)
        for s in range(1, L + 1):                              # plan.cpp: entry [N/2 + i] = psi_N^(+-(2i+1)), N = 2^s
            N = 1 << s
            ex = (n // N) * (2 * np.arange(N // 2) + 1)
            fw[N // 2:N] = np.asarray(ru, dtype=U)[ex]
            iw[N // 2:N] = np.asarray(rui, dtype=U)[ex]
        self.fw, self.iw = self.pair(fw), self.pair(iw)
        S = self.R.mhatinv[0]
        assert S == pow(n, -1, q)
        self.sc = self.pair(U(S))                              # plan.cpp d_scale32: S, then psi_2^-1 S
        self.l1 = self.pair(U(int(rui[n // 2]) * S % q))
        self.r = self.pair(U(TWO32 % q))                       # make_modctx: r32, r32p
        self.nqinv = U(pow(-q, -1, TWO32))
        self.fwd_max = {}                                      # AR = 4: largest forward value after each level
        self.entry = None

    def pair(self, w):
        return w, (w << U(32)) // U(self.q)                    # Shoup pair: wp = floor(w 2^32 / q)

    def shoup32(self, y, wwp):
        w, wp = wwp
        assert (y <= M32).all()
        Q = (wp * y) >> U(32)                                  # __umulhi(wp, y)
        t = w * y - Q * U(self.q)
        assert (t < U(2 * self.q)).all(), "Shoup product out of [0, 2q)"
        return t

    @staticmethod
    def csub32(x, m):
        assert (x <= M32).all()
        return np.minimum(x, (x - U(m)) & M32)

    def enter(self, x):
        """take(): the staged low dword plus q, mod 2^32"""
        q = self.q
        low = np.ascontiguousarray(x, dtype=np.int64).view(U) & M32
        raw = low + U(q if self.entry_add else 0)
        self.entry = (np.asarray(x), raw)
        v = raw & M32
        if self.entry_add:
            assert ((v > 0) & (v < U(2 * q))).all(), "entry out of (0, 2q)"
        return v

    def forward(self, v):
        q, n, ar, B = self.q, self.n, self.ar, v.shape[0]
        lim = {2: 4 * q, 3: 2 * q}
        for s in range(1, self.L + 1):
            h = 1 << (s - 1)
            v = v.reshape(B, n // (2 * h), 2, h)
            X, Y = v[:, :, 0, :], v[:, :, 1, :]
            tw = (self.fw[0][h:2 * h], self.fw[1][h:2 * h])
            if ar == 3:
                assert (v < U(lim[3])).all(), f"forward input out of [0, 2q) at level {s}"
                x = self.csub32(X, q)
                t = self.csub32(self.shoup32(Y, tw), q)
                assert (x < U(q)).all() and (t < U(q)).all()
                Xn, Yn = x + t, x + U(q) - t
                assert (Xn < U(2 * q)).all() and (Yn < U(2 * q)).all() and (Yn > 0).all()
            elif ar == 2:
                assert (v < U(lim[2])).all(), f"forward input out of [0, 4q) at level {s}"
                x = self.csub32(X, 2 * q)
                assert (x < U(2 * q)).all()
                t = self.shoup32(Y, tw)
                Xn, Yn = x + t, x + U(2 * q) - t
                assert (Xn < U(4 * q)).all() and (Yn < U(4 * q)).all()
            else:
                t = self.shoup32(Y, tw)
                Xn, Yn = X + t, X + U(2 * q) - t                # integers, not yet reduced mod 2^32
                top = int(max(Xn.max(), Yn.max()))
                self.fwd_max[s] = max(self.fwd_max.get(s, 0), top)
                assert top < 2 * q + 2 * s * q, f"level {s}: {top / q:.3f} q, stated bound {2 + 2 * s} q"
                assert top < TWO32, f"level {s}: {top} wraps a 32-bit word"
            v = np.stack([Xn, Yn], axis=2)
        return v.reshape(B, n)

    def park(self, v):
        p = self.csub32(self.shoup32(v, self.r), self.q)
        assert (p < U(self.q)).all()
        return p

    def pmul(self, a, b):
        q = self.q
        assert (a < U(q)).all() and (b <= M32).all()
        x = a * b
        assert int(x.max()) < q * TWO32, "pmul: a b out of [0, q 2^32)"
        m = ((x & M32) * self.nqinv) & M32
        tot = x + m * U(q)                                     # < 2 q 2^32 <= 2^64 - 2^33
        assert ((tot & M32) == 0).all()
        t = tot >> U(32)
        assert (t < U(2 * q)).all(), "REDC output out of [0, 2q)"
        if self.ar == 3:
            t = self.csub32(t, q)
            assert (t < U(q)).all()
        return t

    def inverse(self, v):
        q, n, ar, B = self.q, self.n, self.ar, v.shape[0]
        lim, off = (q, q) if ar == 3 else (2 * q, 2 * q)       # value range; the offset of the difference
        for s in range(self.L, 0, -1):
            h = 1 << (s - 1)
            v = v.reshape(B, n // (2 * h), 2, h)
            X, Y = v[:, :, 0, :], v[:, :, 1, :]
            assert (v < U(lim)).all(), f"inverse input out of range at level {s}"
            sm, d = X + Y, X + U(off) - Y
            assert (sm <= M32).all() and (d <= M32).all() and (d > 0).all()
            if s == 1:                                         # bfly_inv_last
                Xn, Yn = self.shoup32(sm, self.sc), self.shoup32(d, self.l1)
                if ar == 3:
                    Xn = self.csub32(Xn, q)
            else:
                Xn = self.csub32(sm, lim)
                Yn = self.shoup32(d, (self.iw[0][h:2 * h], self.iw[1][h:2 * h]))
            if ar == 3:
                Yn = self.csub32(Yn, q)
            assert (Xn < U(lim)).all() and (Yn < U(lim)).all(), f"inverse output out of range at level {s}"
            v = np.stack([Xn, Yn], axis=2)
        return v.reshape(B, n)

    def polymul(self, a, b, square=False):
        """a, b: int64 [B][n] representatives in (-q, q), stored order; the kernel's SQ path when square"""
        v = self.forward(self.enter(a))
        va = self.park(v)
        if not square:
            v = self.forward(self.enter(b))
        v = self.inverse(self.pmul(va, v))
        if self.ar != 3:
            v = self.csub32(v, self.q)                         # canon_inv
        assert (v < U(self.q)).all()
        return v.astype(np.int64)


@pytest.mark.parametrize("q", pc.MODULI)
def test_model_ranges_and_result_at_every_class_end(cpuref, q):
    L = 13                                                     # AR = 4's growth depends on the level count
    M = Model(L, q)
    a, b = pc.rows(q, L)
    B, n = a.shape[0], 1 << L
    for square in (False, True):
        got = M.polymul(a.reshape(B, n), b.reshape(B, n), square)
        want = cpuref.polymul(M.R, a, a if square else b).reshape(B, n)
        for nm, i in pc.ROW.items():
            assert np.array_equal(got[i], want[i]), (nm, square)
    if M.ar == 4:
        # not required to reach the bound: Shoup's lazy product exceeds q only by chance
        report = ", ".join(f"{s}: {M.fwd_max[s] / q:.3f}" for s in sorted(M.fwd_max))
        print(f"\nAR = 4, q = {q}: largest forward value after level k, in units of q (bound 2 + 2k; 2^32 = {TWO32 / q:.3f} q): {report}")
        assert sorted(M.fwd_max) == list(range(1, L + 1))
        assert 2 * q + 2 * 14 * q < TWO32                      # from_i64_fwd's claim, with a level to spare at L = 13


def test_model_entry_extremes_occur_at_the_top_of_class_3():
    L, q = 13, pc.TOP[3]
    assert 2 ** 31 - q <= 2 ** 20
    M = Model(L, q)
    a, _ = pc.rows(q, L)
    v = M.enter(a.reshape(a.shape[0], -1))
    x, raw = M.entry
    assert int(v.max()) == 2 * q - 1 and 2 * q - 1 >= 2 ** 32 - 2 ** 21         # x = q - 1: the top of a 32-bit word
    neg = x == -(q - 1)
    assert neg.any() and (raw[neg] == U(TWO32 + 1)).all() and (v[neg] == 1).all()    # the sum wraps: entry value 1
    assert (raw[x == -1] == U(TWO32 - 1 + q)).all() and (v[x == -1] == U(q - 1)).all()
    assert (x == 0).any() and (v[x == 0] == U(q)).all()
    # the sign bit of the staged dword is set exactly on the negative representatives
    low = x.astype(np.int64).view(U) & M32
    assert (((low >> U(31)) == 1) == (x < 0)).all()


def test_model_without_the_entry_offset_is_wrong():
    """the sensitivity check of the suite, on the model: drop the `+ q` of take() and every row with a negative
    representative leaves the lazy range or comes back wrong"""
    L, q = 12, pc.TOP[2]
    a, b = pc.rows(q, L)
    B, n = a.shape[0], 1 << L
    want = Model(L, q).polymul(a.reshape(B, n), b.reshape(B, n))
    for nm in ("negmax_max", "alternating", "minus_one", "random_signed"):
        i = pc.ROW[nm]
        try:
            got = Model(L, q, entry_add=False).polymul(a[i].reshape(1, n), b[i].reshape(1, n))
        except AssertionError:
            continue                                           # a stated range no longer holds
        assert not np.array_equal(got[0], want[i]), nm
