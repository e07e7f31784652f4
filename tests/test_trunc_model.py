"""CPU model (-m "not gpu") of the truncated-NTT route of the 61-bit fused poly-mul (k_pow2, MODE 2, AR 1).

The kernel stops both forward transforms after level L - 2, multiplies 4-coefficient residues
mod (X^4 - zeta) in registers (the base case) and starts the inverse at level L - 2.  This file
replays that exact level structure in Python integers, with the kernel's lazy ranges and its
approximate-quotient Shoup products, asserts every range on every intermediate value, and checks
the result against the oracle's polymul:

  forward (DIT, bit-reversed input)    entered as x + q in (0, 2q) (level 1: no trim), values in [0, 8q),
                                       Shoup products in [0, 4q)
  base case                            a-hat parked in [0, 2q), b-hat and zeta b-hat trimmed to
                                       [0, 2q); 128-bit sums < 16 q^2; one REDC per output < 3q + 1
  inverse (GS, levels L-2 .. 1)        values in [0, 4q); scale (n/4)^-1 2^64 on level 1

Group layout: after level L - 2 the positions x, x + N, x + 2N, x + 3N (N = 2^(L-2), x < N)
hold coefficients 0, 2, 1, 3 of a residue mod X^4 - zeta_x, zeta_x = psi^(4 (2x + 1)): the
level-(L-2) twiddle of x mod N/2, negated when x >= N/2.
"""
import numpy as np
import pytest

from oracle import lolmath as lm
from oracle.oracle import Params

M64 = (1 << 64) - 1


def _q_above(L, lower):
    return lm.first_good_q(1 << (L + 1), lower)


def _q_below(L, upper):
    m = 1 << (L + 1)
    q = (upper // m) * m + 1
    while q >= upper or not lm.is_prime(q):
        q -= m
    return q


# q just above 2^60 (the benchmark's rule) and just below 2^61 (the top of class 1); both are
# 1 mod 2^15, so they serve every L here
Q_LO = _q_above(14, 1 << 60)
Q_HI = _q_below(14, 1 << 61)


def shoup_pair(w, q):
    return w, (w << 64) // q


def shoup_acc(y, w, wp, q, init):
    """zq_dev.h shoup_acc: init + w y - Q q (mod 2^64) with the approximate quotient
    Q = wp.hi y.hi + hi32(wp.hi y.lo) + hi32(wp.lo y.hi); returns (result, result - init)."""
    assert 0 <= y <= M64
    wph, wpl, yh, yl = wp >> 32, wp & 0xFFFFFFFF, y >> 32, y & 0xFFFFFFFF
    Q = wph * yh + ((wph * yl) >> 32) + ((wpl * yh) >> 32)
    t = (w * y - Q * q) & M64
    assert 0 <= t < 4 * q, "Shoup product out of [0, 4q)"
    return (init + t) & M64, t


def csub(x, m):
    return x - m if x >= m else x


class Model:
    def __init__(self, L, q):
        self.L, self.q, self.n = L, q, 1 << L
        P = Params([(2, L + 1)], [q])
        self.P = P
        n = self.n
        ru, rui = P.ru[0], P.ruinv[0]
        # level s = 1..L: entry [N/2 + i] = psi_N^(+-(2i+1)), N = 2^s (plan.cpp)
        self.fwd = [None] * n
        self.inv = [None] * n
        for s in range(1, L + 1):
            N = 1 << s
            for i in range(N // 2):
                ex = (n // N) * (2 * i + 1)
                self.fwd[N // 2 + i] = shoup_pair(ru[ex], q)
                self.inv[N // 2 + i] = shoup_pair(rui[ex], q)
        S4 = pow(n // 4, -1, q) * pow(2, 64, q) % q          # (n/4)^-1 2^64: the truncated route's scale
        self.sc = shoup_pair(S4, q)
        self.l1 = shoup_pair(rui[n // 2] * S4 % q, q)        # psi_2^-1 times the same
        x = pow(-q, -1, 1 << 64)
        self.nqinv = x

    def fwd_levels(self, v, last):
        q, n = self.q, self.n
        for s in range(1, last + 1):
            N = 1 << s
            h = N // 2
            for x in range(n):
                if x & h:
                    continue
                X, Y = v[x], v[x + h]
                assert 0 <= X < 8 * q and 0 <= Y < 8 * q, "forward input out of [0, 8q)"
                w, wp = self.fwd[h + (x & (h - 1))]
                if s == 1:                   # entered as x + q in (0, 2q): level 1 has no trim (bfly_fwd L1)
                    assert X < 2 * q
                    xx = X
                else:
                    xx = csub(X, 4 * q)
                Xn, _ = shoup_acc(Y, w, wp, q, xx)
                v[x], v[x + h] = Xn, 2 * xx + 4 * q - Xn
                assert 0 <= v[x] < 8 * q and 0 <= v[x + h] < 8 * q
        return v

    def inv_levels(self, v, first):
        q, n = self.q, self.n
        for s in range(first, 0, -1):
            N = 1 << s
            h = N // 2
            for x in range(n):
                if x & h:
                    continue
                X, Y = v[x], v[x + h]
                assert 0 <= X < 4 * q and 0 <= Y < 4 * q, "inverse input out of [0, 4q)"
                sm, d = X + Y, X + 4 * q - Y
                if s == 1:
                    v[x], _ = shoup_acc(sm, *self.sc, q, 0)
                    v[x + h], _ = shoup_acc(d, *self.l1, q, 0)
                else:
                    w, wp = self.inv[h + (x & (h - 1))]
                    v[x] = csub(sm, 4 * q)
                    v[x + h], _ = shoup_acc(d, w, wp, q, 0)
                assert 0 <= v[x] < 4 * q and 0 <= v[x + h] < 4 * q
        return v

    def redc(self, T):
        q = self.q
        assert 0 <= T < 16 * q * q, "base-case sum out of [0, 16 q^2)"
        lo, hi = T & M64, T >> 64
        m = (lo * self.nqinv) & M64
        r = hi + ((m * q) >> 64) + (lo != 0)
        assert (r - T * pow(2, -64, q)) % q == 0
        assert 0 <= r < 3 * q + 1, "REDC result out of [0, 3q]"
        return r

    def base_case(self, va, vb):
        """va: parked a-hat in [0, 2q); vb: b-hat in [0, 8q).  Returns the REDC outputs (< 3q + 1)."""
        q, n = self.q, self.n
        N = n // 4
        c = [0] * n
        pos = [0, 2 * N, N, 3 * N]           # coefficient k sits at x + N bitrev2(k)
        for x in range(N):
            w, wp = self.fwd[N // 2 + (x & (N // 2 - 1))]
            if x & (N // 2):                 # zeta_x = -psi_N^(2 (x - N/2) + 1)
                w, wp = q - w, M64 - wp
            a = [va[x + p] for p in pos]
            braw = [vb[x + p] for p in pos]
            for y in a:
                assert 0 <= y < 2 * q
            b = [csub(csub(y, 4 * q), 2 * q) for y in braw]
            zb = [None] + [csub(shoup_acc(b[j], w, wp, q, 0)[0], 2 * q) for j in range(1, 4)]
            for y in b + zb[1:]:
                assert 0 <= y < 2 * q
            for k in range(4):
                T = sum(a[i] * (b[k - i] if i <= k else zb[k - i + 4]) for i in range(4))
                c[x + pos[k]] = self.redc(T)
        return c

    def polymul(self, a, b):
        """a, b: reference-style int inputs in (-q, q), stored (bit-reversed) order."""
        q, L = self.q, self.L
        va = self.fwd_levels([(int(y) + q) & M64 for y in a], L - 2)        # from_i64_fwd
        va = [csub(csub(y, 4 * q), 2 * q) for y in va]       # park_fwd
        vb = self.fwd_levels([(int(y) + q) & M64 for y in b], L - 2)
        v = self.inv_levels(self.base_case(va, vb), L - 2)
        out = []
        for y in v:
            y = csub(csub(y, 2 * q), q)                       # canon_inv
            assert 0 <= y < q
            out.append(y)
        return out


def _inputs(kind, q, n, rng):
    if kind == "random":
        return rng.integers(0, q, size=n, dtype=np.int64), rng.integers(0, q, size=n, dtype=np.int64)
    if kind == "allmax":
        return np.full(n, q - 1, dtype=np.int64), np.full(n, q - 1, dtype=np.int64)
    # reference-style negative representatives, extreme magnitudes mixed in
    a = -rng.integers(1, q, size=n, dtype=np.int64)
    b = rng.integers(-(q - 1), q, size=n, dtype=np.int64)
    a[::7] = -(q - 1)
    b[::5] = q - 1
    return a, b


@pytest.mark.parametrize("q", [Q_LO, Q_HI], ids=["q2^60", "q2^61-"])
@pytest.mark.parametrize("L", [11, 12, 13, 14])
def test_trunc_model_vs_oracle(cpuref, L, q):
    rng = np.random.default_rng(1000 * L + (q & 0xFFFF))
    M = Model(L, q)
    n = 1 << L
    for kind in ("random", "allmax", "negative"):
        a, b = _inputs(kind, q, n, rng)
        got = np.array(M.polymul(a, b), dtype=np.int64)
        want = cpuref.polymul(M.P, a.reshape(1, n, 1), b.reshape(1, n, 1)).reshape(n)
        assert np.array_equal(got, np.mod(want, q)), kind


def test_trunc_model_squaring(cpuref):
    L, q = 12, Q_HI
    rng = np.random.default_rng(5)
    M = Model(L, q)
    a, _ = _inputs("negative", q, 1 << L, rng)
    got = np.array(M.polymul(a, a), dtype=np.int64)
    want = cpuref.polymul(M.P, a.reshape(1, -1, 1), a.reshape(1, -1, 1)).reshape(-1)
    assert np.array_equal(got, np.mod(want, q))
