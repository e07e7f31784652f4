"""CPU restatement of the key-homomorphic ring PRF over q = 2^k (lol-apps KeyHomomorphicPRF.hs buildDecTree / ringPRF'
with ZP = Zq 2^k, which has no CRT basis) for the tests of lolhip_khprf_create_lifted.  Independent of the device
method: a ring product of two R_q elements is taken over the integers from their centred lifts, by an exact negacyclic
convolution when m = 2^e, otherwise through the CPU oracle at a prime Q' (different from the device's Q) and a centred
lift mod Q', and then reduced mod q.  One input at a time, no sharing.  Test infrastructure only.

Elements are powerful-basis coefficient vectors [.][n] of residues in [0, q); trees are preorder leaf counts."""
import numpy as np

from oracle import lolmath as lm
from oracle import she_ref as sr
from oracle.oracle import Params

import khprf_ref as kr


class LiftedRing:
    """R_q = Z_q[zeta_m] for q = 2^k, powerful basis, with exact products"""

    def __init__(self, cpu, m, q, prime_lower=2 ** 50):
        self.cpu, self.m, self.q = cpu, m, q
        self.pps = lm.factor_pps(m)
        self.n = lm.totient_pps(self.pps)
        self.pow2 = len(self.pps) == 1 and self.pps[0][0] == 2
        self.Pq = Params.__new__(Params)                      # only what she_ref.decompose reads
        self.Pq.qs, self.Pq.T, self.Pq.n = [q], 1, self.n
        self.Qp = lm.first_good_q(m, prime_lower)
        self.PQ = Params(self.pps, [self.Qp])

    def exponents(self):
        """m = 2^e: powerful-basis coefficient j is that of zeta^(bit reversal of j over e - 1 bits) (the basis is the
        tensor product of e - 1 two-dimensional factors, the first one innermost)"""
        bits = self.n.bit_length() - 1
        return np.array([int(format(j, f"0{bits}b")[::-1], 2) if bits else 0 for j in range(self.n)], dtype=np.int64)

    def _to_Q(self, a):
        return (sr.lift_centered(a, self.q) % self.Qp).astype(np.int64)

    def _from_Q(self, a):
        return (sr.lift_centered(a, self.Qp) % self.q).astype(np.int64)

    def mul(self, a, b):
        """a * b for [B][n] batches (b broadcast from [n] allowed) -> [B][n] in [0, q)"""
        a = np.atleast_2d(np.asarray(a, dtype=np.int64))
        b = np.broadcast_to(np.asarray(b, dtype=np.int64), a.shape)
        if self.pow2:
            n, out = self.n, np.zeros(a.shape, dtype=object)
            ex = self.exponents()
            for r in range(a.shape[0]):
                ea, eb = np.zeros(n, dtype=object), np.zeros(n, dtype=object)
                ea[ex] = sr.lift_centered(a[r], self.q)
                eb[ex] = sr.lift_centered(b[r], self.q)
                full = np.convolve(ea, eb)
                c = full[:n].copy()
                c[: n - 1] -= full[n:]                          # zeta^n = -1
                out[r] = c[ex]
            return (out % self.q).astype(np.int64)
        B, n = a.shape
        ca = self.cpu.crt(self.PQ, self._to_Q(a).reshape(B, n, 1))
        cb = self.cpu.crt(self.PQ, self._to_Q(b).reshape(B, n, 1))
        prod = self.cpu.crtinv(self.PQ, self.cpu.mul(self.PQ, ca, cb))
        return self._from_Q(prod.reshape(B, n))

    def linv(self, a):
        """lInv (powerful -> decoding basis) mod q: an integer map, applied at Q' to the centred lift"""
        if self.pow2:
            return np.asarray(a, dtype=np.int64)
        a = np.atleast_2d(np.asarray(a, dtype=np.int64))
        B, n = a.shape
        return self._from_Q(self.cpu.linv(self.PQ, self._to_Q(a).reshape(B, n, 1)).reshape(B, n))


def decompose_matrix(R, row, base):
    """G^-1 of the 1 x L row [L][n] (powerful, mod q) -> [L (digit i)][L (entry j)][n] digit residues mod q"""
    nL = row.shape[0]
    return sr.decompose(R.Pq, np.asarray(row).reshape(nL, R.n, 1), base).reshape(nL, nL, R.n)


def row_times(R, lval, dec):
    nL = lval.shape[0]
    out = np.zeros((nL, R.n), dtype=object)
    for i in range(nL):
        out += R.mul(dec[i], lval[i]).astype(object)            # entry j: sum_i L_i digit_i(A_r j)
    return (out % R.q).astype(np.int64)


def eval_tree(R, base, tree, a0, a1, x):
    """A_T(x) [L][n], powerful basis mod q"""
    def sub(x, t):
        if t[0] == "L":
            return np.asarray(a1 if x else a0, dtype=np.int64) % R.q
        _, _, lt, rt = t
        cr = kr.leaves(rt)
        return row_times(R, sub(x >> cr, lt), decompose_matrix(R, sub(x & ((1 << cr) - 1), rt), base))

    t = kr.parse(tree)
    assert 0 <= x < (1 << kr.leaves(t))
    return sub(x, t)


def rescale_dec(R, y, p):
    """rescaleDec to Z_p of powerful-basis elements [.][n] mod q: lInv, then fst (divModCent (p lift z) q) mod p"""
    dec = R.linv(y)
    quot, _ = sr.div_mod_cent(p * sr.lift_centered(dec, R.q), R.q)
    return (quot % p).astype(np.int64)


def ring_prf(R, base, tree, a0, a1, s, p, x):
    """ringPRF s x over R_q: [L][n] decoding-basis residues mod p (s in the powerful basis)"""
    A = eval_tree(R, base, tree, a0, a1, x)
    return rescale_dec(R, R.mul(A, np.asarray(s) % R.q), p)


# ---- the creation bound -----------------------------------------------------------------
def growth(m):
    """C_m = max_k sum_{i,j} |(b_i b_j)_k| over the powerful basis, per prime power as in the header"""
    C = 1
    for p, e in lm.factor_pps(m):
        pk = p ** e
        pk1, phi = pk // p, pk - pk // p
        acc = [0] * phi
        for t in range(2 * phi - 1):
            mult = min(t, 2 * phi - 2 - t) + 1
            tt = t % pk
            if tt < phi:
                acc[tt] += mult
            else:
                for l in range(p - 1):
                    acc[l * pk1 + tt - phi] += mult
        C *= max(acc)
    return C


def growth_bruteforce(cpu, m, prime_lower=2 ** 40):
    """the same C_m from the products of every pair of powerful-basis unit vectors through the CPU oracle"""
    pps = lm.factor_pps(m)
    n = lm.totient_pps(pps)
    Q = lm.first_good_q(m, prime_lower)
    P = Params(pps, [Q])
    E = cpu.crt(P, np.eye(n, dtype=np.int64).reshape(n, n, 1)).reshape(n, n)
    acc = np.zeros(n, dtype=np.int64)
    for i in range(n):
        prod = cpu.crtinv(P, cpu.mul(P, np.repeat(E[i:i + 1], n, 0).reshape(n, n, 1), E.reshape(n, n, 1)))
        acc += np.abs(sr.lift_centered(prod.reshape(n, n), Q).astype(np.int64)).sum(axis=0)
    return int(acc.max())


def max_digit(q, base):
    """the largest |digit| of the centred decomposition over lift_q (Numeric.hs:202-205)"""
    if base == 0:
        return q // 2
    v = np.arange(-q // 2, q // 2, dtype=object)
    P = Params.__new__(Params)
    P.qs, P.T = [q], 1
    d = sr.decompose(P, (v % q).astype(np.int64).reshape(-1, 1), base)
    return int(np.abs(sr.lift_centered(d, q).astype(np.int64)).max())


def bound(m, q, base):
    """the smallest Q the lifted family accepts is above 2 max(L C_m (q/2) max|digit|, C_m (q/2)^2)"""
    L = 1 if base == 0 else sr.gadlen(base, q)
    C = growth(m)
    return 2 * max(L * C * (q // 2) * max_digit(q, base), C * (q // 2) ** 2)
