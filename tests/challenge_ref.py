"""Numpy / Python-integer model of whole RLWE / RLWR challenges (the lolhip_chall_* section of include/lolhip.h) for
the tests, built on tests/rlwe_ref.py and the CPU oracle's transforms: I instances of L samples, item b = i L + l under
secret i, every array in the decoding basis.  Test infrastructure only."""
import numpy as np

import enc_ref as er
import rlwe_ref as rr
import rlwe_ring_ref as ring
from oracle.oracle import Params

DISC, CONT, RLWR = 0, 1, 2
INT64_MAX = rr.INT64_MAX


class Model:
    """the transforms of one (m, qs) over the CPU oracle; arrays are [B][n][T] int64"""

    def __init__(self, cpuref, m, qs):
        self.cr, self.m, self.qs = cpuref, m, [int(q) for q in qs]
        self.pps = rr.factor_pps(m)
        self.n, self.T = rr.totient(self.pps), len(qs)
        self.P = Params(self.pps, self.qs)
        self.qv = np.array(self.qs, dtype=object)

    def _sh(self, y):
        return np.ascontiguousarray(np.asarray(y, dtype=np.int64).reshape(-1, self.n, self.T))

    def canon(self, y):
        return (self._sh(y).astype(object) % self.qv).astype(np.int64)

    def to_crt(self, y_dec):
        y = self.canon(y_dec)
        return np.asarray(self.cr.crt(self.P, self.cr.l(self.P, y))).reshape(y.shape)

    def to_dec(self, y_crt):
        y = self._sh(y_crt)
        return np.asarray(self.cr.linv(self.P, self.cr.crtinv(self.P, y))).reshape(y.shape)

    def mul_grouped(self, a_crt, s_crt, L):
        """a_b s_(b / L) in the CRT basis"""
        s = np.repeat(self._sh(s_crt), L, axis=0).astype(object)
        return ((self._sh(a_crt).astype(object) * s) % self.qv).astype(np.int64)

    def stream_dec(self, u):
        """the uniform residues of a stream item (CRT basis on this route) in the decoding basis"""
        return self.to_dec(u)

    def x_grouped(self, a_dec, s_dec, L):
        """the decoding-basis residues of a_b s_(b / L), [B][n][T]"""
        return self.to_dec(self.mul_grouped(self.to_crt(a_dec), self.to_crt(s_dec), L))

    def lift(self, r):
        """the centred lift of residues [B][n][T] to Python integers [B][n]: X in [0, Q), X - Q when 2 X >= Q"""
        r = self.canon(r).astype(object)
        Q, x = 1, np.zeros(r.shape[:2], dtype=object)
        for t, q in enumerate(self.qs):
            # x + Q k = r_t (mod q)
            k = ((r[..., t] - x) * pow(Q, -1, q)) % q
            x, Q = x + Q * k, Q * q
        return np.where(2 * x < Q, x, x - Q)


class RingModel:
    """one modulus q without a CRT basis (tests/rlwe_ring_ref.py): the stream items are powerful-basis coefficients and
    a s is the exact ring product; arrays [B][n][1]"""

    def __init__(self, m, q):
        self.m, self.qs = m, [int(q)]
        self.pps = rr.factor_pps(m)
        self.n, self.T = rr.totient(self.pps), 1
        self.qv = np.array(self.qs, dtype=object)

    def _sh(self, y):
        return np.asarray(y, dtype=np.int64).reshape(-1, self.n)

    def canon(self, y):
        return (np.asarray(y, dtype=np.int64).reshape(-1, self.n, 1).astype(object) % self.qv).astype(np.int64)

    def stream_dec(self, u):
        return ring.linv_mod(self.m, self._sh(u), self.qs[0])[..., None]

    def x_grouped(self, a_dec, s_dec, L):
        q = self.qs[0]
        a_pow, s_pow = ring.l_mod(self.m, self._sh(a_dec), q), ring.l_mod(self.m, self._sh(s_dec), q)
        prod = np.concatenate([ring.product(self.m, q, a_pow[i * L:(i + 1) * L], s_pow[i]) for i in range(len(s_pow))])
        return ring.linv_mod(self.m, prod, q)[..., None]

    def lift(self, r):
        return ring.lift(self.canon(r)[..., 0], self.qs[0]).astype(object)


# ---- generate: the stream contract ------------------------------------------------------------------------------------
def generate(M, kind, I, L, svar, p, key, ctr_s, ctr):
    """dict of s, a (decoding basis, exact), b, and e: RLWR b is exact; the Disc e is the restated rounded Gaussian (a
    device coefficient within 1e-9 of a tie may round the other way) and the Cont b carries the restated Gaussians (the
    device's agree to 1e-12 relative), so their b is the model's own and exact only under the model"""
    B, n, q = I * L, M.n, M.qs[0]
    s_crt = rr.uniform(key, rr.DOM_RLWE_SECRET, ctr_s, I, n, M.qs)
    a_crt = rr.uniform(key, rr.DOM_RLWE_UNIFORM, ctr, B, n, M.qs)
    out = {"s": M.stream_dec(s_crt), "a": M.stream_dec(a_crt), "e": None}
    x = M.x_grouped(out["a"], out["s"], L)
    if kind == RLWR:
        out["b"] = rr.rlwr_round(x[..., 0], q, p)
        return out
    g = rr.gaussian_dec(M.pps, key, ctr, B, svar)
    if kind == CONT:
        out["e"], out["b"] = g, rr.cont_sample(x[..., 0], g, q)
        return out
    e, _ = er.round_coset(g, np.zeros((B, n), dtype=np.int64), 1)
    out["e"] = e
    out["b"] = ((x.astype(object) + np.asarray(e).astype(object)[..., None]) % M.qv).astype(np.int64)
    return out


# ---- verify ---------------------------------------------------------------------------------------------------------------
def sample_values(M, kind, L, s_dec, a_dec, b, p=0):
    """per sample, what the verdict reduces: the Disc norms (int64, saturated), the Cont norms (float64), the RLWR
    mismatch counts"""
    x = M.x_grouped(a_dec, s_dec, L)
    q = M.qs[0]
    if kind == RLWR:
        return (rr.rlwr_round(x[..., 0], q, p) != np.asarray(b).reshape(-1, M.n)).sum(axis=1).astype(np.int64)
    if kind == CONT:
        return rr.gsqnorm_f64(M.pps, rr.cont_error(x[..., 0], np.asarray(b, dtype=np.float64).reshape(-1, M.n), q))
    e = M.lift(M.canon(b).astype(object) - x.astype(object))
    return np.array([min(v, INT64_MAX) for v in rr.gsqnorm_int(M.pps, e)], dtype=np.int64)


def verdict(kind, vals, L, bound=0):
    """(fails int32 [I], worst [I]) of per-sample values [I L]"""
    v = np.asarray(vals).reshape(-1, L)
    if kind == RLWR:
        return (v != 0).sum(axis=1).astype(np.int32), v.max(axis=1).astype(np.int64)
    if kind == CONT:
        worst = np.where(np.isnan(v).any(axis=1), np.nan, np.nanmax(np.where(np.isnan(v), -np.inf, v), axis=1))
        return (~(float(bound) > v)).sum(axis=1).astype(np.int32), worst
    ok = np.array([[int(bound) > int(x) and int(x) != INT64_MAX for x in row] for row in v])
    return (~ok).sum(axis=1).astype(np.int32), v.max(axis=1).astype(np.int64)


def verify(M, kind, L, s_dec, a_dec, b, bound=0, p=0):
    return verdict(kind, sample_values(M, kind, L, s_dec, a_dec, b, p), L, bound)
