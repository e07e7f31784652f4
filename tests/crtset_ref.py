"""Step-by-step restatement of crtSetDec / crtSet / ptTunnel for the tests, from the mathematics (lol-cpp
CPP/Extension.hs:143-164, lol ZmStar.hs:52-88, Tensor.hs:300-313, UCyc.hs:540-565, Linear.hs:75-79), with Python
integers and its own tiny GF(p^d).  Nothing here comes from lol_amd/csrc: the field is found by trial division (the
library uses Rabin's test), twCRTs is multiplied out in the field (the library expands it into power traces), and ring
products go through one reduction table per index (the library reduces prime power by prime power per product).

The root of unity follows the rule stated in include/lolhip.h: GF(p^d) = F_p[x]/(f) with f the first irreducible
x^d + a_(d-1) x^(d-1) + ... + a_0 when (a_(d-1), ..., a_0) counts up as a base-p number from 0; gen the first element of
order p^d - 1 when c_0 + c_1 x + ... counts up as the base-p number sum c_i p^i from 1; w = gen^((p^d - 1)/m')."""
import functools
import itertools
import math

import numpy as np

from oracle import lolmath as lm


# ---- polynomials over F_p, constant coefficient first -----------------------------------------------------------------
def _trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _polyrem(a, f, p):
    """a mod f for monic f"""
    a = list(a)
    df = len(f) - 1
    for k in range(len(a) - 1, df - 1, -1):
        c = a[k] % p
        if c:
            for i in range(df + 1):
                a[k - df + i] = (a[k - df + i] - c * f[i]) % p
    return _trim([v % p for v in a[:df]])


def _digits(c, p, d):
    return [(c // p ** i) % p for i in range(d)]


def _irreducible(f, p):
    d = len(f) - 1
    if d >= 1 and f[0] == 0:
        return d == 1
    for k in range(1, d // 2 + 1):
        for c in range(p ** k):
            if not _polyrem(f, _digits(c, p, k) + [1], p):
                return False
    return True


class GF:
    """GF(p^d) by the stated rule; elements are tuples of d coefficients"""

    def __init__(self, p, d):
        self.p, self.d = p, d
        c = 0
        while not _irreducible(_digits(c, p, d) + [1], p):
            c += 1
        self.f = _digits(c, p, d) + [1]
        self.one = tuple([1 % p] + [0] * (d - 1))
        N = p ** d - 1
        exps = [N // r for r in lm.prime_factors(N)] if N > 1 else []
        c = 1
        while any(self.pow(self.elt(c), ex) == self.one for ex in exps):
            c += 1
        self.gen = self.elt(c)

    def elt(self, c):
        return tuple(_digits(c, self.p, self.d))

    def _fix(self, a):
        a = _polyrem(a, self.f, self.p)
        return tuple(a + [0] * (self.d - len(a)))

    def mul(self, a, b):
        t = [0] * (2 * self.d - 1)
        for i, x in enumerate(a):
            if x:
                for j, y in enumerate(b):
                    t[i + j] += x * y
        return self._fix(t)

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def pow(self, a, e):
        r = self.one
        while e:
            if e & 1:
                r = self.mul(r, a)
            a = self.mul(a, a)
            e >>= 1
        return r

    def trace(self, a):
        s, y = tuple([0] * self.d), a
        for _ in range(self.d):
            s = self.add(s, y)
            y = self.pow(y, self.p)
        assert not any(s[1:]), "a trace lies in F_p"
        return s[0]


def order(p, m):
    """ord_m(p) as ZmStar.order counts it (1 for m = 1)"""
    d, x = 1, p % m
    while x != 1 % m:
        x, d = x * p % m, d + 1
    return d


def count(m, m2, p):
    """K = (phi(m')/ord_m'(p)) / (phi(m)/ord_m(p))"""
    phi = lambda v: lm.totient_pps(lm.factor_pps(v)) if v > 1 else 1
    return (phi(m2) // order(p, m2)) // (phi(m) // order(p, m))


def cosets(p, m):
    """ZmStar.cosets: repeatedly split the coset of the smallest remaining element off Z_m^*"""
    s = {x % m for x in range(1, m + 1) if math.gcd(x, m) == 1}
    out = []
    while s:
        x = min(s)
        c, y = {x}, x * p % m
        while y != x:
            c.add(y)
            y = y * p % m
        out.append(c)
        s -= c
    return out


def partition_cosets(m, m2, p):
    """ZmStar.partitionCosets, line by line: a Map from the m-coset (a Set of residues) to the m'-cosets above it, each
    new coset prepended (insertWith' (++)); elems in key order; transpose; the smallest element of every coset"""
    part = {}
    for c in cosets(p, m2):
        key = tuple(sorted({x % m for x in c}))
        part[key] = [c] + part.get(key, [])
    cols = [part[k] for k in sorted(part)]
    assert len({len(col) for col in cols}) == 1
    return [[min(col[c]) for col in cols] for c in range(len(cols[0]))]


def _pps(m):
    return lm.factor_pps(m) if m > 1 else []


@functools.lru_cache(maxsize=None)
def crtset_dec(m, m2, p):
    """crtSetDec: [K][phi(m')] residues mod p, decoding basis; element c, entry j =
    mhat'^-1 Tr( sum_{i in reps_c} twCRTs(j, zmsToIndex i) ), twCRTs multiplied out in GF(p^d)"""
    assert m2 % m == 0 and m2 % p and lm.is_prime(p)
    pps2 = _pps(m2)
    n2 = lm.totient_pps(pps2) if pps2 else 1
    F = GF(p, order(p, m2))
    w = F.pow(F.gen, (p ** F.d - 1) // m2)
    wpow = [F.one]
    for _ in range(m2 - 1):
        wpow.append(F.mul(wpow[-1], w))
    hinv = pow(lm.value_hat(m2) % p, -1, p) if p > 1 else 0
    reps = partition_cosets(m, m2, p)
    out = []
    for rc in reps:
        row = []
        for j in range(n2):
            acc, jj, js = tuple([0] * F.d), j, []
            for pe in pps2:
                js.append(jj % lm.totient_pp(pe))
                jj //= lm.totient_pp(pe)
            for i in rc:
                term = F.one
                for (q, e), jk in zip(pps2, js):
                    pp = q ** e
                    wk = lambda ex, pp=pp: wpow[(m2 // pp) * (ex % pp) % m2]          # w_pp^ex
                    term = F.mul(term, wk(-lm.index_to_pow((q, e), jk) * (i % pp)))
                    if q != 2:
                        term = F.mul(term, F.sub(F.one, wk((i % pp) * q ** (e - 1))))  # 1 - w_q^i = sigma_i(g_q)
                acc = F.add(acc, term)
            row.append(hinv * F.trace(acc) % p)
        out.append(row)
    return out


# ---- the powerful basis of one index ------------------------------------------------------------------------------------
class PowRing:
    """products in the powerful basis of O_m through one table: zeta_m^a as a powerful-basis vector, a < m"""

    def __init__(self, m):
        self.m, self.pps = m, _pps(m)
        phis = [lm.totient_pp(pe) for pe in self.pps]
        self.n = math.prod(phis)
        strides = [math.prod(phis[:k]) for k in range(len(phis))]
        # basis element j = prod_k zeta_pp_k^pow_k(j_k) = zeta_m^expo[j]
        self.expo = []
        where = {}
        for j in range(self.n):
            jj, a, key = j, 0, []
            for pe, phi in zip(self.pps, phis):
                t = lm.index_to_pow(pe, jj % phi)
                jj //= phi
                a += t * (m // (pe[0] ** pe[1]))
                key.append(t)
            self.expo.append(a % m)
            where[tuple(key)] = j
        self.red = np.zeros((m, self.n), dtype=np.int64)
        for a in range(m):
            per_dim = []
            for (q, e) in self.pps:
                pp, phi = q ** e, (q - 1) * q ** (e - 1)
                t = a * pow(m // pp, -1, pp) % pp if pp > 1 else 0
                # z^t for t >= phi: Phi_{q^e}(z) = sum_{l < q} z^(l q^(e-1)) = 0
                per_dim.append([(1, t)] if t < phi else [(-1, l * q ** (e - 1) + t - phi) for l in range(q - 1)])
            for combo in itertools.product(*per_dim):
                sign = math.prod(s for s, _ in combo)
                self.red[a, where[tuple(t for _, t in combo)]] += sign
        self.expo = np.array(self.expo, dtype=np.int64)

    def mul_matrix(self, b):
        """M with a * b = a @ M for row vectors a (small integer entries)"""
        b = np.asarray(b, dtype=np.int64)
        T = np.zeros((self.n, self.m), dtype=np.int64)
        for i in range(self.n):
            np.add.at(T[i], (self.expo[i] + self.expo) % self.m, b)
        return T @ self.red

    def mul(self, a, b, mod):
        a = np.asarray(a, dtype=np.int64) % mod
        b = np.asarray(b, dtype=np.int64) % mod
        assert mod * mod * self.n < 2 ** 62
        return (a @ (self.mul_matrix(b) % mod)) % mod


@functools.lru_cache(maxsize=None)
def ring(m):
    return PowRing(m)


def _prime_axes(pps, y):
    """y [..., n] -> for every odd prime power a view [..., hi, p^(e-1), p - 1, rts] and its axis, first prime fastest"""
    n = y.shape[-1]
    rts = 1
    for (q, e) in pps:
        phi = (q - 1) * q ** (e - 1)
        if q != 2:
            yield y.reshape(y.shape[:-1] + (n // (phi * rts), q ** (e - 1), q - 1, rts))
        rts *= phi


def l_pow(pps, y, mod):
    """decoding -> powerful basis: prefix sums along every odd prime's axis"""
    y = np.array(y, dtype=np.int64)
    for v in _prime_axes(pps, y):
        np.cumsum(v, axis=-2, out=v)
    return y % mod


def l_inv(pps, y, mod):
    """powerful -> decoding basis: adjacent differences"""
    y = np.array(y, dtype=np.int64)
    for v in _prime_axes(pps, y):
        v[..., 1:, :] = v[..., 1:, :] - v[..., :-1, :]
    return y % mod


def embed_pow(m, m2, y):
    idx = lm.base_indices_pow(_pps(m), _pps(m2))
    y = np.asarray(y, dtype=np.int64)
    out = np.zeros(y.shape[:-1] + (len(idx),), dtype=np.int64)
    for i2, (j0, j1) in enumerate(idx):
        if j0 == 0:
            out[..., i2] = y[..., j1]
    return out


def embed_dec(m, m2, y, mod):
    y = np.asarray(y, dtype=np.int64)
    ents = lm.base_indices_dec(_pps(m), _pps(m2))
    out = np.zeros(y.shape[:-1] + (len(ents),), dtype=np.int64)
    for i2, ent in enumerate(ents):
        if ent is not None:
            out[..., i2] = (-y[..., ent[0]]) % mod if ent[1] else y[..., ent[0]]
    return out


@functools.lru_cache(maxsize=None)
def crtset(m, m2, p, e):
    """crtSet: strip the p-parts, crtSetDec, lift, Dec -> Pow, e - 1 p-th powers mod p^e, embedPow; a numpy [K][phi(m')]"""
    strip = lambda v: v // p ** next(k for k in itertools.count() if v % p ** (k + 1))
    mb, mb2, pe = strip(m), strip(m2), p ** e
    x = l_pow(_pps(mb2), np.array(crtset_dec(mb, mb2, p), dtype=np.int64), pe)
    R = ring(mb2)
    for _ in range(e - 1):
        y = x.copy()
        for _ in range(p - 1):
            y = np.stack([R.mul(yc, xc, pe) for yc, xc in zip(y, x)])
        x = y
    return embed_pow(mb2, m2, x)


def tunnel_funcs(rings, p, e):
    """per hop the first dim_h elements of crtSet(gcd(r_h, r_(h+1)), r_(h+1), p, e)"""
    out = []
    for r, s in zip(rings[:-1], rings[1:]):
        eh = math.gcd(r, s)
        dim = lm.totient_pps(_pps(r)) // (lm.totient_pps(_pps(eh)) if eh > 1 else 1)
        cs = crtset(eh, s, p, e)
        assert len(cs) >= dim
        out.append(cs[:dim])
    return out


def evallin(eh, r, s, r_dec, ys_pow, mod):
    """evalLin (Linear.hs:75-79) by schoolbook products: sum_i ys_i * embed(coeffsDec_i r), powerful basis of S mod `mod`"""
    r_dec = np.asarray(r_dec, dtype=np.int64) % mod
    idx = np.array(lm.ext_indices_coeffs(_pps(eh), _pps(r)), dtype=np.int64)        # [rel][n_E]
    R = ring(s)
    out = np.zeros((r_dec.shape[0], R.n), dtype=np.int64)
    for i in range(idx.shape[0]):
        c = l_pow(_pps(s), embed_dec(eh, s, r_dec[:, idx[i]], mod), mod)
        out = (out + c @ (R.mul_matrix(np.asarray(ys_pow[i]) % mod) % mod)) % mod
    return out


def pt_tunnel(rings, funcs, x_dec, mod):
    """ptTunnel: evalLin hop by hop; x_dec [B][n_R0] decoding basis -> [B][n_S_last] powerful basis"""
    x = np.asarray(x_dec, dtype=np.int64) % mod
    for h, (r, s) in enumerate(zip(rings[:-1], rings[1:])):
        y = evallin(math.gcd(r, s), r, s, x, funcs[h], mod)
        x = l_inv(_pps(s), y, mod)
    return y
