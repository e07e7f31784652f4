"""Restatement of RLWE / RLWR instances over one modulus without a CRT basis (lolhip_rlwe_ring_*, include/lolhip.h) for
the tests: the exact ring product of tests/ringmul_ref.py, L and L^-1 over the integers from tests/eltops_ref.py (the
recurrences of l.cpp, checked against the CPU oracle in test_rlwe_ring_host.py), and tests/rlwe_ref.py / tests/enc_ref.py
for the streams, the roundings and RRq.  Also the classification of rlwe-challenges' parameter list by the project's own
rules.  Test infrastructure only."""
import os

import numpy as np

import eltops_ref as el
import ringmul_ref as rm
import rlwe_ref as rr
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "rlwe_challenge_params.txt")
DISC, CONT, RLWR = 0, 1, 2
KINDS = {"Disc": DISC, "Cont": CONT, "RLWR": RLWR}


# ---- the challenge list ---------------------------------------------------------------------------------------------------
def challenge_lines():
    """[(kind, m, q, v)]: v = the scaled variance (Cont, Disc) or the rounding modulus p (RLWR)"""
    out = []
    for ln in open(PARAMS):
        f = ln.split()
        if f:
            out.append((f[1], int(f[2]), int(f[3]), int(f[4]) if f[1] == "RLWR" else float(f[4])))
    return out


def is_prime(q):
    if q < 2:
        return False
    i = 2
    while i * i <= q:
        if q % i == 0:
            return False
        i += 1
    return True


def sampler_index_ok(m):
    """the sampler's limits (sampler_internal.h): a 2-power up to n = 16384, else every prime <= 13 and n <= 8192"""
    pps = rr.factor_pps(m)
    n = rr.totient(pps)
    if all(p == 2 for p, _ in pps):
        return n <= 16384
    return n <= 8192 and all(p <= 13 for p, _ in pps)


def classify(kind, m, q):
    """"plan": lolhip_rlwe_* serves the line;  "ring": only lolhip_rlwe_ring_* does;  "index": the sampler refuses m"""
    if kind != "RLWR" and not sampler_index_ok(m):
        return "index"
    return "plan" if is_prime(q) and q % m == 1 else "ring"


def ring_pairs():
    """the distinct (m, q) of the ring-route lines, in the list's order"""
    seen = []
    for kind, m, q, _ in challenge_lines():
        if classify(kind, m, q) == "ring" and (m, q) not in seen:
            seen.append((m, q))
    return seen


# ---- layouts ----------------------------------------------------------------------------------------------------------------
def even(x):
    return (x + 1) & ~1


def work_len(kind, B, n, K):
    """include/lolhip.h: the lifted a | the residues | (Disc, Cont) the Gaussians or the error"""
    return even(B * n * K) + even(B * n) + (0 if kind == RLWR else even(B * n))


# ---- arithmetic -------------------------------------------------------------------------------------------------------------
def _int_op(op, m, x):
    """L or L^-1 over the integers on x [B][n]: the recurrences of tests/eltops_ref.py on Python integers (sums and
    differences only, so an object array runs them exactly)"""
    x = np.asarray(x).astype(object)
    return el.transform(op, rr.factor_pps(m), x[..., None])[..., 0]


def l_mod(m, e, q):
    """l(e) mod q for integers e [B][n]"""
    return (_int_op(el.OP_L, m, e) % q).astype(np.int64)


def linv_mod(m, x, q):
    """lInv x mod q for integers x [B][n]"""
    return (_int_op(el.OP_LINV, m, x) % q).astype(np.int64)


def product(m, q, a_pow, s_pow):
    """a s in R_q, powerful basis: a [B][n], s [n] -> [B][n] in [0, q)"""
    a, s = np.asarray(a_pow), np.asarray(s_pow)
    if m & (m - 1) == 0:
        return np.stack([rm.mul_pow2(m, row, s, q) for row in a])
    sb = np.broadcast_to(s[None, :, None], a.shape + (1,))
    return rm.mul(m, a[..., None], sb, [q])[..., 0]


def x_dec(m, q, a_pow, s_pow):
    """the decoding-basis residues in [0, q) of a s"""
    return linv_mod(m, product(m, q, a_pow, s_pow), q)


def lift(r, q):
    """r -> r when 2 r < q, else r - q (RingMul's convention, the reference's lift)"""
    r = np.asarray(r).astype(object) % q
    return np.where(2 * r < q, r, r - q).astype(np.int64)


def disc_b(m, q, a_pow, s_pow, e):
    """b = (a s + l(e)) mod q, powerful basis"""
    return ((product(m, q, a_pow, s_pow).astype(object) + l_mod(m, e, q).astype(object)) % q).astype(np.int64)


def disc_error(m, q, a_pow, b, s_pow):
    d = (np.asarray(b).astype(object) - product(m, q, a_pow, s_pow).astype(object)) % q
    return lift(linv_mod(m, d.astype(np.int64), q), q)


def uniform(key, domain, ctr, B, n, q):
    return rr.uniform(key, domain, ctr, B, n, [q])[..., 0]


def rlwr_b(m, q, p, a_pow, s_pow):
    return rr.rlwr_round(x_dec(m, q, a_pow, s_pow), q, p)


def good_prime(m, lower):
    return next(lm.good_qs(m, lower))
