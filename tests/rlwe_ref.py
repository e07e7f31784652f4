"""Numpy / Python-integer restatement of the RLWE section of include/lolhip.h for the tests: gSqNormDec (norm.cpp:15-75
under tensorFuserPrime, tensor.h:40-80), the sampler streams of domains 5-7, the K/(qR) arithmetic of RRq.hs:47-84, the
RLWR rounding (RLWR.hs:34-44) and the error bounds (Continuous.hs:74-84, Discrete.hs:65-76).  Test infrastructure only."""
import math

import numpy as np

import enc_ref as er

DOM_RLWE_UNIFORM, DOM_RLWE_GAUSS, DOM_RLWE_SECRET = 5, 6, 7
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63


def factor_pps(m):
    out, p = [], 2
    while m > 1:
        if m % p == 0:
            e = 0
            while m % p == 0:
                m //= p
                e += 1
            out.append((p, e))
        p += 1
    return out


def totient(pps):
    n = 1
    for p, e in pps:
        n *= (p - 1) * p ** (e - 1)
    return n


# ---- gSqNormDec -------------------------------------------------------------------------------------------------------
def norm_operator(pps, e):
    """y = (⊗ I_{p^(e-1)} ⊗ (I+J)_{p-1}) e for e [B][n] (any dtype, object included), the first prime power of pps
    fastest-varying and, inside a prime power, the p - 1 coordinate fastest"""
    e = np.asarray(e)
    B, n = e.shape
    dims = [(p - 1) * p ** (x - 1) for p, x in pps]
    y = e.reshape([B] + dims[::-1]).copy()
    for i, (p, x) in enumerate(pps):
        if p == 2:
            continue
        ax = len(dims) - i                                    # the axis of prime power i (axis 0 is the batch)
        sh = list(y.shape)
        z = y.reshape(sh[:ax] + [p ** (x - 1), p - 1] + sh[ax + 1:])
        z = z + z.sum(axis=ax + 1, keepdims=True)
        y = z.reshape(sh)
    return y.reshape(B, n)


def gsqnorm_int(pps, e):
    """exact values as Python integers, [B]"""
    eo = np.asarray(e).astype(object)
    return [int(v) for v in (eo * norm_operator(pps, eo)).sum(axis=1)]


def gsqnorm_sat(pps, e):
    """the int64 contract: min(value, INT64_MAX), and INT64_MAX where a coefficient is INT64_MIN; int64 [B]"""
    e = np.asarray(e, dtype=np.int64)
    marked = (e == INT64_MIN).any(axis=1)
    return np.array([INT64_MAX if mk else min(v, INT64_MAX) for v, mk in zip(gsqnorm_int(pps, e), marked)], dtype=np.int64)


def gsqnorm_f64(pps, e):
    e = np.asarray(e, dtype=np.float64)
    return (e * norm_operator(pps, e)).sum(axis=1)


# ---- sampler streams ----------------------------------------------------------------------------------------------------
def uniform(key, domain, ctr, B, n, qs):
    """[B][n][T] int64: residue r = j*T + t from block r >> 2 of item ctr + b, as one 128-bit integer mod q_t"""
    T = len(qs)
    nT = n * T
    w = er.stream(key, domain, ctr, B, (nT + 3) // 4).reshape(B, -1, 4)[:, :nT].astype(object)
    v = w[..., 0] + (w[..., 1] << 32) + (w[..., 2] << 64) + (w[..., 3] << 96)
    qv = np.array([qs[r % T] for r in range(nT)], dtype=object)
    return (v % qv).astype(np.int64).reshape(B, n, T)


def gaussian_dec(pps, key, ctr, B, svar):
    """tGaussianDec svar of items ctr .. ctr + B - 1 of domain 6, unrounded, float64 [B][n]"""
    from oracle import floatref as fr
    n = totient(pps)
    g = er.gaussians(key, DOM_RLWE_GAUSS, ctr, B, n, er.sigma(pps, svar))
    if any(p != 2 for p, _ in pps):
        g = np.asarray(fr.gaussian_dec(pps, g), dtype=np.float64).reshape(B, n)
    return g


# ---- K/(qR) (RRq.hs:47-84): IEEE doubles, these operations in this order ----------------------------------------------------
def rrq_reduce(x, q):
    x = np.asarray(x, dtype=np.float64)
    return x - q * np.floor(x / q)


def rrq_add(x, y, q):
    z = x + y
    return np.where(z >= q, z - q, z)


def cont_sample(x, g, q):
    """b from the residues x of a s in [0, q) and the Gaussians g"""
    q = float(q)
    return rrq_add(np.asarray(x, dtype=np.int64).astype(np.float64), rrq_reduce(g, q), q)


def cont_error(x, b, q):
    """lift (b - x)"""
    q = float(q)
    y = rrq_add(np.asarray(b, dtype=np.float64), rrq_reduce(-np.asarray(x, dtype=np.int64).astype(np.float64), q), q)
    return np.where(y + y < q, y, y - q)


# ---- RLWR -----------------------------------------------------------------------------------------------------------------
def rlwr_round(x, q, p):
    """per residue x in [0, q): l = 2x < q ? x : x - q, floor((p l + floor(q/2)) / q) mod p, Python integers"""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype=np.int64)
    flat, of = x.reshape(-1), out.reshape(-1)
    for i, v in enumerate(flat):
        v = int(v)
        l = v if 2 * v < q else v - q
        of[i] = ((p * l + q // 2) // q) % p
    return out


# ---- error bounds -----------------------------------------------------------------------------------------------------------
def _stabilize(c):
    x = 1 / (2 * math.pi)
    while True:
        x1 = (1 / 2 + math.log(2 * math.pi * x) / 2 - c) / math.pi
        if x1 - x < 0.0001:
            return x1
        x = x1


def error_bound_cont(m, svar, eps):
    pps = factor_pps(m)
    n = totient(pps)
    mhat = m // 2 if m % 2 == 0 else m
    return mhat * n * svar * _stabilize(math.log(eps) / n)


def error_bound_disc(m, svar, eps):
    pps = factor_pps(m)
    n = totient(pps)
    odd = sum(1 for p, _ in pps if p != 2)
    return math.ceil((2 ** odd) * n * _stabilize(math.log(eps)) + error_bound_cont(m, svar, eps))
