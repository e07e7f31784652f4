"""Numpy restatement of the key-switch hint samplers of include/lolhip.h (lolhip_kshint_batch) for the tests: row j of
batch item b is LWE sample ctr + b L + j, its rounded Gaussians from domain 3 and its c1 from domain 4 of the ChaCha20
stream of tests/enc_ref.py.  Test infrastructure only."""
import numpy as np

import enc_ref as er
from oracle import floatref as fr

DOM_HINT_GAUSS, DOM_HINT_UNIFORM = 3, 4


def two_power(pps):
    return all(p == 2 for p, _ in pps)


def uniform_crt(key, domain, ctr, rows, n, qs):
    """[rows][n][T]: residue r = c*T + t of item ctr + row from block r >> 2, (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q_t"""
    T = len(qs)
    nT = n * T
    w = er.stream(key, domain, ctr, rows, (nT + 3) // 4).reshape(rows, -1, 4)[:, :nT].astype(object)
    v = w[..., 0] + (w[..., 1] << 32) + (w[..., 2] << 64) + (w[..., 3] << 96)
    qv = np.array([qs[r % T] for r in range(nT)], dtype=object)
    return (v % qv).astype(np.int64).reshape(rows, n, T)


def rounded_gaussians(key, ctr, rows, pps, n, svar):
    """(e [rows][n] int64, near_tie): errorRounded svar of items ctr .. ctr + rows - 1 of domain 3, decoding basis"""
    g = er.gaussians(key, DOM_HINT_GAUSS, ctr, rows, n, er.sigma(pps, svar))
    if not two_power(pps):
        g = fr.gaussian_dec(pps, g).reshape(rows, n)
    return er.round_coset(g, np.zeros((rows, n), dtype=np.int64), 1)
