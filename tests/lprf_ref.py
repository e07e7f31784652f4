"""Restatement of the key-homomorphic lattice PRF (lol-apps KeyHomomorphicPRF.hs: buildSubtree of buildDecTree and
latticePRF', eq. 2.3 of [BP14]) in Python integers (object arrays): one input at a time, nothing shared between inputs.

Digits come from oracle.she_ref.decompose on a one-modulus parameter object (so the oracle and k_decompose are tied to one
digit convention), the rounding from she_ref.div_mod_cent / lift_centered.  Also the host restatements the tests need of
what lprf_api.cpp derives: the gadget length, max|digit|, both exactness certificates and the work layout.
"""
import types

import numpy as np

import khprf_cases as kc
from oracle import she_ref as sr


def one_mod(q):
    """what she_ref.decompose / gadget / digit_counts read of a parameter object: one modulus"""
    return types.SimpleNamespace(qs=[int(q)], T=1)


def ell_of(q, base):
    return sr.digit_counts(one_mod(q), base)[0]


def ginv(q, base, A):
    """G^-1(A) = fmap reduce (decomposeMatrix A) (Gadget.hs:76-81): A [n][K] -> [K][K] object array of residues in
    [0, q); row i ell + j of column c is digit j of entry (i, c)"""
    A = np.asarray(A, dtype=object)
    n, K = A.shape
    d = sr.decompose(one_mod(q), (A % q).astype(np.int64).reshape(1, n * K, 1), base)     # [ell][1][n K][1]
    ell = d.shape[0]
    assert n * ell == K, (n, ell, K)
    d = d.reshape(ell, n, K)
    return np.ascontiguousarray(d.transpose(1, 0, 2)).reshape(K, K).astype(object)


def eval_tree(q, base, tree, a0, a1, x):
    """A_T(x): buildSubtree x T (rbits = x & (2^c_r - 1), lbits = x >> c_r; val = lval * decompr), [n][K] object"""
    import khprf_ref as kr

    def sub(x, t):
        if t[0] == "L":
            return np.asarray(a1 if x else a0, dtype=object) % q
        _, _, lt, rt = t
        cr = kr.leaves(rt)
        lval = sub(x >> cr, lt)
        rval = sub(x & ((1 << cr) - 1), rt)
        return lval.dot(ginv(q, base, rval)) % q

    return sub(int(x), kr.parse(tree))


def rescale(z, q, p):
    """rescaleMod (ZqBasic.hs:130): fst (divModCent (p lift z) q) mod p"""
    quot, _ = sr.div_mod_cent(p * sr.lift_centered(z, q), q)
    return quot % p


def lattice_prf(q, base, tree, a0, a1, s, p, x):
    """latticePRF' s x = rescale <$> s * A_T(x): s [n] -> [K] object array in [0, p)"""
    A = eval_tree(q, base, tree, a0, a1, x)
    return rescale((np.asarray(s, dtype=object) % q).dot(A) % q, q, p)


def eval_window(q, base, tree, a0, a1, x0, B):
    """[B][n][K] int64"""
    n, K = np.asarray(a0).shape
    out = np.zeros((B, n, K), dtype=np.int64)
    for b in range(B):
        out[b] = eval_tree(q, base, tree, a0, a1, x0 + b).astype(np.int64)
    return out


def prf_window(q, base, tree, a0, a1, s, p, x0, B):
    """s [nkeys][n] -> [nkeys][B][K] int64"""
    s = np.asarray(s, dtype=object)
    K = np.asarray(a0).shape[1]
    out = np.zeros((s.shape[0], B, K), dtype=np.int64)
    for b in range(B):
        A = eval_tree(q, base, tree, a0, a1, x0 + b)
        for k in range(s.shape[0]):
            out[k, b] = rescale((s[k] % q).dot(A) % q, q, p).astype(np.int64)
    return out


# ---- what the host derives ----------------------------------------------------------------------------------------------
def max_digit(q, base):
    """max|digit| of the centred decomposition over every residue, from the range ends (the digit maps are monotone):
    remainders reach base div 2, the last digit is f^(ell-1) of the ends of the lift's range, f v = floor((v + b/2)/b)"""
    if base == 0:
        return q // 2
    lo, hi = -(q // 2), (q - 1) // 2
    for _ in range(ell_of(q, base) - 1):
        lo, hi = (lo + base // 2) // base, (hi + base // 2) // base
    return max(base // 2, abs(lo), abs(hi))


def brute_max_digit(q, base):
    """the same over all q residues through she_ref.decompose (small q)"""
    d = sr.decompose(one_mod(q), np.arange(q, dtype=np.int64).reshape(1, q, 1), base)
    return int(np.abs(sr.lift_centered(d.reshape(-1), q)).max())


def valu_fold(q, base):
    """terms per signed 64-bit lazy sum of the VALU route ((q-1) + fold (q-1) D <= 2^63 - 1); 0: 128-bit sums"""
    F = (2 ** 63 - 1 - (q - 1)) // ((q - 1) * max_digit(q, base))
    return 0 if F < 8 else min(F, 2 ** 30)


def mfma_limbs(q, base, K):
    """W of the matrix route, 0 where its certificate refuses: max|digit| <= 127 and K 128 max|digit| < 2^31"""
    D = max_digit(q, base)
    if D > 127 or K * 128 * D >= 2 ** 31:
        return 0
    W = 1
    while W < 8 and q - 1 > 127 * ((256 ** W - 1) // 255):
        W += 1
    return W


MFMA_MIN_K = 56                                                      # lprf_api.cpp: the measured crossover of the routes


def mfma_default(q, base, K):
    """W where the host rule takes the matrix route by default (admitted, and K at or above the crossover), else 0"""
    return mfma_limbs(q, base, K) if K >= MFMA_MIN_K else 0


def work_len(tree, n, K, nkeys, x0, B):
    """the header's formula: U_v n K per internal node below the root, U_l nkeys K for a keyed internal root"""
    if B == 0:
        return 0
    nodes = kc.parse(tree)
    tot = sum(kc.view(v, x0, B)[0] * n * K for i, v in enumerate(nodes) if i and not v.leaf)
    if nkeys > 0 and not nodes[0].leaf:
        tot += kc.view(nodes[nodes[0].l], x0, B)[0] * nkeys * K
    return tot
