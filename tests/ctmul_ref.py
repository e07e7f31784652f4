"""A CPU restatement of the SymmSHE ciphertext product (*) of any degree (instance Ring.C (CT ...), lol-apps
SymmSHE.hs:438-452) in the reference's own order, over the CPU oracle: toLSD of the first operand when both are MSD, crt
of every component, the polynomial product in Python integers, mulG in the CRT basis (the pointwise product with gCRT,
CPP.hs:230) on every coefficient, crtInv when asked.

A ciphertext is the dict of tests/public_ref.py: {"enc": "LSD" | "MSD", "k", "l", "c": [ncs][B][n'][T] int64}, powerful
basis unless "crt" is set.  Also: the rule of (enc, k, l) alone, the work-buffer layout of lolhip_ct_mul_batch, and a
replay of k_ct_mul's lazy accumulator in Python integers.
"""
import os
import re
from math import gcd, prod

import numpy as np

import public_ref as pr
from oracle import lolmath as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 8


def lazy_interval():
    """the reduction interval lol_amd/csrc/ctmul.h states (LOLHIP_CT_MUL_LAZY)"""
    text = open(os.path.join(ROOT, "lol_amd", "csrc", "ctmul.h")).read()
    return int(re.search(r"#define\s+LOLHIP_CT_MUL_LAZY\s+(\d+)", text).group(1))


def g_crt(P):
    """gCRT [n][T] as Python integers"""
    return np.stack([np.array(lm.g_crt(P.pps, q), dtype=object) for q in P.qs], axis=-1)


def rule(qs, p, enc1, k1, l1, enc2, k2, l2):
    """(alpha [T], enc, k, l) of ct1 * ct2 (SymmSHE.hs:444-452); ValueError where the reference has no inverse"""
    if p < 2:
        raise ValueError("p < 2")
    alpha = [1 % q for q in qs]
    l1, l2 = l1 % p, l2 % p
    if enc1 == "MSD" and enc2 == "MSD":                       # toLSD ct1 * ct2
        if gcd(prod(qs), p) != 1:
            raise ValueError("gcd(Q, p) != 1")
        alpha, zp = pr.encode_scales(qs, p, False)
        l1 = l1 * zp % p
    enc = "LSD" if enc1 == "LSD" and enc2 == "LSD" else "MSD"
    return alpha, enc, k1 + k2 + 1, l1 * l2 % p


def _crt_comps(cpu, P, ct):
    c = [np.ascontiguousarray(x) for x in ct["c"]]
    if not ct.get("crt"):
        c = [np.asarray(cpu.crt(P, x)).reshape(x.shape) for x in c]
    return [x.astype(object) for x in c]


def ct_mul(cpu, P, ct1, ct2, p, out_crt=False):
    """ct1 * ct2 -> {"enc", "k", "l", "c" [na + nb - 1][B][n'][T]} (and "crt" with out_crt)"""
    qs = P.qs
    _, enc, k, l = rule(qs, p, ct1["enc"], ct1["k"], ct1["l"], ct2["enc"], ct2["k"], ct2["l"])
    if ct1["enc"] == "MSD" and ct2["enc"] == "MSD":
        ct1 = pr.to_lsd(ct1, qs, p)                                   # scaling commutes with crt: either basis
    a, b = _crt_comps(cpu, P, ct1), _crt_comps(cpu, P, ct2)
    g, qv = g_crt(P), np.array(qs, dtype=object)
    out = []
    for kk in range(len(a) + len(b) - 1):
        acc = 0
        for i in range(len(a)):
            if 0 <= kk - i < len(b):
                acc = acc + a[i] * b[kk - i]
        out.append(((acc % qv) * g % qv).astype(np.int64))            # mulG <$> (c1 * c2)
    if not out_crt:
        out = [np.asarray(cpu.crtinv(P, np.ascontiguousarray(x))).reshape(x.shape) for x in out]
    res = {"enc": enc, "k": k, "l": l, "c": np.ascontiguousarray(np.stack(out))}
    if out_crt:
        res["crt"] = True
    return res


def work_len(n, T, na, nb, cs_crt, square, B):
    """lolhip_ct_mul_work_len restated: the operands' copies for the powerful-basis route, the square's once"""
    return 0 if cs_crt else (na + (0 if square else nb)) * B * n * T


def replay(q, na, nb, lazy, square=False):
    """k_ct_mul's accumulator schedule with every residue q - 1, in Python integers: the largest value any accumulator
    holds when it is reduced before a term arrives at an accumulator of `lazy` terms (the residue counts as one)"""
    v, peak = q - 1, 0
    for k in range(na + nb - 1):
        acc = cnt = 0
        if square:
            for i in range(na):
                j = k - i
                if j <= i or j >= na:
                    continue
                if cnt == lazy:
                    acc, cnt = acc % q, 1
                acc, cnt = acc + v * v, cnt + 1
                peak = max(peak, acc)
            diag = k % 2 == 0 and k // 2 < na
            acc = 2 * acc if 2 * cnt + diag <= lazy else 2 * (acc % q)     # the doubled sum counts as twice its terms
            if diag:
                acc += v * v
            peak = max(peak, acc)
        else:
            for i in range(na):
                if not 0 <= k - i < nb:
                    continue
                if cnt == lazy:
                    acc, cnt = acc % q, 1
                acc, cnt = acc + v * v, cnt + 1
                peak = max(peak, acc)
    return peak


def saturated(qs, alpha, g, na, nb):
    """the closed form for every residue q_t - 1: out_k = alpha_t g (pairs i + j = k) mod q_t, [na + nb - 1][n][T]"""
    qv = np.array(qs, dtype=object)
    al = np.array([int(x) for x in alpha], dtype=object)
    out = []
    for k in range(na + nb - 1):
        pairs = sum(1 for i in range(na) if 0 <= k - i < nb)            # (-1)(-1) = 1 per pair
        out.append((g * al * pairs % qv).astype(np.int64))
    return np.stack(out)
