"""A CPU restatement of the SymmSHE public operations and ciphertext addition (lol-apps SymmSHE.hs:214-230, 381-436;
ZqBasic.hs:92-94, 132-137) in the reference's own order, over the CPU oracle: gpow on a mod-p Params, decode', embed_pow,
then crt at m'.  The device folds the embedding into a gather after a crt at index m; following the reference's order
here makes bit-exact parity check that shortcut as well.

A ciphertext is a dict {"enc": "LSD" | "MSD", "k", "l", "c": [ncs][B][n'][T] int64}, powerful basis unless "crt" is set.
"""
from math import prod

import numpy as np

from oracle import lolmath as lm
from oracle.oracle import Params


def params(m, qs):
    """oracle Params, also for a modulus without a CRT basis (prime ops only, as tests/test_decrypt.py does)"""
    try:
        return Params(lm.factor_pps(m), qs)
    except ValueError:
        P = Params.__new__(Params)
        P.pps = lm.factor_pps(m)
        P.qs, P.T, P.m, P.n = list(qs), len(qs), m, lm.totient_pps(P.pps)
        return P


def decode(v, p):
    """decode' (ZqBasic.hs:92-94) elementwise: v mod p lifted to v if 2v < p, else v - p (object array)"""
    v = np.asarray(v).astype(object) % p
    return np.where(2 * v < p, v, v - p)


def reduce(x, qs):
    """integers [...] -> residues [...][T]"""
    x = np.asarray(x).astype(object)
    return np.ascontiguousarray(np.stack([(x % q).astype(np.int64) for q in qs], axis=-1))


def encode_scales(qs, p, to_msd):
    """lsdToMSD = ([p^-1 mod q_t], -Q mod p); msdToLSD = ([p mod q_t], (-Q)^-1 mod p) (Prelude.hs:310-315)"""
    Q = prod(qs)
    if to_msd:
        return [pow(p % q, -1, q) for q in qs], (-Q) % p
    return [p % q for q in qs], pow((-Q) % p, -1, p)


def lincomb(qs, a, alpha, b=None, beta=None):
    """out_i = alpha_t a_i + beta_t b_i, a missing component counting as zero"""
    na, nb = len(a), (0 if b is None else len(b))
    out = []
    for i in range(max(na, nb)):
        acc = 0
        if i < na:
            acc = acc + np.asarray(a[i]).astype(object) * np.array([int(x) for x in alpha], dtype=object)
        if i < nb:
            acc = acc + np.asarray(b[i]).astype(object) * np.array([int(x) for x in beta], dtype=object)
        out.append((acc % np.array(qs, dtype=object)).astype(np.int64))
    return np.ascontiguousarray(np.stack(out))


def to_msd(ct, qs, p):
    if ct["enc"] == "MSD":
        return ct
    zq, zp = encode_scales(qs, p, True)
    return dict(ct, enc="MSD", l=ct["l"] * zp % p, c=lincomb(qs, ct["c"], zq))


def to_lsd(ct, qs, p):
    if ct["enc"] == "LSD":
        return ct
    zq, zp = encode_scales(qs, p, False)
    return dict(ct, enc="LSD", l=ct["l"] * zp % p, c=lincomb(qs, ct["c"], zq))


def mul_scalar(ct, qs, a, p):
    v = int(decode(a, p))
    return dict(ct, c=lincomb(qs, ct["c"], [v] * len(qs)))


def negate(ct, qs):
    return dict(ct, c=lincomb(qs, ct["c"], [-1] * len(qs)))


def mul_gct(cpu, P_hi, ct):
    """mulGCT (SymmSHE.hs:413-416): mulG on every component (gpow, or the pointwise gCRT product in the CRT basis)"""
    f = (lambda y: cpu.crt(P_hi, cpu.gpow(P_hi, cpu.crtinv(P_hi, y)))) if ct.get("crt") else (lambda y: cpu.gpow(P_hi, y))
    c = np.stack([np.asarray(f(np.ascontiguousarray(x))).reshape(np.shape(x)) for x in ct["c"]])
    return dict(ct, k=ct["k"] + 1, c=np.ascontiguousarray(c))


def ct_add(cpu, P_hi, ct1, ct2, p):
    """(+) with the reference's alignment (SymmSHE.hs:420-436), recursively until l, k and enc agree"""
    qs = P_hi.qs
    while True:
        l1, l2 = ct1["l"] % p, ct2["l"] % p
        if l1 != l2:
            ct1 = dict(mul_scalar(ct1, qs, l1 * pow(l2, -1, p) % p, p), l=l2)
        elif ct1["k"] < ct2["k"]:
            ct1 = mul_gct(cpu, P_hi, ct1)
        elif ct1["k"] > ct2["k"]:
            ct2 = mul_gct(cpu, P_hi, ct2)
        elif ct1["enc"] != ct2["enc"]:
            if ct1["enc"] == "LSD":
                ct1 = to_msd(ct1, qs, p)
            else:
                ct2 = to_msd(ct2, qs, p)
        else:
            break
    return dict(ct1, c=lincomb(qs, ct1["c"], [1] * len(qs), ct2["c"], [1] * len(qs)))


def mod_switch_pt(ct, qs, p, p2):
    ct = to_msd(ct, qs, p)
    return dict(ct, l=int(decode(ct["l"], p)) % p2)


def _embedded(cpu, P_lo, P_hi, v_int, crt):
    """decode'd integers [Bv][n_m] -> reduced into the q_t, embedded into R'_{m'} (embed_pow), crt at m' if asked"""
    x = reduce(v_int, P_hi.qs)                                      # [Bv][n_m][T]
    if P_lo is not None:
        x = np.asarray(cpu.embed_pow(P_lo, P_hi, x)).reshape(x.shape[0], P_hi.n, P_hi.T)
    if crt:
        x = np.asarray(cpu.crt(P_hi, x)).reshape(x.shape[0], P_hi.n, P_hi.T)
    return x


def add_public(cpu, P_hi, P_lo, b, ct, p, B):
    """addPublic b (SymmSHE.hs:381-390).  b [Bv][n_m] (Bv = 1 or B), any int64; ct["c"] [ncs][Bc][n'][T] (Bc = 1 or B)"""
    qs = P_hi.qs
    ct = to_lsd(ct, qs, p)
    n_m = P_hi.n if P_lo is None else P_lo.n
    m = P_hi.m if P_lo is None else P_lo.m
    v = (np.asarray(b).astype(object) % p).reshape(-1, n_m)
    if ct["k"] > 0:
        Pp = params(m, [p])
        x = np.ascontiguousarray((v % p).astype(np.int64)[..., None])
        for _ in range(ct["k"]):
            x = np.asarray(cpu.gpow(Pp, x)).reshape(x.shape)            # mulGPow of index m, mod p
        v = x[..., 0].astype(object)
    v = v * pow(ct["l"], -1, p) % p
    a = _embedded(cpu, P_lo, P_hi, decode(v, p), ct.get("crt", False))
    c = np.asarray(ct["c"]).astype(object)
    c = np.broadcast_to(c, (c.shape[0], B) + c.shape[2:]).copy()
    c[0] = (c[0] + np.broadcast_to(a.astype(object), c[0].shape)) % np.array(qs, dtype=object)
    return dict(ct, c=np.ascontiguousarray((c % np.array(qs, dtype=object)).astype(np.int64)))


def mul_public(cpu, P_hi, P_lo, a, ct, p, B):
    """mulPublic a (SymmSHE.hs:405-411), CRT basis in and out"""
    qs = P_hi.qs
    n_m = P_hi.n if P_lo is None else P_lo.n
    x = _embedded(cpu, P_lo, P_hi, decode(np.asarray(a).reshape(-1, n_m), p), True).astype(object)
    c = np.asarray(ct["c"]).astype(object)
    c = np.broadcast_to(c, (c.shape[0], B) + c.shape[2:])
    out = (c * np.broadcast_to(x, c.shape[1:])[None]) % np.array(qs, dtype=object)
    return dict(ct, c=np.ascontiguousarray(out.astype(np.int64)))


def absorb_g(cpu, P_hi, ct, p):
    """absorbGFactors (SymmSHE.hs:464-473): d = divG^k 1 in R_{m'} mod p, every c_i times decode'(d); CRT basis"""
    if ct["k"] == 0:
        return ct
    Pp = params(P_hi.m, [p])
    d = np.zeros((1, P_hi.n, 1), dtype=np.int64)
    d[0, 0, 0] = 1
    for _ in range(ct["k"]):
        d = cpu.ginvpow(Pp, d)
        assert d is not None, "divG mod p"
        d = np.asarray(d).reshape(1, P_hi.n, 1)
    B = np.asarray(ct["c"]).shape[1]
    return dict(mul_public(cpu, P_hi, None, d[..., 0], ct, p, B), k=0)


def negacyclic(a, b, p):
    """a * b mod p in R_m, m = 2^e, powerful-basis vectors [n]: coefficient j is that of zeta^(bit reversal of j over
    e - 1 bits) (tests/khprf_lifted_ref.py), and zeta^n = -1"""
    n = len(a)
    bits = n.bit_length() - 1
    ex = np.array([int(format(j, f"0{bits}b")[::-1], 2) if bits else 0 for j in range(n)], dtype=np.int64)
    ea, eb = np.zeros(n, dtype=object), np.zeros(n, dtype=object)
    ea[ex] = np.asarray(a, dtype=object)
    eb[ex] = np.asarray(b, dtype=object)
    full = np.convolve(ea, eb)
    out = full[:n].copy()
    out[: n - 1] -= full[n:]
    return out[ex] % p
