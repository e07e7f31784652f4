"""numpy restatement of L, L^-1, mulG and divG over Z, R and C and of mulC (lolhip_elt_op_batch, lolhip_mulc_batch;
DESIGN.md 3.4k): the recurrences of l.cpp:28-57, 67-98 and g.cpp:16-35, 37-58, 60-90, 92-123 under tensorFuserPrime
(tensor.h:39-74), run sequentially per (p-1)-vector in the reference's order of operations and vectorised only ACROSS
vectors, so every float64 value sees the same IEEE operations in the same order (numpy never contracts a multiply and an
add).  Integers are uint64 that wrap; divG over Z tests and divides the wrapped int64 values exactly with % and //, per
item; over R it divides by float(oddrad).

Slabs are [B][n][T]; complex128 is viewed as float64 with 2 T components (every map is real-linear and componentwise)."""
import numpy as np

OP_L, OP_LINV, OP_MULGPOW, OP_MULGDEC, OP_DIVGPOW, OP_DIVGDEC = 4, 5, 6, 7, 8, 9
OPS = (OP_L, OP_LINV, OP_MULGPOW, OP_MULGDEC, OP_DIVGPOW, OP_DIVGDEC)
OP_NAMES = {OP_L: "l", OP_LINV: "linv", OP_MULGPOW: "mulgpow", OP_MULGDEC: "mulgdec", OP_DIVGPOW: "divgpow",
            OP_DIVGDEC: "divgdec"}


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


def oddrad(pps):
    r = 1
    for p, _ in pps:
        if p != 2:
            r *= p
    return r


def _prime(op, v, p):
    """v [lts][p-1][rest], in place: one prime-index map on every vector v[:, :, j] at once"""
    E = v.dtype.type
    d = p - 1
    if op == OP_L:
        for i in range(1, d):
            v[:, i] = v[:, i] + v[:, i - 1]
    elif op == OP_LINV:
        for i in range(d - 1, 0, -1):
            v[:, i] = v[:, i] - v[:, i - 1]
    elif op == OP_MULGPOW:
        last = v[:, d - 1].copy()
        for i in range(d - 1, 0, -1):
            v[:, i] = v[:, i] + (last - v[:, i - 1])
        v[:, 0] = v[:, 0] + last
    elif op == OP_MULGDEC:
        acc = v[:, 0].copy()
        for i in range(d - 1, 0, -1):
            acc = acc + v[:, i]
            v[:, i] = v[:, i] - v[:, i - 1]
        v[:, 0] = v[:, 0] + acc
    elif op == OP_DIVGPOW:
        lelts = np.zeros_like(v[:, 0])
        for i in range(d):
            lelts = lelts + v[:, i]
        relts = np.zeros_like(lelts)
        for i in range(d - 1, -1, -1):
            z = v[:, i].copy()
            v[:, i] = E(p - 1 - i) * lelts - E(i + 1) * relts
            lelts = lelts - z
            relts = relts + z
    elif op == OP_DIVGDEC:
        acc = np.zeros_like(v[:, 0])
        for i in range(1, p):
            acc = acc + E(i) * v[:, i - 1]
        rp = E(p)
        for i in range(d - 1, 0, -1):
            tmp = acc.copy()
            acc = acc - v[:, i] * rp
            v[:, i] = tmp
        v[:, 0] = acc
    else:
        raise ValueError(op)


def transform(op, pps, y):
    """the prime-index part of `op` (no division) on words y [B][n][W], uint64 or float64; returns a new array"""
    y = np.array(y, copy=True)
    B, n, W = y.shape
    assert n == totient(pps)
    rts = 1
    with np.errstate(over="ignore"):
        for p, e in pps:
            dim = (p - 1) * p ** (e - 1)
            if p != 2:
                v = y.reshape(B * n // (rts * (p - 1)), p - 1, rts * W)
                _prime(op, v, p)
            rts *= dim
    return y


def _words(y, T):
    """(words [B][n][W], restore) of an int64 / float64 / complex128 slab [B][n][T]"""
    y = np.ascontiguousarray(y)
    B, n = y.shape[0], y.shape[1]
    if y.dtype == np.int64:
        return y.reshape(B, n, T).view(np.uint64), lambda w: w.view(np.int64).reshape(y.shape)
    if y.dtype == np.float64:
        return y.reshape(B, n, T), lambda w: w.reshape(y.shape)
    if y.dtype == np.complex128:
        return y.reshape(B, n, T).view(np.float64), lambda w: np.ascontiguousarray(w).view(np.complex128).reshape(y.shape)
    raise TypeError(y.dtype)


def elt_op(op, pps, y, T=1):
    """op on the slab y [B][n][T] (int64, float64 or complex128).  Returns the result, or (result, ok int32 [B]) for
    divG over int64: ok[b] = 1 and the exact quotients where every coefficient of item b's transform is divisible by
    oddrad, else ok[b] = 0 and the undivided transform."""
    w, restore = _words(y, T)
    out = transform(op, pps, w)
    if op not in (OP_DIVGPOW, OP_DIVGDEC):
        return restore(out)
    r = oddrad(pps)
    if out.dtype == np.float64:
        return restore(out / float(r))
    B = out.shape[0]
    ok = np.ones(B, dtype=np.int32)
    if r == 1:
        return restore(out), ok
    s = out.view(np.int64)
    div = ((s % r) == 0).reshape(B, -1).all(axis=1)     # numpy's int64 % and // are exact (floor) operations
    s[div] = s[div] // r
    ok[~div] = 0
    return restore(out), ok


def mulc(a, b):
    """a * b over complex128 as types.h:146-152: two rounded products and one rounded sum per part"""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    ar, ai, br, bi = a.real.copy(), a.imag.copy(), b.real.copy(), b.imag.copy()
    out = np.empty(a.shape, dtype=np.complex128)
    out.real = ar * br - ai * bi
    out.imag = ar * bi + ai * br
    return out


def wide_floats(rng, shape):
    """normals times 10^k, k uniform in -8 .. 8 per value: a contracted multiply-add or a reordered sum changes bits"""
    return rng.normal(size=shape) * 10.0 ** rng.integers(-8, 9, size=shape)
