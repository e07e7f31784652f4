"""Numpy restatement of the SymmSHE samplers of include/lolhip.h (encrypt / errorRounded) for the tests: the ChaCha20
block function (RFC 8439 §2.3), the stream layout, basic Box-Muller, the uniform CRT-basis residues and coset rounding
(roundCoset, lol Prelude.hs:156-161, half to even).  Test infrastructure only."""
import math

import numpy as np

SIGMA_C = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
DOM_ENC_GAUSS, DOM_UNIFORM, DOM_ERR_ROUNDED = 0, 1, 2
TWO_PI = 6.283185307179586


def key_words(key):
    return [int.from_bytes(bytes(key)[4 * i:4 * i + 4], "little") for i in range(8)]


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def chacha20_blocks(key, counter, n0, n1, n2):
    """blocks [N][16] uint32 for arrays (or scalars) of counter and nonce words, one key"""
    counter, n0, n1, n2 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64).astype(np.uint32) for v in (counter, n0, n1, n2)])
    N = counter.size
    kw = key_words(key)
    init = [np.full(N, c, dtype=np.uint32) for c in SIGMA_C] + [np.full(N, k, dtype=np.uint32) for k in kw] + \
        [counter.ravel().copy(), n0.ravel().copy(), n1.ravel().copy(), n2.ravel().copy()]
    x = [v.copy() for v in init]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 16)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 12)
        x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 8)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        out = [x[i] + init[i] for i in range(16)]
    return np.stack(out, axis=-1)


def stream(key, domain, ctr, B, nblk):
    """[B][nblk][16]: the blocks of items ctr .. ctr+B-1 of one domain"""
    item = (np.uint64(ctr) + np.arange(B, dtype=np.uint64))[:, None]
    blk = np.arange(nblk, dtype=np.uint64)[None, :]
    item, blk = np.broadcast_arrays(item, blk)
    w = chacha20_blocks(key, blk.ravel(), domain, item.ravel() & np.uint64(0xFFFFFFFF), item.ravel() >> np.uint64(32))
    return w.reshape(B, nblk, 16)


def mrad(pps):
    """m / rad m as a float, as the library computes it"""
    r = 1.0
    for p, e in pps:
        for _ in range(1, e):
            r *= p
    return r


def sigma(pps, v):
    return math.sqrt(v * mrad(pps) / TWO_PI)


def gaussians(key, domain, ctr, B, n, sig):
    """[B][n] float64: pair i from block i >> 2, words 4(i&3) .. 4(i&3)+3, basic Box-Muller"""
    npairs = (n + 1) // 2
    w = stream(key, domain, ctr, B, (npairs + 3) // 4).reshape(B, -1, 4, 4).reshape(B, -1, 4)[:, :npairs].astype(np.uint64)
    a = w[..., 0] | (w[..., 1] << np.uint64(32))
    c = w[..., 2] | (w[..., 3] << np.uint64(32))
    u1 = ((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (c >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r = sig * np.sqrt(-2.0 * np.log(u1))
    th = TWO_PI * u2
    g = np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).reshape(B, 2 * npairs)
    return np.ascontiguousarray(g[:, :n])


def uniform_crt(key, ctr, B, n, qs):
    """[B][n][T] int64: residue r = j*T + t from block r >> 2, (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q_t"""
    T = len(qs)
    nT = n * T
    w = stream(key, DOM_UNIFORM, ctr, B, (nT + 3) // 4).reshape(B, -1, 4).reshape(B, -1, 4)[:, :nT].astype(object)
    v = w[..., 0] + (w[..., 1] << 32) + (w[..., 2] << 64) + (w[..., 3] << 96)
    qv = np.array([qs[r % T] for r in range(nT)], dtype=object)
    return (v % qv).astype(np.int64).reshape(B, n, T)


def centred(x, p):
    x = np.asarray(x, dtype=np.int64) % p
    return np.where(2 * x < p, x, x - p)


def round_coset(g, rep, p):
    """(e, near_tie): e = rep + p rint((g - rep) / p), half to even; near_tie where (g - rep) / p is within 1e-9 of a
    half-integer (where ulp differences of libm can move the result)"""
    rep = np.asarray(rep, dtype=np.int64)
    y = (g - rep.astype(np.float64)) / float(p)
    e = rep + p * np.rint(y).astype(np.int64)
    near = np.abs(np.abs(y - np.floor(y)) - 0.5) < 1e-9
    return e, near
