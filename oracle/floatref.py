"""oracle/floatref.py — numpy restatement of the floating-point members of the Tensor class.
TEST INFRASTRUCTURE (only tests/ may import it).

  crt_c / crtinv_c   the closed form of SURVEY.md Appendix A evaluated over C with
                     omega_m = exp(2 pi i / m): what lol-cpp's tensorCRTC / tensorCRTInvC
                     (crt.cpp:583-598, ppcrt/ppcrtinv at Complex) compute, as a dense n x n matrix
                     (small n only: O(n^2))
  gaussian_dec       tensorGaussianDec (random.cpp:19-64): per odd prime p the real
                     (p-1) x (p-1) matrix of primeD applied along axis k
  *_ext              the same in x86-64 long double, one dense matrix per prime-power axis (any n up
                     to 8192); crtinv_c_residual is the backward error of a computed crtInvC

Pinned against lol-cpp itself (oracle/_ref, run here) and the committed fixtures in
tests/golden/golden_float.npz (tests/test_float.py).
"""
from __future__ import annotations

import numpy as np

from . import lolmath as lm


def _digits(pps):
    """phi_k and the mixed-radix digit tables of the tensor index (k = 1 fastest, tensor.h:46-73)."""
    phis = [(p - 1) * p ** (e - 1) for p, e in pps]
    n = int(np.prod(phis)) if phis else 1
    idx = np.arange(n)
    digs = []
    for ph in phis:
        digs.append(idx % ph)
        idx = idx // ph
    return phis, n, digs


def crt_matrix_c(pps, inverse=False):
    """M[i, j] = prod_k omega_{pp_k}^{pow_k(j_k) * zms_k(i_k)} (Tensor.hs:359-368; Appendix A)."""
    phis, n, digs = _digits(pps)
    M = np.ones((n, n), dtype=np.complex128)
    for (p, e), dig in zip(pps, digs):
        pp = p ** e
        zms = p * (dig // (p - 1)) + dig % (p - 1) + 1                       # units of Z_{p^e}, row index
        hi = dig // (p - 1)
        rev = np.array([lm.digit_rev(p, e - 1, int(h)) for h in hi])         # digit-reversed powerful basis, column index
        pw = p ** (e - 1) * (dig % (p - 1)) + rev
        ex = (zms[:, None] * pw[None, :]) % pp
        M *= np.exp(2j * np.pi * ex / pp)
    return np.linalg.inv(M) if inverse else M


def crt_c(pps, y):
    n = lm.totient_pps(pps)
    return np.asarray(y, dtype=np.complex128).reshape(-1, n) @ crt_matrix_c(pps).T


def crtinv_c(pps, y):
    n = lm.totient_pps(pps)
    return np.asarray(y, dtype=np.complex128).reshape(-1, n) @ crt_matrix_c(pps, inverse=True).T


def gaussian_dec(pps, y):
    """random.cpp:19-64: out[row] = (sum_col 2 c(row*col mod p) y[col-1]) / sqrt 2 on every
    (p-1)-vector of axis k; c = Re omega_p^k for col <= p/2, Im for col > p/2; identity for p = 2."""
    phis, n, _ = _digits(pps)
    y = np.asarray(y, dtype=np.float64).reshape(-1, n).copy()
    B = y.shape[0]
    rts = 1
    for (p, e), ph in zip(pps, phis):
        if p != 2:
            D = np.zeros((p - 1, p - 1))
            for row in range(p - 1):
                for col in range(1, p):
                    ang = 2.0 * np.pi * ((row * col) % p) / p
                    D[row, col - 1] = 2.0 * (np.cos(ang) if col <= p // 2 else np.sin(ang)) / np.sqrt(2.0)
            lts = n // (rts * (p - 1))
            v = y.reshape(B, lts, p - 1, rts)
            y = np.einsum("rc,blcs->blrs", D, v).reshape(B, n)
        rts *= ph
    return y


# ---- extended precision (x86-64 80-bit long double: 64-bit mantissa) --------------------------------
# The same closed forms, evaluated so that the oracle's own error (about 2^-64 per operation) sits three
# decimal digits below float64's: a kernel that loses a few digits is then measured, not masked.  Roots
# come from a long-double pi and exponents reduced exactly as integers mod pp; every axis is applied as one
# dense phi x phi matrix (never the kernel's factorisation into stages), in row chunks so that phi = 8192
# stays within a few hundred MB.

PI_EXT = 4 * np.arctan(np.longdouble(1))
_CHUNK = 256


def _roots_ext(pp, inverse=False):
    """omega_pp^(+-k), k < pp, as clongdouble."""
    ang = (2 * PI_EXT / np.longdouble(pp)) * np.arange(pp).astype(np.longdouble)
    r = np.empty(pp, dtype=np.clongdouble)
    r.real = np.cos(ang)
    r.imag = -np.sin(ang) if inverse else np.sin(ang)
    return r


def _axis_exponents(p, e, rows):
    """ex[i, j] = pw(j) * zms(i) mod p^e for output digits `rows` (Tensor.hs:359-368; crt_matrix_c)."""
    pp, phi = p ** e, (p - 1) * p ** (e - 1)
    i = np.asarray(rows, dtype=np.int64)
    zms = p * (i // (p - 1)) + i % (p - 1) + 1
    j = np.arange(phi, dtype=np.int64)
    rev = np.array([lm.digit_rev(p, e - 1, int(h)) for h in range(p ** (e - 1))], dtype=np.int64)
    pw = p ** (e - 1) * (j % (p - 1)) + rev[j // (p - 1)]
    return (zms[:, None] * pw[None, :]) % pp


def _apply_axes(pps, y, axis_op):
    """y [B][n] with axis k of length phi_k (k = 0 fastest): axis_op(k, v [phi_k][cols]) -> [phi_k][cols]."""
    phis, n, _ = _digits(pps)
    B = y.shape[0]
    rts = 1
    for k, ph in enumerate(phis):
        lts = n // (rts * ph)
        v = y.reshape(B, lts, ph, rts).transpose(2, 0, 1, 3).reshape(ph, -1)
        y = axis_op(k, v).reshape(ph, B, lts, rts).transpose(1, 2, 0, 3).reshape(B, n)
        rts *= ph
    return y


def crt_c_ext(pps, y):
    """crt_c in long double: y [B][n] (any complex dtype) -> clongdouble [B][n]."""
    n = lm.totient_pps(pps)
    y = np.asarray(y).astype(np.clongdouble).reshape(-1, n)

    def axis(k, v):
        p, e = pps[k]
        w = _roots_ext(p ** e)
        phi = v.shape[0]
        out = np.empty_like(v)
        for r0 in range(0, phi, _CHUNK):
            out[r0:r0 + _CHUNK] = w[_axis_exponents(p, e, range(r0, min(phi, r0 + _CHUNK)))] @ v
        return out

    return _apply_axes(pps, y, axis)


def crtinv_c_residual(pps, got, z):
    """Normwise backward error of a computed crtInvC, per row: ||M_ext got - z|| / ||z|| with M_ext the
    long-double forward map (numpy has no long-double solver; the forward map is the exact closed form)."""
    n = lm.totient_pps(pps)
    z = np.asarray(z).astype(np.clongdouble).reshape(-1, n)
    r = crt_c_ext(pps, got) - z
    return np.sqrt(np.sum(np.abs(r) ** 2, axis=1)) / np.sqrt(np.sum(np.abs(z) ** 2, axis=1))


def gaussian_dec_ext(pps, y):
    """gaussian_dec in long double: per odd prime p the (p-1) x (p-1) primeD matrix (random.cpp:19-64)."""
    n = lm.totient_pps(pps)
    y = np.asarray(y).astype(np.longdouble).reshape(-1, n)
    phis, _, _ = _digits(pps)
    B = y.shape[0]
    rts = 1
    s2 = np.sqrt(np.longdouble(2))
    for (p, e), ph in zip(pps, phis):
        if p != 2:
            row = np.arange(p - 1)[:, None]
            col = np.arange(1, p)[None, :]
            ang = (2 * PI_EXT / np.longdouble(p)) * ((row * col) % p).astype(np.longdouble)
            D = 2 * np.where(col <= p // 2, np.cos(ang), np.sin(ang)) / s2
            lts = n // (rts * (p - 1))
            v = y.reshape(B, lts, p - 1, rts).transpose(2, 0, 1, 3).reshape(p - 1, -1)
            y = (D @ v).reshape(p - 1, B, lts, rts).transpose(1, 2, 0, 3).reshape(B, n)
        rts *= ph
    return y


def rel_err(got, want):
    """Normwise relative error per row, in long double: ||got - want|| / ||want||."""
    want = np.asarray(want)
    n = want.shape[-1]
    w = want.reshape(-1, n)
    d = np.asarray(got).astype(w.dtype).reshape(-1, n) - w
    return np.sqrt(np.sum(np.abs(d) ** 2, axis=1)) / np.sqrt(np.sum(np.abs(w) ** 2, axis=1))
