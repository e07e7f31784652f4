"""lol_amd/wire.py — Lol's protocol-buffer messages (lol/Lol.proto, lol-apps SHE.proto and HomomPRF.proto) to and
from numpy arrays, through the library's host-side readers and writers (csrc/wire.cpp).  No device code."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import _i64p, _len, _u8p
from .tensor import lib


def _raw(data: bytes):
    return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")


def _two_pass(fn, *args) -> bytes:
    """size query (out = NULL), then the write"""
    need = _len(fn(*args, None, 0))
    buf = (C.c_uint8 * max(need, 1))()
    return bytes(buf[:_len(fn(*args, buf, need))])


def _byte_parts(parts):
    """list of bytes objects -> (array of pointers, array of lengths, keep-alive list)"""
    keep = [_raw(p) for p in parts]
    ptrs = (_u8p * max(len(parts), 1))(*[C.cast(k, _u8p) for k in keep])
    lens = np.array([len(p) for p in parts] or [0], dtype=np.int64)
    return ptrs, lens, keep


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(_i64p)


def rqproduct_write(m: int, qs, xs) -> bytes:
    """Serialise decoding-basis residues xs [n][T] as a Lol `RqProduct` message (lol/Lol.proto;
    IZipVector.hs:127-205): one Rq per modulus, centred lifts, unpacked sint64."""
    (xs, xp), (qa, qp) = _i64(xs), _i64(qs)
    T = len(qa)
    return _two_pass(lib().lolhip_rqproduct_write, m, qp, T, xp, xs.size // max(T, 1))


def rqproduct_read(data: bytes):
    """Parse a Lol `RqProduct` message -> (m, [q_t], xs [n][T]) with canonical residues."""
    m, T = C.c_uint32(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    args = (_raw(data), len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T))
    n = _len(lib().lolhip_rqproduct_read(*args, None, 0))
    xs = np.zeros((n, T.value), dtype=np.int64)
    _len(lib().lolhip_rqproduct_read(*args, xs.ctypes.data_as(_i64p), xs.size))
    return int(m.value), [int(q) for q in qs[:T.value]], xs


def kshint_read(data: bytes):
    """Parse a SymmSHE `KSHint` message (lol-apps/SHE.proto) -> (m, [q_t], xs [L][K][n][T]),
    decoding basis; `plan.crt(plan.l(xs.reshape(L*K, n, T)))` is the hint slab of keySwitch."""
    m, T, Lh, K = C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    args = (_raw(data), len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T), C.byref(Lh), C.byref(K))
    n = _len(lib().lolhip_kshint_read(*args, None, 0))
    xs = np.zeros((Lh.value, K.value, n, T.value), dtype=np.int64)
    _len(lib().lolhip_kshint_read(*args, xs.ctypes.data_as(_i64p), xs.size))
    return int(m.value), [int(q) for q in qs[:T.value]], xs


def r_read(data: bytes):
    """Lol.proto `R` -> (m, xs[n]) integer decoding-basis coefficients."""
    raw, m = _raw(data), C.c_uint32(0)
    n = _len(lib().lolhip_r_read(raw, len(data), C.byref(m), None, 0))
    xs = np.zeros(n, dtype=np.int64)
    _len(lib().lolhip_r_read(raw, len(data), C.byref(m), xs.ctypes.data_as(_i64p), n))
    return int(m.value), xs


def secretkey_read(data: bytes):
    """SHE.proto `SecretKey` -> (m, scaled variance v, sk[n])."""
    raw, m, v = _raw(data), C.c_uint32(0), C.c_double(0)
    n = _len(lib().lolhip_secretkey_read(raw, len(data), C.byref(m), C.byref(v), None, 0))
    xs = np.zeros(n, dtype=np.int64)
    _len(lib().lolhip_secretkey_read(raw, len(data), C.byref(m), C.byref(v), xs.ctypes.data_as(_i64p), n))
    return int(m.value), float(v.value), xs


def kqproduct_read(data: bytes):
    """Lol.proto `KqProduct` -> (m, [q_t], xs [n][T] float64)."""
    m, T = C.c_uint32(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    args = (_raw(data), len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T))
    n = _len(lib().lolhip_kqproduct_read(*args, None, 0))
    xs = np.zeros((n, T.value), dtype=np.float64)
    _len(lib().lolhip_kqproduct_read(*args, xs.ctypes.data_as(C.POINTER(C.c_double)), xs.size))
    return int(m.value), [int(q) for q in qs[:T.value]], xs


def linearrq_read(data: bytes):
    """Lol.proto `LinearRq` -> (e, r, m_out, [q_t], xs [C][n][T]) decoding basis, canonical residues."""
    e, r, m, Cn, T = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    args = (_raw(data), len(data), C.byref(e), C.byref(r), C.byref(Cn), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T))
    n = _len(lib().lolhip_linearrq_read(*args, None, 0))
    xs = np.zeros((Cn.value, n, T.value), dtype=np.int64)
    _len(lib().lolhip_linearrq_read(*args, xs.ctypes.data_as(_i64p), xs.size))
    return int(e.value), int(r.value), int(m.value), [int(q) for q in qs[:T.value]], xs


def kshint_write(m: int, qs, xs, gad=(0, 0)) -> bytes:
    """xs [L][K][n][T] decoding-basis residues -> SHE.proto `KSHint` bytes (gad = TypeRep words)."""
    (xs, xp), (_, qp) = _i64(xs), _i64(qs)
    Lh, K, n, T = xs.shape
    return _two_pass(lib().lolhip_kshint_write, m, qp, T, Lh, K, xp, n, int(gad[0]), int(gad[1]))


def tunnelhint_read(data: bytes):
    """SHE.proto `TunnelHint` -> dict(e, r, s, p, func = linearrq_read(...), hints = [kshint_read(...)])."""
    e, r, s, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    fo, fl = C.c_int64(0), C.c_int64(0)
    args = (_raw(data), len(data), C.byref(e), C.byref(r), C.byref(s), C.byref(p), C.byref(fo), C.byref(fl))
    nh = _len(lib().lolhip_tunnelhint_read(*args, None, None, 0))
    ho, hl = np.zeros(max(nh, 1), dtype=np.int64), np.zeros(max(nh, 1), dtype=np.int64)
    _len(lib().lolhip_tunnelhint_read(*args, ho.ctypes.data_as(_i64p), hl.ctypes.data_as(_i64p), nh))
    return {"e": int(e.value), "r": int(r.value), "s": int(s.value), "p": int(p.value),
            "func": linearrq_read(data[fo.value: fo.value + fl.value]),
            "hints": [kshint_read(data[int(o): int(o) + int(l)]) for o, l in zip(ho[:nh], hl[:nh])]}


def r_write(m: int, xs) -> bytes:
    """integer decoding-basis coefficients xs [n] -> Lol.proto `R` bytes."""
    xs, xp = _i64(xs)
    return _two_pass(lib().lolhip_r_write, m, xp, xs.size)


def secretkey_write(m: int, v: float, xs) -> bytes:
    """SHE.proto `SecretKey` (ring element xs [n] as `R`, scaled variance v)."""
    xs, xp = _i64(xs)
    return _two_pass(lib().lolhip_secretkey_write, m, C.c_double(v), xp, xs.size)


def linearrq_write(e: int, r: int, m: int, qs, xs) -> bytes:
    """xs [C][n][T] (values of an E-linear function on the relative decoding basis) -> Lol.proto `LinearRq` bytes."""
    (xs, xp), (_, qp) = _i64(xs), _i64(qs)
    Cn, n, T = xs.shape
    return _two_pass(lib().lolhip_linearrq_write, e, r, m, qp, T, Cn, xp, n)


def tunnelhint_write(func: bytes, hints, e: int, r: int, s: int, p: int) -> bytes:
    """SHE.proto `TunnelHint` from an encoded LinearRq and a list of encoded KSHints."""
    ptrs, lens, keep = _byte_parts(list(hints))
    return _two_pass(lib().lolhip_tunnelhint_write, _raw(func), len(func), ptrs, lens.ctypes.data_as(_i64p), len(hints), e, r, s, p)


def chain_write(elems) -> bytes:
    """HomomPRF.proto chain (LinearFuncChain / TunnelHintChain / RoundHintChain) of encoded elements."""
    ptrs, lens, keep = _byte_parts(list(elems))
    return _two_pass(lib().lolhip_chain_write, ptrs, lens.ctypes.data_as(_i64p), len(elems))


def chain_read(data: bytes):
    """HomomPRF.proto chain -> list of the encoded elements (hand them to linearrq_read / tunnelhint_read / kshint_read)."""
    raw = _raw(data)
    cnt = _len(lib().lolhip_chain_read(raw, len(data), None, None, 0))
    off, ln = np.zeros(max(cnt, 1), dtype=np.int64), np.zeros(max(cnt, 1), dtype=np.int64)
    _len(lib().lolhip_chain_read(raw, len(data), off.ctypes.data_as(_i64p), ln.ctypes.data_as(_i64p), cnt))
    return [data[int(o): int(o) + int(l)] for o, l in zip(off[:cnt], ln[:cnt])]
