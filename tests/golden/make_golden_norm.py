"""Generator of tests/golden/golden_norm.npz: inputs and outputs of the reference's own gSqNormDec, tensorNormSqR /
tensorNormSqD (tupSize = 1), called through ctypes on oracle/_ref/libctensor.so (built by `make -C oracle ref`).

Per index m: e_i_<m> int32 [B][n] (|e| < 2^20), n_i_<m> int64 [B]; e_d_<m> float32 [B][n], n_d_<m> float64 [B].  The
inputs are stored narrow to keep the file small: the int64 / float64 inputs of the calls are exactly their widenings
(the doubles carry 16 significant bits).  B = 3, and 1 for the three largest indices.

    python tests/golden/make_golden_norm.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rlwe_ref as rr  # noqa: E402

INDICES = [8, 12, 23, 45, 81, 1456, 11648, 14400, 2 ** 14, 2 ** 15]


class PE(C.Structure):
    _fields_ = [("prime", C.c_int16), ("exponent", C.c_int16)]


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libctensor.so"))
    for nm in ("tensorNormSqR", "tensorNormSqD"):
        getattr(lib, nm).argtypes = [C.c_int16, C.c_void_p, C.c_int32, C.POINTER(PE), C.c_int16]
        getattr(lib, nm).restype = None
    rng = np.random.default_rng(147151)
    big = sorted(INDICES, key=lambda m: rr.totient(rr.factor_pps(m)))[-3:]
    out = {}
    for m in INDICES:
        pps = rr.factor_pps(m)
        n = rr.totient(pps)
        B = 1 if m in big else 3
        pe = (PE * len(pps))(*[PE(p, e) for p, e in pps])
        ei = np.clip(np.rint(rng.normal(size=(B, n)) * 3000.0), -2 ** 20 + 1, 2 ** 20 - 1).astype(np.int32)
        ei[0, rng.integers(0, n)] = 2 ** 20 - 1                          # the stated range's edge
        ed = (rng.normal(size=(B, n)) * 37.5).astype(np.float32)
        ed = (ed.view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)   # 16 significant bits
        ni, ndv = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float64)
        for b in range(B):
            yi = np.ascontiguousarray(ei[b], dtype=np.int64)
            lib.tensorNormSqR(1, yi.ctypes.data, n, pe, len(pps))
            ni[b] = yi[0]
            yd = np.ascontiguousarray(ed[b], dtype=np.float64)
            lib.tensorNormSqD(1, yd.ctypes.data, n, pe, len(pps))
            ndv[b] = yd[0]
        out[f"e_i_{m}"], out[f"n_i_{m}"], out[f"e_d_{m}"], out[f"n_d_{m}"] = ei, ni, ed, ndv
    path = os.path.join(HERE, "golden_norm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
