"""Generator of tests/golden/golden_eltops.npz: inputs and outputs of the reference's own tensorL / tensorLInv / tensorGPow /
tensorGDec over R (int64), Double (L and LInv: all the reference has) and C, of mulC, and the UNDIVIDED result of
tensorGInvPowR / tensorGInvDecR on mulG x, called through ctypes on oracle/_ref/libctensor.so (built by
`make -C oracle ref`).  hDim_t is int32, hShort_t int16; one call per polynomial, tupSize = T.

Per index m and T (B = 4 polynomials, slabs [B][n][T]):
  r_in_<m>_<T>   int64, full range               r_<op>_<m>_<T>   op in l, linv, mulgpow, mulgdec
  r_x_<m>_<T>    int64, |x| < 2^20               r_ginvpow_<m>_<T>, r_ginvdec_<m>_<T>: tensorGInv{Pow,Dec}R on the
                 reference's own tensorG{Pow,Dec}R x.  Its divisibility test is inverted (g.cpp:175-181, 228-234), so it
                 returns 0 at the first coefficient and leaves the transform, oddrad x, untouched: the prime-index part
                 of divG.  (At m = 8 there is nothing to divide by: oddrad = 1 and the result is x.)
  d_in_<m>_<T>   float64                         d_l_<m>_<T>, d_linv_<m>_<T>
  c_in_<m>_<T>   complex128 (T = 1, 2)           c_<op>_<m>_<T>   op as for r
mulc_a, mulc_b [257] complex128, mulc_ab = a * b, mulc_aa = a * a with b a COPY of a.  (Called with b == a the reference
reads b.real after it has stored the new a.real, types.h:149-150, and returns a_re a_im + a_im new_re as the imaginary
part; its one caller always passes a fresh copy of a, CPP.hs:364-374 cZipDispatch.  The device reads both operands before it writes, so its
aliased call is the square.)
Floats are normals times 10^k, k in -8 .. 8 per value.

    python tests/golden/make_golden_eltops.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eltops_ref as er  # noqa: E402

INDICES = [3, 5, 9, 12, 25, 17, 105, 252, 8]
B = 4
OPS = {"l": "tensorL", "linv": "tensorLInv", "mulgpow": "tensorGPow", "mulgdec": "tensorGDec"}


class PE(C.Structure):
    _fields_ = [("prime", C.c_int16), ("exponent", C.c_int16)]


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libctensor.so"))
    names = [f + s for f in OPS.values() for s in ("R", "C")] + ["tensorLDouble", "tensorLInvDouble", "tensorGInvPowR",
                                                                  "tensorGInvDecR"]
    for nm in names:
        getattr(lib, nm).argtypes = [C.c_int16, C.c_void_p, C.c_int32, C.POINTER(PE), C.c_int16]
        getattr(lib, nm).restype = C.c_int16 if "GInv" in nm else None
    lib.mulC.argtypes = [C.c_int16, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mulC.restype = None
    rng = np.random.default_rng(20261020)
    out = {}

    def run(name, y, T, n, pe, npe):
        y = np.array(y, copy=True)
        for b in range(B):
            row = np.ascontiguousarray(y[b])
            getattr(lib, name)(T, row.ctypes.data, n, pe, npe)
            y[b] = row
        return y

    for m in INDICES:
        pps = er.factor_pps(m)
        n = er.totient(pps)
        pe = (PE * len(pps))(*[PE(p, e) for p, e in pps])
        for T in (1, 3):
            k = f"{m}_{T}"
            r_in = rng.integers(-2 ** 63, 2 ** 63, size=(B, n, T), dtype=np.int64)
            out[f"r_in_{k}"] = r_in
            for op, fn in OPS.items():
                out[f"r_{op}_{k}"] = run(fn + "R", r_in, T, n, pe, len(pps))
            x = rng.integers(-2 ** 20 + 1, 2 ** 20, size=(B, n, T), dtype=np.int64)
            out[f"r_x_{k}"] = x
            out[f"r_ginvpow_{k}"] = run("tensorGInvPowR", run("tensorGPowR", x, T, n, pe, len(pps)), T, n, pe, len(pps))
            out[f"r_ginvdec_{k}"] = run("tensorGInvDecR", run("tensorGDecR", x, T, n, pe, len(pps)), T, n, pe, len(pps))
            d_in = er.wide_floats(rng, (B, n, T))
            out[f"d_in_{k}"] = d_in
            out[f"d_l_{k}"] = run("tensorLDouble", d_in, T, n, pe, len(pps))
            out[f"d_linv_{k}"] = run("tensorLInvDouble", d_in, T, n, pe, len(pps))
        for T in (1, 2):
            k = f"{m}_{T}"
            c_in = er.wide_floats(rng, (B, n, T)) + 1j * er.wide_floats(rng, (B, n, T))
            out[f"c_in_{k}"] = c_in
            for op, fn in OPS.items():
                out[f"c_{op}_{k}"] = run(fn + "C", c_in, T, n, pe, len(pps))
    a = er.wide_floats(rng, 257) + 1j * er.wide_floats(rng, 257)
    b = er.wide_floats(rng, 257) + 1j * er.wide_floats(rng, 257)
    ab, aa, a2 = a.copy(), a.copy(), a.copy()
    lib.mulC(1, ab.ctypes.data, b.ctypes.data, 257)
    lib.mulC(1, aa.ctypes.data, a2.ctypes.data, 257)
    out["mulc_a"], out["mulc_b"], out["mulc_ab"], out["mulc_aa"] = a, b, ab, aa
    path = os.path.join(HERE, "golden_eltops.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
