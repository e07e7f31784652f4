#!/usr/bin/env python3
"""tests/golden/make_golden_live.py — known answers of the reference's own lol-cpp C++ for the
seeded inputs of the cross-checks in tests/test_oracle.py and tests/test_float.py.

Those checks once called the reference library (oracle/_ref/libctensor.so) while the tests ran,
so they only ran where the reference tree was at hand.  This script draws the same inputs from
the same seeds, runs them through the reference library, and stores inputs and outputs as data
in tests/golden/golden_live.npz; the tests compare the restatements against that fixture.

Keys:  zq/<k>/{y,z,crt,crtinv,mul,<prime op>}   for the k-th (m, qs) of ZQ_CASES (seed 11);
       neg/{y,<op>}                            reference-style negative inputs at m = 21, q = 8191 (seed 12);
       fl/<m>/{z,g,crtc,crtinvc_crtc,gauss}    CRT over C and the Gaussian decoding-basis map (seed 5).
A prime op the reference refuses (Nothing) has no key.

Usage:  python tests/golden/make_golden_live.py        (rewrites golden_live.npz; needs the reference tree)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import lolmath as lm  # noqa: E402
from oracle.oracle import CTRef, Params, build  # noqa: E402
from params import PRIME_OPS, TENSOR1  # noqa: E402

ZQ_CASES = TENSOR1 + [(45, [1171, 1531]), (1155, [1051051]), (432, [1297]), (2048, [12289])]
NEG_OPS = ("crt", "crtinv", "l", "linv", "gpow", "gdec", "ginvpow", "ginvdec")
FLOAT_INDICES = (12, 25, 35, 2 ** 6 * 3)


def main():
    build(ref=True)
    ct = CTRef()
    out = {}

    rng = np.random.default_rng(11)
    for k, (m, qs) in enumerate(ZQ_CASES):
        P = Params(lm.factor_pps(m), qs)
        y, z = P.random(rng, 2), P.random(rng, 2)
        out[f"zq/{k}/y"], out[f"zq/{k}/z"] = y, z
        for op in ("crt", "crtinv") + PRIME_OPS:
            r = getattr(ct, op)(P, y)
            if r is not None:
                out[f"zq/{k}/{op}"] = np.asarray(r, dtype=np.int64)
        out[f"zq/{k}/mul"] = np.asarray(ct.mul(P, y, z), dtype=np.int64)

    rng = np.random.default_rng(12)
    P = Params(lm.factor_pps(21), [8191])
    y = P.random(rng, 1) - 8191 // 2
    out["neg/y"] = y
    for op in NEG_OPS:
        out[f"neg/{op}"] = np.asarray(getattr(ct, op)(P, y), dtype=np.int64)

    rng = np.random.default_rng(5)
    for m in FLOAT_INDICES:
        pps = lm.factor_pps(m)
        n = lm.totient_pps(pps)
        z = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
        crtc = ct.crtc(pps, z)
        g = rng.standard_normal((2, n))
        out[f"fl/{m}/z"], out[f"fl/{m}/g"] = z, g
        out[f"fl/{m}/crtc"] = crtc
        out[f"fl/{m}/crtinvc_crtc"] = ct.crtinvc(pps, crtc)
        out[f"fl/{m}/gauss"] = ct.gaussian_dec(pps, g)

    path = os.path.join(HERE, "golden_live.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
