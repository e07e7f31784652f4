#!/usr/bin/env python3
"""tests/golden/make_golden_scalar.py — known answers of the reference's own lol-cpp C++ at indices with a prime
factor >= 17, for tests/test_scalar_interp_host.py.

The other fixtures stop at m = 89 (a prime, e = 1).  The GPU tests of the scalar stage interpreter
(tests/test_scalar_interp.py) compare with the restatement oracle/cpu_ref.c at composites, prime powers and
2^e * 17; this fixture pins the restatement there: seeded inputs (seed 17) through the reference library, inputs and
outputs stored as data in tests/golden/golden_scalar.npz.

Keys:  <m>/{q,y,crt,crtinv,<prime op>}  for m in INDICES: two polynomials [2][n][1], q the largest good prime
       below 2^31 (the reference's arithmetic is valid below ~2^31.5).  Row 1 holds q - 1 at the even coefficients.

Usage:  python tests/golden/make_golden_scalar.py      (rewrites golden_scalar.npz; needs the reference tree)
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
from params import PRIME_OPS  # noqa: E402

INDICES = (51, 153, 221, 289, 323, 544)
SEED = 17


def modulus(m):
    """largest prime q = 1 (mod m) below 2^31"""
    q = (2 ** 31 - 2) // m * m + 1
    while not lm.is_prime(q):
        q -= m
    return q


def inputs(P, rng):
    y = P.random(rng, 2)
    y[1, ::2] = P.qs[0] - 1
    return y


def main():
    build(ref=True)
    ct = CTRef()
    out = {}
    rng = np.random.default_rng(SEED)
    for m in INDICES:
        q = modulus(m)
        P = Params(lm.factor_pps(m), [q])
        y = inputs(P, rng)
        out[f"{m}/q"] = np.array([q], dtype=np.int64)
        out[f"{m}/y"] = y
        for op in ("crt", "crtinv") + PRIME_OPS:
            r = getattr(ct, op)(P, y)
            assert r is not None, (m, op)
            out[f"{m}/{op}"] = np.asarray(r, dtype=np.int64)
    path = os.path.join(HERE, "golden_scalar.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
