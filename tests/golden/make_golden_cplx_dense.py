#!/usr/bin/env python3
"""Generates tests/golden/golden_cplx_dense.npz: lol-cpp's own tensorCRTC / tensorCRTInvC (crt.cpp:583-598) at the indices
of tests/cplx_dense_cases.DENSE_INDICES, run from the reference's sources (oracle/_ref/libctensor.so, built by
oracle/Makefile).  Inputs are tests/float_stages.stage_inputs(m) (regenerated from the seed, not stored); of the outputs
the fixture keeps float_stages.fixture_columns(m): every column up to n = 384, a seeded sample of 384 beyond.

    python tests/golden/make_golden_cplx_dense.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cplx_dense_cases import DENSE_INDICES  # noqa: E402
from float_stages import fixture_columns, stage_inputs  # noqa: E402
from oracle import lolmath as lm  # noqa: E402
from oracle.oracle import CTRef  # noqa: E402


def main():
    ct = CTRef()
    out = {"indices": np.array(DENSE_INDICES, dtype=np.int64)}
    for m in DENSE_INDICES:
        pps = lm.factor_pps(m)
        z = stage_inputs(m)[0]
        cols = fixture_columns(m)
        out[f"m{m}_crtc"] = ct.crtc(pps, z)[:, cols]
        out[f"m{m}_crtinvc"] = ct.crtinvc(pps, z)[:, cols]
    path = os.path.join(ROOT, "tests", "golden", "golden_cplx_dense.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
