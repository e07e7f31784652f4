#!/usr/bin/env python3
"""Generates tests/golden/golden_gauss_dense.npz: lol-cpp's own tensorGaussianDec (oracle/_ref/libctensor.so, built by
oracle/Makefile) at the indices of tests/gauss_dense_cases.py, each with a prime above 13.  Only outputs are stored,
and of each row only the columns float_stages.fixture_columns names (all of them for n <= 384); the inputs are
regenerated from a fixed seed (float_stages.stage_inputs).  Rerunning the script reproduces the same arrays.

    python tests/golden/make_golden_gauss_dense.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from float_stages import fixture_columns, stage_inputs  # noqa: E402
from gauss_dense_cases import DENSE_INDICES  # noqa: E402
from oracle import lolmath as lm  # noqa: E402
from oracle.oracle import CTRef  # noqa: E402


def main():
    ct = CTRef()
    out = {"indices": np.array(DENSE_INDICES, dtype=np.int64)}
    for m in DENSE_INDICES:
        out[f"m{m}_gauss"] = ct.gaussian_dec(lm.factor_pps(m), stage_inputs(m)[1])[:, fixture_columns(m)]
    path = os.path.join(ROOT, "tests", "golden", "golden_gauss_dense.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
