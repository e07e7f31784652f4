#!/usr/bin/env python3
"""Generates tests/golden/golden_float_stages.npz: lol-cpp's own tensorCRTC / tensorCRTInvC /
tensorGaussianDec (oracle/_ref/libctensor.so, built by oracle/Makefile) at the index set of
tests/float_stages.py, where every dense stage size of the float kernels occurs.  Only outputs are stored,
and of each row only the columns float_stages.fixture_columns names (all of them for n <= 384), so the file
stays small; the inputs are regenerated from a fixed seed (float_stages.stage_inputs).  Rerunning the script
reproduces the same arrays.

    python tests/golden/make_golden_float_stages.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from float_stages import STAGE_INDICES, fixture_columns, stage_inputs  # noqa: E402
from oracle import lolmath as lm  # noqa: E402
from oracle.oracle import CTRef  # noqa: E402


def main():
    ct = CTRef()
    out = {"indices": np.array(STAGE_INDICES, dtype=np.int64)}
    for m in STAGE_INDICES:
        pps = lm.factor_pps(m)
        z, g = stage_inputs(m)
        cols = fixture_columns(m)
        out[f"m{m}_crtc"] = ct.crtc(pps, z)[:, cols]
        out[f"m{m}_crtinvc"] = ct.crtinvc(pps, z)[:, cols]
        out[f"m{m}_gauss"] = ct.gaussian_dec(pps, g)[:, cols]
    path = os.path.join(ROOT, "tests", "golden", "golden_float_stages.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
