"""Child process of tests/test_gauss_dense.py: gaussianDec on opted-in plans at the indices given on the command line,
inputs as tests/float_stages.stage_inputs, outputs to an .npz.  The parent starts it with LOLHIP_GAUSS_DENSE set (the
switch is read when a plan is built and conftest does not release it, so it never enters the test process) and with
LOLHIP_GAUSS_INFO, and reads the launcher's lines from its stderr.

    python tests/gauss_dense_child.py OUT.npz M [M ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lol_amd
    from float_stages import stage_inputs
    from oracle import lolmath as lm
    out = {}
    for m in (int(a) for a in sys.argv[2:]):
        P = lol_amd.Plan.for_index(m, [lm.first_good_q(m, 1000)], dense_gauss=True)
        out[f"m{m}"] = P.gaussianDec(stage_inputs(m)[1])
        out[f"route{m}"] = np.array(P.gaussRoute())
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
