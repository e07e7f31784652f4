"""Child process of tests/test_cplx_dense.py: crtC and crtInvC on plans created with dense_cplx=True at the indices
given on the command line, inputs as tests/float_stages.stage_inputs, outputs to an .npz.  The parent starts it with
LOLHIP_CPLX_DENSE and / or LOLHIP_CPLX_DENSE_VALU set (the switches are read when a plan is built, so they never enter
the test process) and with LOLHIP_CPLX_INFO, and reads the launcher's lines from its stderr: two per index, crtC first.

    python tests/cplx_dense_child.py OUT.npz M [M ...]
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
    out = {}
    for m in (int(a) for a in sys.argv[2:]):
        P = lol_amd.Plan.for_index(m, [12289], dense_cplx=True)
        z = stage_inputs(m)[0]
        out[f"route{m}"] = np.array(P.cplxRoute())
        out[f"crtc{m}"] = P.crtC(z)
        out[f"crtinvc{m}"] = P.crtInvC(z)
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
