"""GPU parity (-m gpu) of the truncated-NTT route of the 61-bit fused poly-mul (k_pow2 TR, pow2_impl.h):
both forward transforms stop after level L - 2, a degree-3 base case multiplies in registers, the inverse
starts at level L - 2.  Bit-exact against the CPU oracle, with the route on and forced off (NO_TRUNC),
through the 16-byte and the 8-byte kernels (NO_T1), at L = 11..14, q just above 2^60 and just below 2^61.
tests/test_trunc_model.py checks the same level structure and its ranges on the CPU.
"""
import numpy as np
import pytest
import torch

from oracle import lolmath as lm
from oracle.oracle import Params
from test_trunc_model import Q_HI, Q_LO

pytestmark = pytest.mark.gpu


@pytest.fixture
def routes(gpu):
    yield gpu
    gpu.debug_set("NO_TRUNC", False)
    gpu.debug_set("NO_T1", False)


def _inputs(R, rng, B, q):
    y, z = R.random(rng, B), R.random(rng, B)
    y[0] = np.where(y[0] > 0, y[0] - q, 0)                 # reference-style (-q, 0] representatives
    z[1] = -(q - 1)
    y[-1] = q - 1                                          # all-(q-1) operand
    z[-1] = q - 1
    return y, z


@pytest.mark.parametrize("q", [Q_LO, Q_HI], ids=["q2^60", "q2^61-"])
@pytest.mark.parametrize("L", [11, 12, 13, 14])
def test_trunc_polymul(routes, cpuref, L, q):
    gpu = routes
    rng = np.random.default_rng(L * 7 + (q & 0xFF))
    pps = [(2, L + 1)]
    P, R = gpu.Plan(pps, [q]), Params(pps, [q])
    B = 5                                                  # ragged: not a multiple of any launch granule
    y, z = _inputs(R, rng, B, q)
    want = cpuref.polymul(R, y, z)
    want_sq = cpuref.polymul(R, y, y)
    for no_t1 in (False, True):
        gpu.debug_set("NO_T1", no_t1)
        for no_trunc in (False, True):
            gpu.debug_set("NO_TRUNC", no_trunc)
            tag = (L, q, no_t1, no_trunc)
            assert np.array_equal(P.polymul(y, z), want), tag
            assert np.array_equal(P.polymul(y, y), want_sq), tag + ("square",)
            # on the device: c aliasing a, and squaring in place
            da, db = torch.from_numpy(y.copy()).cuda(), torch.from_numpy(z).cuda()
            P.polymul(da, db, out=da)
            torch.cuda.synchronize()
            assert np.array_equal(da.cpu().numpy(), want), tag + ("c = a",)
            da = torch.from_numpy(y.copy()).cuda()
            P.polymul(da, da, out=da)
            torch.cuda.synchronize()
            assert np.array_equal(da.cpu().numpy(), want_sq), tag + ("a *= a",)


def test_trunc_two_moduli(routes, cpuref):
    """T = 2: the 8-byte kernel with per-component tables and scale pairs."""
    gpu = routes
    L = 13
    g = lm.good_qs(1 << (L + 1), 1 << 60)
    qs = [next(g), next(g)]
    pps = [(2, L + 1)]
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    rng = np.random.default_rng(3)
    y, z = R.random(rng, 3), R.random(rng, 3)
    want = cpuref.polymul(R, y, z)
    for no_trunc in (False, True):
        gpu.debug_set("NO_TRUNC", no_trunc)
        assert np.array_equal(P.polymul(y, z), want), no_trunc
