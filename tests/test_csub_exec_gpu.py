"""GPU parity (-m gpu) of the 64-bit class's kernels with the EXEC-predicated lazy-range trims (csubx, zq_dev.h;
DESIGN.md 3.1e): crt, crtInv and polymul (distinct operands, squaring, out aliasing an operand) bit-exact against
the CPU oracle at L = 4..14, q just above 2^60 and just below 2^61, T = 1 and T = 2, B = 5 (ragged) and B = 1,
through the routes NO_T1 x NO_TRUNC.

Operands are chosen so that the lanes of one wave decide differently in the trims and so that range ends are
reached: all q - 1, all -(q - 1), all zero, a single non-zero coefficient at position 0 / 1 / n - 1, alternating
0 and q - 1, and random residues (with reference-style negative representatives mixed in).
tests/test_csub_exec_host.py checks the generated code statically; tools/microbench_csub.hip the trim alone on
every 64-bit value.
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


def _moduli(L, q, T):
    """T = 1: q itself; T = 2: q and the next NTT-friendly prime of the same size (below q at the top of the class)"""
    if T == 1:
        return [q]
    m = 1 << (L + 1)
    if q == Q_LO:
        g = lm.good_qs(m, q)
        q2 = next(g)
        while q2 == q:
            q2 = next(g)
    else:
        q2 = q - m
        while not lm.is_prime(q2):
            q2 -= m
    assert q2 != q and q2 % m == 1 and (1 << 60) < q2 < (1 << 61)
    return [q, q2]


PATTERNS = ("max", "negmax", "zero", "e0", "e1", "elast", "alt", "random")


def _operand(R, rng, B, kind):
    """[B, n, T] int64 in (-q, q) per component"""
    n, T = R.n, R.T
    qs = np.array(R.qs, dtype=np.int64)
    y = np.zeros((B, n, T), dtype=np.int64)
    if kind == "max":
        y[:] = qs - 1
    elif kind == "negmax":
        y[:] = -(qs - 1)
    elif kind == "zero":
        pass
    elif kind in ("e0", "e1", "elast"):
        pos = {"e0": 0, "e1": 1, "elast": n - 1}[kind]
        y[:, pos, :] = qs - 1 - np.arange(B, dtype=np.int64)[:, None]      # a different non-zero value per polynomial
    elif kind == "alt":
        y[:, 1::2, :] = qs - 1
    else:
        y = R.random(rng, B)
        y[0] = np.where(y[0] > 0, y[0] - qs, 0)                            # reference-style (-q, 0] representatives
    return np.ascontiguousarray(y)


def _canon(R, y):
    qs = np.array(R.qs, dtype=np.int64)
    return np.where(y < 0, y + qs, y)


@pytest.mark.parametrize("B", [5, 1], ids=["B5", "B1"])
@pytest.mark.parametrize("T", [1, 2], ids=["T1", "T2"])
@pytest.mark.parametrize("q", [Q_LO, Q_HI], ids=["q2^60", "q2^61-"])
@pytest.mark.parametrize("L", list(range(4, 15)))
def test_csub_exec_parity(routes, cpuref, L, q, T, B):
    gpu = routes
    rng = np.random.default_rng(L * 131 + T * 17 + B + (q & 0xFF))
    pps = [(2, L + 1)]
    qs = _moduli(L, q, T)
    P, R = gpu.Plan(pps, qs), Params(pps, qs)
    assert R.n == 1 << L
    ops = {k: _operand(R, rng, B, k) for k in PATTERNS}
    # operand pairs: every pattern against random and against itself's neighbour, so products of range ends occur too
    pairs = [(k, "random") for k in PATTERNS] + [("max", "max"), ("max", "negmax"), ("alt", "max"), ("elast", "elast"), ("e1", "alt")]
    want_crt = {k: cpuref.crt(R, _canon(R, ops[k]).copy()) for k in PATTERNS}
    want_inv = {k: cpuref.crtinv(R, _canon(R, ops[k]).copy()) for k in PATTERNS}
    want_mul = {(a, b): cpuref.polymul(R, _canon(R, ops[a]), _canon(R, ops[b])) for a, b in pairs}
    want_sq = {k: cpuref.polymul(R, _canon(R, ops[k]), _canon(R, ops[k])) for k in PATTERNS}
    for no_t1 in (False, True):
        gpu.debug_set("NO_T1", no_t1)
        for no_trunc in (False, True):
            gpu.debug_set("NO_TRUNC", no_trunc)
            tag = (L, qs, B, "NO_T1" if no_t1 else "t1", "NO_TRUNC" if no_trunc else "trunc")
            for k in PATTERNS:
                assert np.array_equal(P.crt(ops[k].copy()), want_crt[k]), tag + ("crt", k)
                assert np.array_equal(P.crtInv(ops[k].copy()), want_inv[k]), tag + ("crtInv", k)
                assert np.array_equal(P.polymul(ops[k], ops[k]), want_sq[k]), tag + ("square", k)
                da = torch.from_numpy(ops[k].copy()).cuda()
                P.polymul(da, da, out=da)                                   # squaring in place
                torch.cuda.synchronize()
                assert np.array_equal(da.cpu().numpy(), want_sq[k]), tag + ("a *= a", k)
            for a, b in pairs:
                assert np.array_equal(P.polymul(ops[a], ops[b]), want_mul[(a, b)]), tag + ("polymul", a, b)
                da, db = torch.from_numpy(ops[a].copy()).cuda(), torch.from_numpy(ops[b].copy()).cuda()
                P.polymul(da, db, out=da)                                   # c aliasing a
                torch.cuda.synchronize()
                assert np.array_equal(da.cpu().numpy(), want_mul[(a, b)]), tag + ("c = a", a, b)
                da = torch.from_numpy(ops[a].copy()).cuda()
                P.polymul(da, db, out=db)                                   # c aliasing b
                torch.cuda.synchronize()
                assert np.array_equal(db.cpu().numpy(), want_mul[(a, b)]), tag + ("c = b", a, b)
