"""The ring-extension kernels (k_gather, k_gather_lds, k_twace_crt, k_coeffs and the evalLin / tunnel compositions on
them) at wide and mixed-width moduli and at every chunk layout, bit for bit against the pure-Python oracle
(CpuRef.embed_* / twace_* / coeffs, oracle/she_ref.py evallin / tunnel).

 - moduli of the UPPER index with widths cycling over 20, 31, 59 and 61 bits, plus all-61-bit and all-59-bit tuples;
 - inputs [B][n][T]: row 0 all q - 1, row 1 alternating q - 1 / 0, random rows after; every input a second time as
   representatives in (-q, 0], with the oracle on the canonical residues as the expected value;
 - CASES: the shapes and T at which launch_gather / launch_twace_crt take each of their routes (16-byte chunks with 1 to
   8 chunks per coefficient, one word per chunk with up to 16, the LDS-staged gather split over several workgroups, its
   64 KiB admission limit and the first size above it, several tiles with a partial last one).  The routes themselves
   are restated and asserted per case in tests/test_ext_width_host.py, which imports this table;
 - for even T every call is made twice: on 16-byte aligned slabs and on slabs one word off (the TW = 1 fallback);
 - ALIGN_CASES: only the input or only the output off, on a side stream, with guard words around the output;
 - LIN_CASES: evalLin and tunnel over lcm(r, s) moduli of at least 2^29 (the wide knapsack variant).
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import lolmath as lm
from oracle import she_ref as sr
from oracle.oracle import Params

pytestmark = pytest.mark.gpu

WIDTHS = (20, 31, 59, 61)
B_OPS = 3
GUARD = 0x7E7E7E7E7E7E
GUARD_AFTER = 32

SMALL = [(1, 8), (4, 12), (3, 21), (9, 45)]
SMALL_T = (1, 2, 4, 5, 6, 7, 8, 16)
# (m, m', T, moduli)
CASES = ([(m, m2, T, "mixed") for m, m2 in SMALL for T in SMALL_T] +
         [(8, 8, T, "mixed") for T in (2, 4)] +
         [(56, 2912, T, "mixed") for T in (4, 5, 6, 7)] +
         [(728, 2912, T, "mixed") for T in (4, 3)] +
         [(4096, 12288, T, "mixed") for T in (4, 5)] +
         [(4, 12, 4, "u61"), (56, 2912, 6, "u61"), (9, 45, 5, "u59"), (56, 2912, 4, "u59")])
# both / only the input / only the output one word off a 16-byte boundary: (input offset, output offset) in words
ALIGN_CASES = [(56, 2912, 4, "mixed"), (4096, 12288, 4, "mixed")]
ALIGN_OFFSETS = [(1, 1), (1, 2), (2, 1)]
# (e, r, s)
LIN_SHAPES = [(4, 12, 12), (3, 21, 21), (4, 12, 20), (8, 16, 40)]
LIN_MODULI = [(2, "mixed"), (4, "mixed"), (5, "mixed"), (2, "u61")]
LIN_CASES = [(e, r, s, T, kind) for e, r, s in LIN_SHAPES for T, kind in LIN_MODULI]
TUNNEL_BASES = (0, 16)
B_LIN = 2

OPS = ("embedPow", "embedDec", "embedCRT", "twacePowDec", "twaceCRT")
ORACLE = {"embedPow": "embed_pow", "embedDec": "embed_dec", "embedCRT": "embed_crt", "twacePowDec": "twace_powdec",
          "twaceCRT": "twace_crt"}
TO_HI = {"embedPow": True, "embedDec": True, "embedCRT": True, "twacePowDec": False, "twaceCRT": False}


def case_id(c):
    return "-".join(str(v) for v in c)


def moduli(m, T, kind):
    """T good moduli of index m: widths cycling over 20, 31, 59 and 61 bits ("mixed"), or all of one width ("u61")"""
    if kind == "mixed":
        gens = [lm.good_qs(m, 2 ** (b - 1)) for b in WIDTHS]
        return [next(gens[t % 4]) for t in range(T)]
    g = lm.good_qs(m, 2 ** (int(kind[1:]) - 1))
    return [next(g) for _ in range(T)]


def extreme(R, rng, B):
    """[B][n][T] with q - 1 everywhere (row 0), alternating q - 1 / 0 (row 1), random rows after"""
    qv = np.array(R.qs, dtype=np.int64)
    y = R.random(rng, B)
    y[0] = qv - 1
    if B > 1:
        y[1] = 0
        y[1, ::2] = qv - 1
    return y


def neg(y, qs):
    """the same residues as representatives in (-q, 0]"""
    return np.where(y > 0, y - np.asarray(qs, dtype=np.int64), 0)


def case_inputs(m, m2, T, kind):
    """moduli, oracle parameters and the two inputs of a case; the same on the host and on the GPU side"""
    qs = moduli(m2, T, kind)
    Rl, Rh = Params(lm.factor_pps(m), qs), Params(lm.factor_pps(m2), qs)
    rng = np.random.default_rng(1000 * m2 + 16 * m + T)
    return qs, Rl, Rh, extreme(Rl, rng, B_OPS), extreme(Rh, rng, B_OPS)


_cases = {}


def _case(gpu, cpuref, key):
    """plans, inputs and the oracle's answers for one case, computed once and left unchanged"""
    if key not in _cases:
        m, m2, T, kind = key
        qs, Rl, Rh, lo, hi = case_inputs(m, m2, T, kind)
        Pl, Ph = gpu.Plan(Rl.pps, qs), gpu.Plan(Rh.pps, qs)
        want = {op: getattr(cpuref, ORACLE[op])(Rl, Rh, lo if TO_HI[op] else hi) for op in OPS}
        want["coeffs"] = cpuref.coeffs(Rl, Rh, hi)
        for w in want.values():
            w.setflags(write=False)
        _cases[key] = SimpleNamespace(qs=qs, Rl=Rl, Rh=Rh, lo=lo, hi=hi, Pl=Pl, Ph=Ph, X=gpu.Ext(Pl, Ph), want=want)
    return _cases[key]


def _slab(torch, size, off, data=None):
    """`size` words that start `off` words into a fresh buffer (off = 1: 8 bytes off a 16-byte boundary, off = 2: on
    one), with guard words in front and GUARD_AFTER guard words behind"""
    buf = torch.full((off + size + GUARD_AFTER,), GUARD, dtype=torch.int64, device="cuda")
    v = buf[off:off + size]
    if data is not None:
        v.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))
    assert v.data_ptr() % 16 == (8 if off % 2 else 0)
    return buf, v


def _guards_intact(buf, off, size):
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + size:] == GUARD).all())


def _run(torch, X, op, x, out_shape, off_in, off_out, stream=None):
    """one call of the device API on slabs at the given word offsets; the output as a host array"""
    size = int(np.prod(out_shape))
    _, vin = _slab(torch, x.size, off_in, x)
    buf, vout = _slab(torch, size, off_out)
    if stream is not None:
        torch.cuda.synchronize()
    getattr(X, op)(vin, out=vout, stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    got = vout.cpu().numpy().reshape(out_shape)
    assert _guards_intact(buf, off_out, size), (op, off_in, off_out)
    return got


def _offsets(T):
    """even T: 16-byte aligned slabs (two components per access), then slabs one word off (one component per access)"""
    return ((2, 2), (1, 1)) if T % 2 == 0 else ((2, 2),)


@pytest.mark.parametrize("rep", ["canonical", "negative"])
@pytest.mark.parametrize("m,m2,T,kind", CASES, ids=[case_id(c) for c in CASES])
def test_ext_ops_match_the_oracle(gpu, cpuref, m, m2, T, kind, rep):
    import torch
    c = _case(gpu, cpuref, (m, m2, T, kind))
    lo, hi = (c.lo, c.hi) if rep == "canonical" else (neg(c.lo, c.qs), neg(c.hi, c.qs))
    rel = c.Rh.n // c.Rl.n
    for off_in, off_out in _offsets(T):
        for op in OPS:
            x, n_out = (lo, c.Rh.n) if TO_HI[op] else (hi, c.Rl.n)
            got = _run(torch, c.X, op, x, (B_OPS, n_out, T), off_in, off_out)
            assert np.array_equal(got, c.want[op]), (op, off_in)
        got = _run(torch, c.X, "coeffs", hi, (rel, B_OPS, c.Rl.n, T), off_in, off_out)
        assert np.array_equal(got, c.want["coeffs"]), ("coeffs", off_in)


@pytest.mark.parametrize("rep", ["canonical", "negative"])
@pytest.mark.parametrize("m,m2,T,kind", CASES, ids=[case_id(c) for c in CASES])
def test_ext_identities_on_the_device(gpu, cpuref, m, m2, T, kind, rep):
    """the reference's own properties (TensorTests.hs:133-234) with the GPU on both sides"""
    c = _case(gpu, cpuref, (m, m2, T, kind))
    X, Pl, Ph = c.X, c.Pl, c.Ph
    lo, hi = (c.lo, c.hi) if rep == "canonical" else (neg(c.lo, c.qs), neg(c.hi, c.qs))
    assert np.array_equal(X.twaceCRT(X.embedCRT(lo)), c.lo)
    assert np.array_equal(X.twacePowDec(X.embedPow(lo)), c.lo)
    assert np.array_equal(X.embedCRT(lo), Ph.crt(X.embedPow(Pl.crtInv(lo))))
    assert np.array_equal(X.twaceCRT(hi), Pl.crt(X.twacePowDec(Ph.crtInv(hi))))
    assert np.array_equal(X.embedDec(lo), Ph.lInv(X.embedPow(Pl.l(lo))))


@pytest.mark.parametrize("off_in,off_out", ALIGN_OFFSETS)
@pytest.mark.parametrize("m,m2,T,kind", ALIGN_CASES, ids=[case_id(c) for c in ALIGN_CASES])
def test_ext_ops_on_slabs_off_a_16_byte_boundary(gpu, cpuref, m, m2, T, kind, off_in, off_out):
    """input and output, only the input, only the output one word off: the words of the aligned call, on a side stream,
    with the guard words around the output untouched"""
    import torch
    c = _case(gpu, cpuref, (m, m2, T, kind))
    side = torch.cuda.Stream()
    for op in OPS:
        canonical = c.lo if TO_HI[op] else c.hi
        shape = (B_OPS, c.Rh.n if TO_HI[op] else c.Rl.n, T)
        for x in (canonical, neg(canonical, c.qs)):
            aligned = _run(torch, c.X, op, x, shape, 2, 2)
            got = _run(torch, c.X, op, x, shape, off_in, off_out, stream=side)
            assert np.array_equal(got, aligned), op
            assert np.array_equal(got, c.want[op]), op


# ---- evalLin / tunnel ---------------------------------------------------------------------------------------------------
def _lin_setup(gpu, e, r, s, T, kind):
    qs = moduli(r * s // math.gcd(r, s), T, kind)
    pe, pr, ps = (lm.factor_pps(x) for x in (e, r, s))
    PE, PR, PS = (Params(p_, qs) for p_ in (pe, pr, ps))
    GE, GR, GS = (gpu.Plan(p_, qs) for p_ in (pe, pr, ps))
    return qs, (PE, PR, PS), (gpu.Ext(GE, GR), gpu.Ext(GE, GS))


@pytest.mark.parametrize("e,r,s,T,kind", LIN_CASES, ids=[case_id(c) for c in LIN_CASES])
def test_evallin_at_wide_moduli(gpu, cpuref, e, r, s, T, kind):
    qs, (PE, PR, PS), (XR, XS) = _lin_setup(gpu, e, r, s, T, kind)
    assert max(qs) >= 2 ** 29                                            # the knapsack variant for moduli of 2^29 and more
    rng = np.random.default_rng(100 * r + s + T)
    x = extreme(PR, rng, B_LIN)
    ys = np.stack([PS.random(rng, 1)[0] for _ in range(PR.n // PE.n)])
    want = sr.evallin(cpuref, PE, PR, PS, x, ys)
    assert np.array_equal(XR.evalLin(XS, x, ys), want)
    assert np.array_equal(XR.evalLin(XS, neg(x, qs), ys), want), "negative"


@pytest.mark.parametrize("base", TUNNEL_BASES)
@pytest.mark.parametrize("e,r,s,T,kind", LIN_CASES, ids=[case_id(c) for c in LIN_CASES])
def test_tunnel_at_wide_moduli(gpu, cpuref, e, r, s, T, kind, base):
    qs, (PE, PR, PS), (XR, XS) = _lin_setup(gpu, e, r, s, T, kind)
    rng = np.random.default_rng(100 * r + s + T + base)
    rel, L = PR.n // PE.n, sum(sr.digit_counts(PS, base))
    c0, c1 = extreme(PR, rng, B_LIN), extreme(PR, rng, B_LIN)[::-1].copy()
    ys = np.stack([PS.random(rng, 1)[0] for _ in range(rel)])
    hints = np.stack([np.stack([np.stack([PS.random(rng, 1)[0] for _ in range(2)]) for _ in range(L)]) for _ in range(rel)])
    want = sr.tunnel(cpuref, PE, PR, PS, c0, c1, ys, hints, base)
    assert np.array_equal(XR.tunnel(XS, c0, c1, ys, hints, base), want)
    assert np.array_equal(XR.tunnel(XS, neg(c0, qs), neg(c1, qs), ys, hints, base), want), "negative"
