"""Host side of L, L^-1, mulG and divG over Z, R and C and of mulC (lolhip_elt_op_batch, lolhip_mulc_batch, Plan.eltOp;
DESIGN.md 3.4k): the symbols are declared, exported and bound; the numpy restatement (tests/eltops_ref.py) equals the
reference's own outputs (tests/golden/golden_eltops.npz) bit for bit, so a GPU failure points at the kernel; it obeys the
class law divG (mulG x) = x and refuses what is not divisible; every host-decided status in its stated order.  No GPU:
host-only plans."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eltops_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE = 0, -1, -5
I64, F64, C64 = 0, 1, 2
INDICES = [3, 5, 9, 12, 25, 17, 105, 252, 8]
FWD = {"l": er.OP_L, "linv": er.OP_LINV, "mulgpow": er.OP_MULGPOW, "mulgdec": er.OP_MULGDEC}


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_eltops.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_symbols_are_declared_exported_and_bound(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in ("lolhip_elt_op_batch", "lolhip_mulc_batch"):
        assert nm in names
        assert hasattr(raw, nm)
        assert getattr(lolhip.lib(), nm).argtypes is not None
    for nm in ("LOLHIP_ELT_I64 = 0", "LOLHIP_ELT_F64 = 1", "LOLHIP_ELT_C64 = 2"):
        assert nm in hdr
    for nm in ("eltOp", "lR", "lInvR", "mulGPowR", "mulGDecR", "divGPowR", "divGDecR"):
        assert callable(getattr(lolhip.Plan, nm))
    assert callable(lolhip.mulC)
    # the drop-in surface stays lol-cpp's: no second definition of its symbols for these element types
    for nm in ("tensorLR", "tensorLDouble", "tensorLC", "tensorGPowR", "tensorGPowC", "tensorGInvPowR", "tensorGInvDecC", "mulC"):
        assert not hasattr(raw, nm)


@pytest.mark.parametrize("m", INDICES)
def test_restatement_equals_the_reference_bit_for_bit(gold, m):
    pps = er.factor_pps(m)
    seen = 0
    for kind, Ts, ops in (("r", (1, 3), FWD), ("d", (1, 3), {"l": er.OP_L, "linv": er.OP_LINV}), ("c", (1, 2), FWD)):
        for T in Ts:
            x = gold[f"{kind}_in_{m}_{T}"]
            assert x.shape == (4, er.totient(pps), T)
            for name, op in ops.items():
                assert same_bits(er.elt_op(op, pps, x, T), gold[f"{kind}_{name}_{m}_{T}"]), (kind, name, m, T)
                seen += 1
    assert seen == 8 + 4 + 8


@pytest.mark.parametrize("m", INDICES)
def test_restatement_divg_transform_equals_the_reference(gold, m):
    """the reference's tensorGInv*R leave the undivided transform of mulG x (oddrad x): the prime-index part of divG"""
    pps = er.factor_pps(m)
    for T in (1, 3):
        x = gold[f"r_x_{m}_{T}"]
        for name, mul, div in (("ginvpow", er.OP_MULGPOW, er.OP_DIVGPOW), ("ginvdec", er.OP_MULGDEC, er.OP_DIVGDEC)):
            want = gold[f"r_{name}_{m}_{T}"]
            assert np.array_equal(want, x * er.oddrad(pps))
            gx = er.elt_op(mul, pps, x, T)
            assert same_bits(er.transform(div, pps, gx.view(np.uint64)).view(np.int64), want)


def divg_cases(gold, m, T):
    """(name, div op, x, g x, g x with items 1 and 3 raised by one in one coefficient) for both bases"""
    pps = er.factor_pps(m)
    x = gold[f"r_x_{m}_{T}"]
    for name, mul, div in (("pow", er.OP_MULGPOW, er.OP_DIVGPOW), ("dec", er.OP_MULGDEC, er.OP_DIVGDEC)):
        gx = er.elt_op(mul, pps, x, T)
        bad = gx.copy()
        bad[1, 0, 0] += 1
        bad[3, -1, -1] += 1
        yield name, div, x, gx, bad


@pytest.mark.parametrize("m", INDICES)
def test_restatement_obeys_the_class_law(gold, m):
    pps = er.factor_pps(m)
    flags = set()
    for T in (1, 3):
        for name, div, x, gx, bad in divg_cases(gold, m, T):
            q, ok = er.elt_op(div, pps, gx, T)
            assert ok.dtype == np.int32 and ok.tolist() == [1, 1, 1, 1] and same_bits(q, x), (name, m, T)
            q, ok = er.elt_op(div, pps, bad, T)
            flags.update(ok.tolist())
            if er.oddrad(pps) == 1:                      # m = 8: everything is divisible, nothing changes
                assert ok.tolist() == [1, 1, 1, 1] and same_bits(q, bad)
                continue
            assert ok.tolist() == [1, 0, 1, 0], (name, m, T)
            num = er.transform(div, pps, bad.view(np.uint64)).view(np.int64)
            for b in range(4):                           # divisible items are x, the others keep their numerators
                assert same_bits(q[b], x[b] if ok[b] else num[b])
            # over R and C the same input always divides: y / oddrad per component
            f = er.elt_op(div, pps, bad.astype(np.float64), T)
            assert same_bits(f, er.transform(div, pps, bad.astype(np.float64)) / float(er.oddrad(pps)))
    assert flags == ({1} if er.oddrad(pps) == 1 else {0, 1})


def test_restatement_mulc(gold):
    a, b = gold["mulc_a"], gold["mulc_b"]
    assert same_bits(er.mulc(a, b), gold["mulc_ab"])
    assert same_bits(er.mulc(a, a), gold["mulc_aa"])


def _call(lolhip, p, op=er.OP_L, elt=I64, T=1, y=None, ok=None, B=0):
    return lolhip.lib().lolhip_elt_op_batch(p._h if p else None, None, op, elt, T, y, ok, B)


def test_statuses_in_order(lolhip):
    p = lolhip.Plan(er.factor_pps(45), [12289], host_only=True)
    big = lolhip.Plan([(2, 16)], [12289], host_only=True)            # n = 32768 > 16384
    assert big.n == 32768
    # a valid call on a host-only plan: NO_DEVICE, at B = 0 too; NULL pointers are looked at only after that
    for op in er.OPS:
        for elt in (I64, F64, C64):
            for T in (1, 16):
                assert _call(lolhip, p, op, elt, T) == NO_DEVICE
                assert _call(lolhip, p, op, elt, T, y=8, ok=8, B=3) == NO_DEVICE
                assert _call(lolhip, p, op, elt, T, y=None, ok=None, B=3) == NO_DEVICE
    # INVALID first: a NULL plan, unknown op or elt, T, B, n
    assert _call(lolhip, None) == INVALID
    for op in (0, 1, 2, 3, 10, 11, -1, 12):
        assert _call(lolhip, p, op) == INVALID
    for elt in (-1, 3):
        assert _call(lolhip, p, er.OP_L, elt) == INVALID
    for T in (0, -1, 17):
        assert _call(lolhip, p, er.OP_L, I64, T) == INVALID
    assert _call(lolhip, p, B=-1) == INVALID
    assert _call(lolhip, big) == INVALID and _call(lolhip, big, y=8, B=1) == INVALID
    # the Python methods raise the same codes before they stage anything
    for call, code in ((lambda: p.eltOp(3, np.zeros((1, 24, 1), dtype=np.int64)), INVALID),
                       (lambda: p.eltOp(er.OP_L, np.zeros((1, 24, 17), dtype=np.float64)), INVALID),
                       (lambda: p.divGPowR(np.zeros((2, 24, 2), dtype=np.int64)), NO_DEVICE),
                       (lambda: p.lR(np.zeros((24,), dtype=np.complex128)), NO_DEVICE)):
        with pytest.raises(lolhip.LolHipError) as e:
            call()
        assert e.value.code == code
    with pytest.raises(TypeError):
        p.eltOp(er.OP_L, np.zeros((1, 24, 1), dtype=np.float32))


def test_mulc_statuses(lolhip):
    L = lolhip.lib()
    assert L.lolhip_mulc_batch(None, None, None, -1) == INVALID
    if lolhip.device_count() == 0:
        assert L.lolhip_mulc_batch(None, None, None, 0) == NO_DEVICE
        assert L.lolhip_mulc_batch(None, 16, 16, 4) == NO_DEVICE
        assert L.lolhip_mulc_batch(None, None, None, 4) == NO_DEVICE
    else:
        assert L.lolhip_mulc_batch(None, None, None, 0) == OK
        assert L.lolhip_mulc_batch(None, None, None, 4) == INVALID
