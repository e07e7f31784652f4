"""L, L^-1, mulG and divG over Z, R and C and mulC on the device (-m gpu), bit for bit against the numpy restatement
(tests/eltops_ref.py, which test_eltops_host.py ties to the reference's own outputs) and against the reference's outputs
themselves (tests/golden/golden_eltops.npz).

Every call runs with LOLHIP_ELT_INFO set, and the route (LDS-resident items, or one pass per odd prime from HBM) is read
from the launcher's stderr line, never assumed: every index that fits the LDS runs on both routes (debug switch
ELT_GLOBAL) and must give the same bits.  The slab and the flags sit between guard words; runs at B = 1 start 8 bytes
off a 16-byte boundary (the one-word memory path), the others on one (the two-word path)."""
import os
import re

import numpy as np
import pytest

import eltops_ref as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, F64, C64 = 0, 1, 2
FIXTURE = [3, 5, 9, 12, 25, 17, 105, 252, 8]
INDICES = FIXTURE + [128 * 7 * 13, 3 * 2 ** 14]
LDS_BYTES = 160 * 1024
GUARD = 0x5AFEC0DE5AFEC0DE
OK_GUARD = -77
INFO = re.compile(r"^k_elt: route (lds|global), op (\d), word (u64|f64), n (\d+), W (\d+), lds (\d+) B$", re.M)


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_eltops.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture
def info(monkeypatch, capfd):
    """reads the launcher's lines printed since the last call: [(route, op, word, n, W, lds bytes)]"""
    monkeypatch.setenv("LOLHIP_ELT_INFO", "1")
    capfd.readouterr()

    def read():
        return [(r, int(o), w, int(n), int(W), int(b)) for r, o, w, n, W, b in INFO.findall(capfd.readouterr().err)]
    return read


@pytest.fixture
def forced(gpu):
    """force(True / False): the ELT_GLOBAL switch, released afterwards whatever happens"""
    try:
        yield lambda on: gpu.debug_set("ELT_GLOBAL", on)
    finally:
        gpu.debug_set("ELT_GLOBAL", False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def words_of(elt, T):
    return 2 * T if elt == C64 else T


def fits_lds(n, W):
    """the route rule of DESIGN.md 3.4k: n W words, one pad word per 32 and 128 bytes of item flags within 160 KiB"""
    return lds_bytes(n, W) <= LDS_BYTES


def lds_bytes(n, W):
    return (n * W + (n * W >> 5)) * 8 + 128


def run(gpu, plan, op, elt, T, y, stream=None, off=2):
    """lolhip_elt_op_batch on a copy of y [B][n][T] between guard words (`off` of them before it).  Returns the slab, or
    (slab, ok) for divG over int64."""
    import torch
    y = np.ascontiguousarray(y)
    B = y.shape[0]
    w = y.reshape(-1).view(np.uint64)
    buf = np.full(w.size + off + 2, GUARD, dtype=np.uint64)
    buf[off:off + w.size] = w
    d = torch.from_numpy(buf.view(np.int64)).cuda()
    divi = elt == I64 and op in (er.OP_DIVGPOW, er.OP_DIVGDEC)
    dok = torch.full((B + 2,), OK_GUARD, dtype=torch.int32, device="cuda")
    s = 0 if stream is None else stream.cuda_stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rc = gpu.lib().lolhip_elt_op_batch(plan._h, s, op, elt, T, d.data_ptr() + 8 * off, dok.data_ptr() + 4 if divi else None, B)
    assert rc == 0, rc
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint64)
    assert (got[:off] == GUARD).all() and (got[off + w.size:] == GUARD).all(), "guard words around y"
    ok = dok.cpu().numpy()
    assert ok[0] == OK_GUARD and ok[-1] == OK_GUARD, "guard words around ok"
    if not divi:
        assert (ok == OK_GUARD).all(), "ok is ignored outside divG over int64"
    out = got[off:off + w.size].copy().view(y.dtype).reshape(y.shape)
    return (out, ok[1:-1].copy()) if divi else out


def make_input(rng, pps, op, elt, T, B):
    """the slab of one case.  int64: full range for L / LInv / mulG; for divG, mulG x with the odd items raised by one in
    one coefficient.  float64 / complex128: normals times 10^k, k in -8 .. 8"""
    n = er.totient(pps)
    if elt == I64:
        if op not in (er.OP_DIVGPOW, er.OP_DIVGDEC):
            return rng.integers(-2 ** 63, 2 ** 63, size=(B, n, T), dtype=np.int64)
        x = rng.integers(-2 ** 20 + 1, 2 ** 20, size=(B, n, T), dtype=np.int64)
        gx = er.elt_op(er.OP_MULGPOW if op == er.OP_DIVGPOW else er.OP_MULGDEC, pps, x, T)
        gx.reshape(B, -1)[1::2, rng.integers(0, n * T)] += 1
        return gx
    if elt == F64:
        return er.wide_floats(rng, (B, n, T))
    return er.wide_floats(rng, (B, n, T)) + 1j * er.wide_floats(rng, (B, n, T))


def check(got, want, what):
    if isinstance(want, tuple):
        assert same_bits(got[1], want[1]), ("ok", what, got[1], want[1])
        assert same_bits(got[0], want[0]), what
    else:
        assert same_bits(got, want), what


def prefix(want, B):
    return (want[0][:B], want[1][:B]) if isinstance(want, tuple) else want[:B]


@pytest.mark.parametrize("elt", [I64, F64, C64])
@pytest.mark.parametrize("m", INDICES)
def test_device_equals_restatement(gpu, info, forced, m, elt):
    pps = er.factor_pps(m)
    n = er.totient(pps)
    plan = gpu.Plan(pps, [12289])                       # the moduli play no role
    rng = np.random.default_rng(m * 3 + elt)
    odd = er.oddrad(pps) > 1
    for T in (1, 2, 3):
        W = words_of(elt, T)
        Bfull = max(3, -(-4096 // (n * W)))             # at least 4096 values per case
        routes = ["lds", "global"] if fits_lds(n, W) else ["global"]
        if m == 3 * 2 ** 14:
            assert routes == (["lds", "global"] if (elt, T) in ((I64, 1), (F64, 1)) else ["global"])
        for op in er.OPS:
            y = make_input(rng, pps, op, elt, T, Bfull)
            want = er.elt_op(op, pps, y, T)
            if isinstance(want, tuple) and odd:
                assert set(want[1].tolist()) == {0, 1} and want[1][0] == 1 and want[1][1] == 0
            for route in routes:
                forced(route == "global" and "lds" in routes)
                for B in sorted({1, 3, Bfull}):
                    got = run(gpu, plan, op, elt, T, y[:B], off=1 if B == 1 else 2)
                    check(got, prefix(want, B), (m, elt, T, op, route, B))
                    lines = info()
                    if odd:
                        assert lines == [(route, op - er.OP_L, "u64" if elt == I64 else "f64", n, W,
                                          0 if route == "global" else lds_bytes(n, W))], (lines, route)
                    else:
                        assert lines == []              # m = 2^k: the identity, nothing but the flags is launched
            forced(False)


@pytest.mark.parametrize("m", FIXTURE)
def test_device_equals_the_reference(gpu, gold, m):
    """the reference's own outputs, where it is right: L, LInv, mulGPow, mulGDec over R, Double and C"""
    pps = er.factor_pps(m)
    plan = gpu.Plan(pps, [12289])
    fwd = {"l": er.OP_L, "linv": er.OP_LINV, "mulgpow": er.OP_MULGPOW, "mulgdec": er.OP_MULGDEC}
    for kind, elt, Ts, names in (("r", I64, (1, 3), fwd), ("d", F64, (1, 3), ("l", "linv")), ("c", C64, (1, 2), fwd)):
        for T in Ts:
            for name in names:
                got = run(gpu, plan, fwd[name], elt, T, gold[f"{kind}_in_{m}_{T}"])
                assert same_bits(got, gold[f"{kind}_{name}_{m}_{T}"]), (kind, name, m, T)
    for T in (1, 3):                                     # the class law on the reference's own mulG x
        x = gold[f"r_x_{m}_{T}"]
        for mul, div in ((er.OP_MULGPOW, er.OP_DIVGPOW), (er.OP_MULGDEC, er.OP_DIVGDEC)):
            gx = run(gpu, plan, mul, I64, T, x)
            q, ok = run(gpu, plan, div, I64, T, gx)
            assert ok.tolist() == [1, 1, 1, 1] and same_bits(q, x)


@pytest.mark.parametrize("m", [5, 12])
def test_many_items(gpu, info, forced, m):
    """B = 1025: many chunks of 32 items and a ragged last one"""
    pps = er.factor_pps(m)
    plan = gpu.Plan(pps, [12289])
    rng = np.random.default_rng(m)
    for elt, T, op in ((I64, 1, er.OP_L), (I64, 3, er.OP_DIVGPOW), (I64, 1, er.OP_DIVGDEC), (F64, 2, er.OP_DIVGDEC),
                       (C64, 1, er.OP_MULGDEC), (F64, 1, er.OP_LINV), (I64, 2, er.OP_MULGPOW)):
        y = make_input(rng, pps, op, elt, T, 1025)
        want = er.elt_op(op, pps, y, T)
        for route in ("lds", "global"):
            forced(route == "global")
            check(run(gpu, plan, op, elt, T, y), want, (m, elt, T, op, route))
            assert [ln[0] for ln in info()] == [route]
        forced(False)


def test_grid_stride(gpu, info, forced):
    """m = 3, B = 2^20 + 5: more chunks than the on-chip launch has workgroups and more vectors than the global one has
    threads, so both kernels go round their grid-stride loops"""
    pps = er.factor_pps(3)
    plan = gpu.Plan(pps, [12289])
    rng = np.random.default_rng(3)
    B = 2 ** 20 + 5
    for elt, op in ((I64, er.OP_L), (I64, er.OP_DIVGPOW), (F64, er.OP_DIVGDEC)):
        y = make_input(rng, pps, op, elt, 1, B)
        want = er.elt_op(op, pps, y, 1)
        for route in ("lds", "global"):
            forced(route == "global")
            check(run(gpu, plan, op, elt, 1, y), want, (elt, op, route))
            assert [ln[0] for ln in info()] == [route]
        forced(False)


def test_large_prime(gpu, info, forced):
    """m = 1021: one vector of 1020 words per item and component, one thread each (a plan of a much larger prime takes
    too long to build for a test)"""
    pps = [(1021, 1)]
    plan = gpu.Plan(pps, [12289])
    rng = np.random.default_rng(1021)
    for elt, T, ops in ((I64, 1, er.OPS), (F64, 2, (er.OP_L, er.OP_MULGPOW, er.OP_DIVGDEC))):
        for op in ops:
            y = make_input(rng, pps, op, elt, T, 5)
            want = er.elt_op(op, pps, y, T)
            for route in ("lds", "global"):
                forced(route == "global")
                check(run(gpu, plan, op, elt, T, y), want, (elt, op, route))
                assert [ln[0] for ln in info()] == [route]
            forced(False)


def test_side_stream_and_split(gpu, forced):
    import torch
    pps = er.factor_pps(105)
    plan = gpu.Plan(pps, [12289])
    rng = np.random.default_rng(105)
    side = torch.cuda.Stream()
    for elt, T, op in ((I64, 2, er.OP_DIVGDEC), (C64, 1, er.OP_DIVGPOW), (F64, 3, er.OP_L)):
        y = make_input(rng, pps, op, elt, T, 7)
        want = er.elt_op(op, pps, y, T)
        for route in ("lds", "global"):
            forced(route == "global")
            check(run(gpu, plan, op, elt, T, y, stream=side), want, (elt, op, route, "side stream"))
            whole, a, b = run(gpu, plan, op, elt, T, y), run(gpu, plan, op, elt, T, y[:3]), run(gpu, plan, op, elt, T, y[3:])
            if isinstance(whole, tuple):
                assert same_bits(np.concatenate([a[1], b[1]]), whole[1]) and set(whole[1].tolist()) == {0, 1}
                whole, a, b = whole[0], a[0], b[0]
            assert same_bits(np.concatenate([a, b]), whole)
        forced(False)


def test_python_interface(gpu, gold):
    import torch
    pps = er.factor_pps(105)
    plan = gpu.Plan(pps, [12289])
    x = gold["r_in_105_3"]
    assert same_bits(plan.lR(x), gold["r_l_105_3"]) and same_bits(plan.lInvR(x), gold["r_linv_105_3"])
    assert same_bits(plan.mulGPowR(x), gold["r_mulgpow_105_3"]) and same_bits(plan.mulGDecR(x), gold["r_mulgdec_105_3"])
    assert same_bits(plan.lR(gold["d_in_105_1"][:, :, 0]), gold["d_l_105_1"][:, :, 0])          # [B][n]: T = 1
    assert same_bits(plan.mulGDecR(gold["c_in_105_2"]), gold["c_mulgdec_105_2"])
    small = gold["r_x_105_1"]
    t = torch.from_numpy(small.copy()).cuda()
    assert plan.mulGPowR(t) is t                         # a device tensor is transformed in place
    q, ok = plan.divGPowR(t)
    assert q is t and ok.dtype == torch.int32 and ok.cpu().tolist() == [1, 1, 1, 1] and same_bits(t.cpu().numpy(), small)
    bad = plan.mulGDecR(small)
    bad[2, 5, 0] += 1
    q, ok = plan.divGDecR(bad)
    want = er.elt_op(er.OP_DIVGDEC, pps, bad, 1)
    assert same_bits(ok, want[1]) and ok.tolist() == [1, 1, 0, 1] and same_bits(q, want[0])
    f = plan.divGDecR(bad.astype(np.float64))
    assert same_bits(f, er.elt_op(er.OP_DIVGDEC, pps, bad.astype(np.float64), 1))


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2 ** 16 + 3])
def test_mulc(gpu, gold, count):
    import torch
    if count <= 257:
        a, b = gold["mulc_a"][:count], gold["mulc_b"][:count]
        assert same_bits(er.mulc(a, b), gold["mulc_ab"][:count]) and same_bits(er.mulc(a, a), gold["mulc_aa"][:count])
    else:
        rng = np.random.default_rng(count)
        a = er.wide_floats(rng, count) + 1j * er.wide_floats(rng, count)
        b = er.wide_floats(rng, count) + 1j * er.wide_floats(rng, count)
    assert same_bits(gpu.mulC(a, b), er.mulc(a, b))
    ta = torch.from_numpy(a.copy()).cuda()
    assert gpu.mulC(ta, ta) is ta                        # b aliasing a: the square
    assert same_bits(ta.cpu().numpy(), er.mulc(a, a))
    # 8 bytes off a 16-byte boundary (the one-word memory path), between guard words
    buf = np.full(2 * count + 3, np.float64(-7.25))
    buf[1:1 + 2 * count] = a.view(np.float64)
    da, db = torch.from_numpy(buf).cuda(), torch.from_numpy(np.concatenate([[0.0], b.view(np.float64)])).cuda()
    assert gpu.lib().lolhip_mulc_batch(0, da.data_ptr() + 8, db.data_ptr() + 8, count) == 0
    torch.cuda.synchronize()
    got = da.cpu().numpy()
    assert got[0] == -7.25 and (got[1 + 2 * count:] == -7.25).all()
    assert same_bits(got[1:1 + 2 * count].copy().view(np.complex128), er.mulc(a, b))
