"""The scan route of the prime ops at primes above 13 (zqscan.hip; plans created with scan_zq=True, LOLHIP_ROUTE_SCAN_ZQ), -m gpu.

Every case runs L, LInv, mulGPow, mulGDec, divGPow and divGDec on an opted-in plan and on a default plan (the scalar
interpreter k_generic, as before) and compares both with each other and with the CPU oracle: `np.array_equal`, no
tolerance anywhere in this file.  The launcher's line (LOLHIP_ZQ_SCAN_INFO, read at every launch) names every stage with
its prime, length, stride and layout; every case asserts it, and that the default plan prints none.

    vector length    prime indices 17, 67, 257, 797, 1021: part of one 64-lane round, one round + 2, four exact rounds,
                     ragged, sixteen rounds
    strides          1, 4, 12 (60 of 64 lanes live, behind a 12-vector stage), 16 (two large primes), a prime power's folded
                     blocks, 64 and 128 (a lane per column); d = 2 .. 12 under ZQ_SCAN against the vector interpreter
    moduli           2, 16, 103, the top of the 4-byte words, the first 8-byte modulus, the tops below 2^61 and 2^62, a
                     three-modulus tuple, a narrow / wide pair, 2^20 (no CRT basis), a multiple of 17 (divG refuses)
    inputs           test_scalar_interp._inputs (random, q - 1 everywhere, alternating, representatives in (-q, 0]) and a
                     row that is q - 1 at the last coefficient only (mulGPow reads it before it overwrites anything)
    batches          B = 1, one more than a tile, three tiles + 1 on a grid of 2, a side stream between guard rows
    composed         RLWE instances and RingRLWE at m = 257, challenges generate -> verify, encrypt -> decrypt at m = 136
"""
import dataclasses
import os

import numpy as np
import pytest

from oracle import lolmath as lm
from params import PLAN_NAME, PRIME_OPS
from saturate import good_below
from test_encrypt import _small_key
from test_scalar_interp import _gpu_ops, _inputs, _oracle_ops, _params, _same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = bytes(range(32))
OPS = range(4, 10)                 # LOLHIP_OP_L ... LOLHIP_OP_DIVGDEC, in the order of PRIME_OPS


@pytest.fixture
def info(monkeypatch, capfd):
    """the launcher's lines since the last read, parsed: n, B, T, word, items, lds, grid, stages"""
    monkeypatch.setenv("LOLHIP_ZQ_SCAN_INFO", "1")

    def read():
        out = []
        for ln in capfd.readouterr().err.splitlines():
            if ln.startswith("k_zq_scan: "):
                head, stages = ln[len("k_zq_scan: "):].split(", stages ")
                f = {}
                for part in head.split(", "):
                    k, v = part.split(" ")[:2]
                    f[k] = int(v)
                f["stages"] = stages.split()
                out.append(f)
        return out
    return read


def _want_stages(m, op):
    """kind:p:d:rts:layout of the program of prime op `op`: one stage per odd prime, the stride the totient of the prime
    powers before it; lanes below a wave, cols from 64 on"""
    out, rts = [], 1
    for p, e in lm.factor_pps(m):
        if p != 2:
            out.append(f"{op}:{p}:{p - 1}:{rts}:{'cols' if rts >= 64 else 'lanes'}")
        rts *= (p - 1) * p ** (e - 1)
    return out


def _rows(R, rng, B=4):
    """_inputs and one more row: q - 1 at the last coefficient, zero elsewhere"""
    y, _ = _inputs(R, rng, B)
    last = np.zeros((1,) + y.shape[1:], dtype=np.int64)
    last[0, -1] = np.array(R.qs, dtype=np.int64) - 1
    return np.ascontiguousarray(np.concatenate([y, last]))


def _check(gpu, cpuref, info, m, qs, seed, B=4):
    """the six ops on an opted-in plan against the oracle and against the default plan; the stages from the launcher's lines"""
    pps = lm.factor_pps(m)
    P, D = gpu.Plan(pps, qs, scan_zq=True), gpu.Plan(pps, qs)
    R = _params(m, qs, P.has_crt)
    y = _rows(R, np.random.default_rng(seed), B)
    assert [P.scanRoute(op) for op in OPS] == [1] * 6 and [D.scanRoute(op) for op in OPS] == [0] * 6, (m, qs)
    info()
    got = _gpu_ops(P, y, y, ops=PRIME_OPS)
    lines = info()
    assert [ln["stages"] for ln in lines] == [_want_stages(m, op) for op in PRIME_OPS], (m, qs, lines[:2])
    assert all(ln["word"] == (4 if max(qs) < 2 ** 32 else 8) and ln["T"] == len(qs) and ln["n"] == R.n and ln["B"] == len(y)
               and ln["lds"] == ln["items"] * R.n * ln["word"] <= 64 * 1024 for ln in lines), (m, qs, lines[:2])
    assert all(v is not None for v in got.values())
    _same(got, _oracle_ops(cpuref, R, y, y, P.has_crt, ops=PRIME_OPS), (m, qs, "oracle"))
    ref = _gpu_ops(D, y, y, ops=PRIME_OPS)
    assert info() == [], "a default plan launched the scan kernel"
    _same(got, ref, (m, qs, "default plan"))
    return got


def _h(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _moduli_sets(m):
    g = lm.good_qs(m, 2 ** 30)
    return [[2], [16], [good_below(m, 2 ** 32)], [lm.first_good_q(m, 2 ** 32)], [good_below(m, 2 ** 61)], [good_below(m, 2 ** 62)],
            [next(g), next(g), next(g)], [good_below(m, 65280), lm.first_good_q(m, 2 ** 32)], [2 ** 20]]


# ---- vector length against the 64-lane round (prime index, stride 1) -------------------------------------------------------
@pytest.mark.parametrize("m", [17, 67, 257, 797])
def test_prime_indices_at_every_modulus_class(gpu, cpuref, info, m):
    for k, qs in enumerate(_moduli_sets(m) + ([[103]] if m == 17 else [])):
        _check(gpu, cpuref, info, m, qs, seed=m * 16 + k)


def test_sixteen_rounds(gpu, cpuref, info):
    _check(gpu, cpuref, info, 1021, [2 ** 20], seed=1021)
    _check(gpu, cpuref, info, 1021, [2 ** 61 - 1], seed=1022)          # a Mersenne prime: 8-byte words, 1021 invertible


# ---- strides -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [34, 136, 221, 323, 289, 2176, 4352])
def test_strides_and_layouts(gpu, cpuref, info, m):
    want = {34: ["lanes"], 136: ["lanes"], 221: ["lanes", "lanes"], 323: ["lanes", "lanes"], 289: ["lanes"], 2176: ["cols"], 4352: ["cols"]}[m]
    assert [s.split(":")[-1] for s in _want_stages(m, "l")] == want
    assert int(_want_stages(m, "l")[-1].split(":")[3]) == {34: 1, 136: 4, 221: 12, 323: 16, 289: 1, 2176: 64, 4352: 128}[m]
    for k, qs in enumerate(([good_below(m, 2 ** 32)], [good_below(m, 2 ** 61)], [lm.first_good_q(m, 2 ** 20), lm.first_good_q(m, 2 ** 40)],
                            [16])):
        _check(gpu, cpuref, info, m, qs, seed=m * 4 + k)


@pytest.mark.parametrize("m", [7 * 13, 45, 3 * 5 * 7 * 11])
def test_short_vectors_against_the_vector_interpreter(gpu, cpuref, info, m):
    """ZQ_SCAN: an opted-in plan takes the scan kernel at primes up to 13 too (d = 2 .. 12), where the default plan runs
    the vector interpreter (the scalar one over q = 8)"""
    assert gpu.Plan.for_index(m, [lm.first_good_q(m, 2 ** 20)], scan_zq=True).scanRoute(4) == 0
    gpu.debug_set("ZQ_SCAN", True)
    try:
        for k, qs in enumerate(([lm.first_good_q(m, 2 ** 20)], [lm.first_good_q(m, 2 ** 58)], [8])):
            _check(gpu, cpuref, info, m, qs, seed=m + k, B=6)
        P = gpu.Plan.for_index(m, [lm.first_good_q(m, 2 ** 20)], scan_zq=True)
        gpu.debug_set("GENERIC_SCALAR", True)                   # wins: no scan launch
        y = _rows(_params(m, P.qs), np.random.default_rng(m))
        info()
        forced = _gpu_ops(P, y, y, ops=PRIME_OPS)
        assert info() == []
        _same(forced, _oracle_ops(cpuref, _params(m, P.qs), y, y, True, ops=PRIME_OPS), (m, "GENERIC_SCALAR"))
    finally:
        gpu.debug_set("GENERIC_SCALAR", False)
        gpu.debug_set("ZQ_SCAN", False)


# ---- divG refuses before any launch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [17 * 7681, 34])
def test_a_modulus_divisible_by_17(gpu, cpuref, info, q):
    import torch
    m, B, SENT = 17, 5, 0x5A5A5A5A5A5A
    P, D, R = gpu.Plan.for_index(m, [q], scan_zq=True), gpu.Plan.for_index(m, [q]), _params(m, [q], False)
    assert not P.has_crt and [P.scanRoute(op) for op in OPS] == [1] * 6        # the route does not know divisibility
    y = _rows(R, np.random.default_rng(q), 4)[:B]
    buf = torch.full((B + 2, R.n, 1), SENT, dtype=torch.int64, device="cuda")
    buf[1:B + 1] = torch.from_numpy(y).cuda()
    before = buf.cpu().numpy().copy()
    info()
    assert P.divGPow(buf[1:B + 1]) is None and P.divGDec(buf[1:B + 1]) is None
    torch.cuda.synchronize()
    assert info() == [] and np.array_equal(buf.cpu().numpy(), before)
    assert P.divGPow(y) is None and P.divGDec(y) is None and info() == []
    four = ("l", "linv", "gpow", "gdec")
    got = _gpu_ops(P, y, y, ops=four)
    assert [ln["stages"] for ln in info()] == [_want_stages(m, op) for op in four]
    _same(got, _oracle_ops(cpuref, R, y, y, False, ops=four), (q, "oracle"))
    _same(got, _gpu_ops(D, y, y, ops=four), (q, "default plan"))
    assert info() == []


# ---- batch shapes ----------------------------------------------------------------------------------------------------------
def _tiles(ln):
    return -(-ln["B"] // ln["items"])


@pytest.mark.parametrize("m,lower", [(17, 2 ** 20), (257, 2 ** 58), (2176, 2 ** 20), (221, 2 ** 58)])
def test_batch_shapes_and_grid_stride(gpu, cpuref, info, monkeypatch, m, lower):
    import torch
    qs = [lm.first_good_q(m, lower), lm.first_good_q(m, 2 * lower)]
    P, R = gpu.Plan.for_index(m, qs, scan_zq=True), _params(m, qs)
    rng = np.random.default_rng(m)
    y = R.random(rng, 1)
    info()
    assert np.array_equal(P.divGDec(y), cpuref.ginvdec(R, y))
    (ln,) = info()
    assert ln["items"] == 1 and ln["grid"] == 2
    # a batch of at most 512 tiles takes the least tile: 1024 words
    items = -(-1024 // R.n)
    for B, grid in ((items + 1, None), (3 * items + 1, 2)):
        if grid:
            monkeypatch.setenv("LOLHIP_ZQ_SCAN_GRID", str(grid))
        y = R.random(rng, B)
        y[B - 1] = np.array(qs, dtype=np.int64) - 1
        for op in ("l", "ginvpow", "ginvdec", "gpow"):
            d = torch.from_numpy(y).cuda()
            getattr(P, PLAN_NAME[op])(d)
            torch.cuda.synchronize()
            (ln,) = info()
            assert ln["B"] == B and ln["items"] == items and _tiles(ln) == (4 if grid else 2)
            assert ln["grid"] == (grid or _tiles(ln) * 2)
            assert np.array_equal(d.cpu().numpy(), getattr(cpuref, op)(R, y)), (B, grid, op)
    monkeypatch.delenv("LOLHIP_ZQ_SCAN_GRID")


@pytest.mark.parametrize("m,lower", [(323, 2 ** 58), (257, 2 ** 20)])
def test_side_stream_between_guard_rows(gpu, cpuref, info, m, lower):
    import torch
    qs = [lm.first_good_q(m, lower)]
    P, R = gpu.Plan.for_index(m, qs, scan_zq=True), _params(m, qs)
    B, SENT = 37, 0x5A5A5A5A5A5A
    y = R.random(np.random.default_rng(m), B)
    buf = torch.full((B + 2, R.n, 1), SENT, dtype=torch.int64, device="cuda")
    buf[1:B + 1] = torch.from_numpy(y).cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    info()
    with torch.cuda.stream(st):
        P.l(buf[1:B + 1], stream=st.cuda_stream)
        P.divGDec(buf[1:B + 1], stream=st.cuda_stream)
        P.mulGPow(buf[1:B + 1], stream=st.cuda_stream)
    st.synchronize()
    assert len(info()) == 3
    out = buf.cpu().numpy()
    assert (out[0] == SENT).all() and (out[B + 1] == SENT).all()
    assert np.array_equal(out[1:B + 1], cpuref.gpow(R, cpuref.ginvdec(R, cpuref.l(R, y))))


# ---- what is composed on the prime ops -----------------------------------------------------------------------------------------
def test_rlwe_instances_then_valid_instances(gpu, info):
    m, q = 257, 9767
    assert (q - 1) % m == 0
    P = gpu.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True, scan_zq=True)
    D = gpu.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True)
    svar, I, L = 1.0 / m, 3, 4
    bound = gpu.RLWE.errorBound(m, svar, 2.0 ** -25, kind="disc")
    info()
    s, a, b = gpu.RLWE(P).instances("disc", I, L, svar=svar, key=KEY, ctr_s=3, ctr=50)
    fails, _ = gpu.RLWE(P).validInstances("disc", s, a, b, bound=bound)
    lines = info()
    assert lines, "no scan launch under RLWE"
    s0, a0, b0 = gpu.RLWE(D).instances("disc", I, L, svar=svar, key=KEY, ctr_s=3, ctr=50)
    fails0, _ = gpu.RLWE(D).validInstances("disc", s0, a0, b0, bound=bound)
    assert info() == []
    for x, x0 in ((s, s0), (a, a0), (b, b0), (fails, fails0)):
        assert np.array_equal(x.cpu().numpy(), x0.cpu().numpy())
    assert not fails.cpu().numpy().any()
    wrong, _ = gpu.RLWE(P).validInstances("disc", s.roll(1, 0), a, b, bound=bound)
    assert wrong.cpu().numpy().all()


def test_ring_rlwe_pair(gpu, info):
    import torch
    m, q, svar = 257, 2048, 1.0 / 257
    r = gpu.RingRLWE(gpu.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True, scan_zq=True))
    r0 = gpu.RingRLWE(gpu.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True))
    assert r.ring.plan_Q.scan_zq and r.ring.plan_Q.scanRoute(4) == 1 and not r0.ring.plan_Q.scan_zq
    info()
    _, shat = r.secret(key=KEY, ctr=0)
    a, b = r.sampleDisc(shat, 3, svar, key=KEY, ctr=10)
    bound = r.errorBound(m, svar, eps=2.0 ** -25, kind="disc")
    _, other = r.secret(key=KEY, ctr=1)
    ok, bad = r.validDisc(bound, shat, a, b), r.validDisc(bound, other, a, b)
    assert info(), "no scan launch under RingRLWE"
    _, shat0 = r0.secret(key=KEY, ctr=0)
    a0, b0 = r0.sampleDisc(shat0, 3, svar, key=KEY, ctr=10)
    ok0, bad0 = r0.validDisc(bound, shat0, a0, b0), r0.validDisc(bound, other, a0, b0)
    assert info() == []
    assert torch.equal(shat, shat0) and torch.equal(a, a0) and torch.equal(b, b0)
    assert np.array_equal(_h(ok), _h(ok0)) and np.array_equal(_h(bad), _h(bad0))
    assert _h(ok).all() and not _h(bad).any()


@pytest.mark.parametrize("which", ["plan", "ring"])
def test_challenges_generate_then_verify(gpu, info, tmp_path, which):
    """one line of a large-prime index on each route, cut to 2 instances of 3 samples"""
    from lol_amd import challenges as ch
    text = open(os.path.join(HERE, "golden", "challenge_params.txt")).read()
    recs = sorted((r for r in ch.parse_params(text, num_instances=2) if r.supported and ch.large_prime(r.m)), key=lambda r: r.m)
    pool = [r for r in recs if ((r.q - 1) % r.m == 0 and lm.is_prime(r.q)) == (which == "plan")]
    cp = dataclasses.replace(([r for r in pool if r.kind != "RLWR"] or pool)[0], numSamples=3)
    assert ch.route(cp)[0] == which and ch.route(cp)[1].scan_zq
    info()
    name = ch.generate(cp, str(tmp_path), KEY, beacon=(1478822400, 63), ctr_s=5, ctr=100)
    res = ch.verify(str(tmp_path), name)
    assert info(), "the challenge engine launched no scan kernel"
    assert sorted(res) == [0, 1] and all(ok and f == 0 for ok, f, _ in res.values()), res
    _, _, s, a, b, _ = ch.read_tree(str(tmp_path), name)
    ok, _ = ch.verify_arrays(cp, np.roll(s, 1, axis=0), a, b)
    assert not np.asarray(ok).any()


def test_encrypt_then_decrypt_over_a_small_plaintext_modulus(gpu, cpuref, info):
    """m = m' = 136, p = 8: LInv of the plaintext and L of the decryption over q <= 16 read a source that is not their
    output; divGDec over p under decrypt's k = 1"""
    import torch
    m, p, B, svar = 136, 8, 9, 1.0
    g = lm.good_qs(m, 2 ** 29)
    qs = [next(g), next(g)]
    rng = np.random.default_rng(136)
    pt = torch.from_numpy(rng.integers(-p + 1, p, size=(B, 64), dtype=np.int64)).cuda()
    s_crt = torch.from_numpy(_small_key(cpuref, m, qs, rng)).cuda()
    out = {}
    for scan in (True, False):
        # the error sampler at a prime above 13 needs the dense Gaussian stage, with and without the bit
        pq, pp = gpu.Plan.for_index(m, qs, dense_gauss=True, scan_zq=scan), gpu.Plan.for_index(m, [p], scan_zq=scan)
        assert pq.n == 64 and pp.scanRoute(9) == int(scan)
        info()
        ct = pq.encrypt(pt, s_crt, pp, svar, key=KEY, ctr=7)
        back = pq.decrypt(ct, s_crt, pp)
        div = pq.decrypt(ct, s_crt, pp, k=1)
        lines = info()
        assert bool(lines) == scan
        if scan:
            kinds = {st.split(":")[0] for ln in lines for st in ln["stages"]}
            assert {"l", "linv", "ginvdec"} <= kinds and {ln["word"] for ln in lines} == {4} and {ln["T"] for ln in lines} == {1, 2}
        assert torch.equal(back, pt % p)
        out[scan] = (ct, back, div)
    assert all(torch.equal(x, x0) for x, x0 in zip(out[True], out[False]))
