"""The dense Z_q stages at primes above 13 (zqdense.hip; plans created with dense_zq=True, LOLHIP_ROUTE_DENSE_ZQ), -m gpu.

Every case runs the same calls on an opted-in plan and on a default plan (the scalar interpreter k_generic, as before) and
compares both with the CPU oracle: `np.array_equal`, no tolerance anywhere in this file.  The launcher's line
(LOLHIP_ZQ_DENSE_INFO, read at every launch) says which route ran, with how many limbs, how each stage ran, the tile and
the grid; every case asserts it, and that the default plan prints none.

    depth and row padding   primes 17 .. 797: d = 16 .. 796 against the 32-deep unit and the 32-row tile of the matrix cores
    moduli                  the largest prime of each limb count W = 2, 3, 4 and the first above it, the top of the 4-byte
                            words, the first 8-byte modulus, the tops below 2^61 and 2^62, a three-modulus tuple, a narrow /
                            wide pair (one wide modulus sends the whole plan to the vector ALU with 8-byte words)
    inputs                  test_scalar_interp._inputs plus rows of floor(q/2) and floor(q/2) + 1: the centred extremes,
                            which saturate the limbs
    program shapes          element-wise stages before a dense one, two and three dense stages ping-ponging, DFT_p with its
                            twiddle in the write-back, merged 6-/8-/18-/20-vectors beside 17, staged CRT_4, the split route's odd
                            part; strides below and above a wave on both routes
    batches                 B = 1, one more than a tile, three tiles + 1 on a grid of 2, a side stream between guard rows
    composed                RLWE instances, RingRLWE, challenges generate -> verify
"""
import dataclasses
import os

import numpy as np
import pytest

from oracle import lolmath as lm
from saturate import good_below
from test_scalar_interp import _gpu_ops, _inputs, _oracle_ops, _params, _same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = bytes(range(32))
W_TOPS = (65279, 16711423, 4278124287)
MFMA_MIN_D = 48


@pytest.fixture
def info(monkeypatch, capfd):
    """the launcher's lines since the last read, parsed: route, W, word, items, grid, B, stages"""
    monkeypatch.setenv("LOLHIP_ZQ_DENSE_INFO", "1")

    def read():
        out = []
        for ln in capfd.readouterr().err.splitlines():
            if ln.startswith("k_zq_dense: "):
                head, stages = ln[len("k_zq_dense: "):].split(", stages ")
                f = {}
                for part in head.split(", "):
                    k, v = part.split(" ")[:2]
                    f[k] = int(v)
                f["stages"] = stages.split()
                out.append(f)
        return out
    return read


def _limbs(q):
    w = 2
    while q // 2 > 127 * (256 ** w - 1) // 255:
        w += 1
    return w if w <= 4 else None


def _want_kinds(P, inverse):
    return ["elt" if not (st[0] in (1, 2, 3) and st[1] > 13) else ("dense-cols" if st[3] >= 64 else "dense-rows")
            for st in P.program(inverse)]


def _want_route(P):
    """the documented rule, from the program and the moduli"""
    d = [int(st[2]) for inv in (False, True) for st in P.program(inv) if st[0] in (1, 2, 3) and st[1] > 13]
    if not d or P.n > 8192:
        return 0, 0
    if all(_limbs(q) for q in P.qs) and max(d) >= MFMA_MIN_D:
        return 2, max(_limbs(q) for q in P.qs)
    return 1, 0


def _want_polymul(P):
    """the poly-mul in one launch (on the transforms' route) when the stage programs alone make the transform, 4 n words
    fit 152 KiB of LDS and the tile is not too small for the inverse program; else 0: composed of lone transforms"""
    if P.pps[0][0] == 2 and P.pps[0][1] >= 5:
        return 0
    word, route = (4 if max(P.qs) < 2 ** 32 else 8), _want_route(P)[0]
    if not route or 4 * P.n * word > 152 * 1024:
        return 0
    dmax = max(int(st[2]) for inv in (False, True) for st in P.program(inv) if st[0] in (1, 2, 3) and st[1] > 13)
    # a 64 KiB tile must leave the inverse program, which runs on half of it, a whole register tile of columns
    cols = max(1, 64 * 1024 // (4 * P.n * word)) * (P.n // dmax)
    return route if cols >= (32 if route == 2 else 8 if word == 4 else 4) else 0


def _extremes(y, qs):
    """two more rows: floor(q/2) and floor(q/2) + 1 everywhere"""
    qv = np.array(qs, dtype=np.int64)
    ext = np.empty((2,) + y.shape[1:], dtype=np.int64)
    ext[0], ext[1] = qv // 2, qv // 2 + 1
    return np.ascontiguousarray(np.concatenate([y, ext]))


def _check(gpu, cpuref, info, m, qs, seed, route=None):
    """every op on an opted-in plan against the oracle and against the default plan; the routes from the launcher's lines"""
    pps = lm.factor_pps(m)
    P, D, R = gpu.Plan(pps, qs, dense_zq=True), gpu.Plan(pps, qs), _params(m, qs)
    y, z = _inputs(R, np.random.default_rng(seed))
    y, z = _extremes(y, qs), _extremes(z, qs)
    want_route, want_W = _want_route(P)
    assert want_route >= 1 and [P.zqRoute(w) for w in range(3)] == [want_route, want_route, _want_polymul(P)], (m, qs)
    assert route is None or route == want_route, (m, qs)
    info()
    got = _gpu_ops(P, y, z)
    lines = info()
    kinds = {tuple(_want_kinds(P, inv)) for inv in (False, True)}
    fused = tuple(_want_kinds(P, False) + ["*"] + _want_kinds(P, True))
    assert lines and all(ln["route"] == want_route and ln["W"] == want_W for ln in lines), (m, qs, lines[:3])
    assert all(tuple(ln["stages"]) == fused if ln["polymul"] else tuple(ln["stages"]) in kinds for ln in lines), (m, qs, lines[:3])
    # _gpu_ops multiplies four times (c apart, c = a, c = b, the square): four launches in all, or none of this kind
    assert sum(ln["polymul"] for ln in lines) == (4 if _want_polymul(P) else 0), (m, qs)
    assert all(ln["word"] == (4 if max(qs) < 2 ** 32 else 8) and ln["T"] == len(qs) and ln["lds"] <= 152 * 1024 for ln in lines)
    _same(got, _oracle_ops(cpuref, R, y, z), (m, qs, "oracle"))
    ref = _gpu_ops(D, y, z)
    assert info() == [], "a default plan launched the dense kernels"
    _same(got, ref, (m, qs, "default plan"))
    return got


def _moduli_sets(m):
    g = lm.good_qs(m, 2 ** 30)
    sets = []
    for top in W_TOPS:
        sets += [[good_below(m, top + 1)], [lm.first_good_q(m, top)]]
    return sets + [[good_below(m, 2 ** 32)], [lm.first_good_q(m, 2 ** 32)], [good_below(m, 2 ** 61)], [good_below(m, 2 ** 62)],
                   [next(g), next(g), next(g)], [good_below(m, 65280), lm.first_good_q(m, 2 ** 32)]]


# d = 16, 18, 30, 36, 66, 96, 178, 256, 796: below one 32-deep unit, astride 32 and 64, at exact multiples, the list's own
@pytest.mark.parametrize("k", range(12))
@pytest.mark.parametrize("m", [17, 19, 31, 37, 67, 97, 179, 257, 797])
def test_prime_indices_at_every_modulus_class(gpu, cpuref, info, m, k):
    qs = _moduli_sets(m)[k]
    # the matrix cores exactly where every modulus fits four limbs and the vector is long enough
    _check(gpu, cpuref, info, m, qs, seed=m * 16 + k, route=2 if (m - 1 >= MFMA_MIN_D and k not in (5, 6, 7, 8, 9, 11)) else 1)


# 51, 221: an element-wise stage, then dense at rts = 2 and 12.  323, 7429: two and three dense stages (n = 6336).
# 289, 4913: DFT_17 (d = 17) with its twiddle.  68: staged CRT_4 first.  544, 2^9 17: the split route's odd part, rts = 16 and
# 256.  335, 4489, 2^6 67, 2^7 67: the same shapes at d = 66 / 67, where the matrix cores take them: rts = 4, a DFT_67 with
# its twiddle (67 rows padded to 96), rts = 32 and 64 (both lane layouts of the data operand)
@pytest.mark.parametrize("m", [51, 221, 323, 7429, 289, 4913, 68, 544, 2 ** 9 * 17, 335, 4489, 2 ** 6 * 67, 2 ** 7 * 67])
def test_program_shapes(gpu, cpuref, info, m):
    g = lm.good_qs(m, 2 ** 30)
    for k, qs in enumerate(([lm.first_good_q(m, 2 ** 20)], [lm.first_good_q(m, 2 ** 58)], [next(g), next(g), next(g)])):
        _check(gpu, cpuref, info, m, qs, seed=m + k, route=(2 if m % 67 == 0 and k != 1 else 1))


@pytest.mark.parametrize("m", [153, 459, 425, 255])
def test_merged_vectors_beside_17(gpu, cpuref, info, m):
    """class-2 moduli: 3^2, 3^3, 5^2 and 3 (x) 5 as one dense 6-, 18-, 20- and 8-vector stage, element-wise on the tile"""
    q26 = lm.first_good_q(m, 2 ** 26)
    P = gpu.Plan.for_index(m, [q26], host_only=True, dense_zq=True)
    assert {6: 153, 18: 459, 20: 425, 8: 255}[max(int(st[2]) for st in P.program() if st[1] <= 13)] == m
    _check(gpu, cpuref, info, m, [q26], seed=m)
    _check(gpu, cpuref, info, m, [q26, lm.first_good_q(m, q26)], seed=m + 1)


# ---- batch shapes ----------------------------------------------------------------------------------------------------------
def _tiles(ln):
    return -(-ln["B"] // ln["items"])


@pytest.mark.parametrize("m,lower", [(17, 2 ** 20), (17, 2 ** 58), (257, 2 ** 20), (257, 2 ** 58), (2 ** 7 * 67, 2 ** 20), (2 ** 9 * 17, 2 ** 20)])
def test_batch_shapes_and_grid_stride(gpu, cpuref, info, monkeypatch, m, lower):
    import torch
    qs = [lm.first_good_q(m, lower), lm.first_good_q(m, 2 * lower)]
    pps = lm.factor_pps(m)
    P, R = gpu.Plan(pps, qs, dense_zq=True), _params(m, qs)
    rng = np.random.default_rng(m)
    # B = 1, then a batch that fills the launcher's tile: its size is the line's
    y = R.random(rng, 1)
    info()
    assert np.array_equal(P.crt(y), cpuref.crt(R, y))
    (ln,) = info()
    assert ln["items"] == 1 and ln["grid"] == 2
    y = R.random(rng, 64)
    assert np.array_equal(P.crtInv(y), cpuref.crtinv(R, y))
    (ln,) = info()
    items = ln["items"]
    assert items < 64
    for B, grid in ((items + 1, None), (3 * items + 1, 2)):
        if grid:
            monkeypatch.setenv("LOLHIP_ZQ_DENSE_GRID", str(grid))
        y = R.random(rng, B)
        y[B - 1] = np.array(qs, dtype=np.int64) // 2 + 1
        d = torch.from_numpy(y).cuda()
        P.crt(d)
        torch.cuda.synchronize()
        (ln,) = info()
        # the same tile as for 64 items (the launcher sizes it by the batch only beyond 512 tiles): exactly 2 and 4 tiles
        assert ln["B"] == B and ln["items"] == items and _tiles(ln) == (4 if grid else 2)
        assert ln["grid"] == (grid or _tiles(ln) * 2)
        assert np.array_equal(d.cpu().numpy(), cpuref.crt(R, y)), (B, grid)
    monkeypatch.delenv("LOLHIP_ZQ_DENSE_GRID")


@pytest.mark.parametrize("m,lower", [(19, 2 ** 58), (257, 2 ** 20)])
def test_side_stream_between_guard_rows(gpu, cpuref, info, m, lower):
    import torch
    qs = [lm.first_good_q(m, lower)]
    P, R = gpu.Plan.for_index(m, qs, dense_zq=True), _params(m, qs)
    B, SENT = 37, 0x5A5A5A5A5A5A
    y = R.random(np.random.default_rng(m), B)
    buf = torch.full((B + 2, R.n, 1), SENT, dtype=torch.int64, device="cuda")
    buf[1:B + 1] = torch.from_numpy(y).cuda()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    info()
    with torch.cuda.stream(st):
        P.crt(buf[1:B + 1], stream=st.cuda_stream)
        P.crtInv(buf[1:B + 1], stream=st.cuda_stream)
        P.crt(buf[1:B + 1], stream=st.cuda_stream)
    st.synchronize()
    assert len(info()) == 3
    out = buf.cpu().numpy()
    assert (out[0] == SENT).all() and (out[B + 1] == SENT).all()
    assert np.array_equal(out[1:B + 1], cpuref.crt(R, y))


# ---- route parity ------------------------------------------------------------------------------------------------------------
def _forced(gpu, name, P, y, z, route):
    gpu.debug_set(name, True)
    try:
        assert P.zqRoute(0) == P.zqRoute(1) == route
        return _gpu_ops(P, y, z)
    finally:
        gpu.debug_set(name, False)


# the matrix cores forced on every shape the vector ALU takes by default (ZQ_DENSE_MFMA): d = 16, 18, 30, 36 against the
# 32-deep unit and the 32-row tile, DFT_17 with its twiddle, strides 2, 12, 16 and 256, two and three dense stages; and
# the vector ALU forced where the matrix cores are the default (ZQ_DENSE_VALU); the scalar interpreter on the same plan
@pytest.mark.parametrize("m", [17, 19, 31, 37, 257, 51, 221, 289, 323, 7429, 544, 2 ** 9 * 17, 4489])
def test_forced_routes_equal_the_default_of_the_plan(gpu, cpuref, info, m):
    for k, qs in enumerate(([lm.first_good_q(m, 1000)], [lm.first_good_q(m, 2 ** 20), good_below(m, W_TOPS[2] + 1)])):
        P, R = gpu.Plan.for_index(m, qs, dense_zq=True), _params(m, qs)
        y, z = _inputs(R, np.random.default_rng(m + k))
        y, z = _extremes(y, qs), _extremes(z, qs)
        route, W = _want_route(P)[0], max(_limbs(q) for q in qs)
        info()
        default = _gpu_ops(P, y, z)
        assert {ln["route"] for ln in info()} == {route}
        _same(default, _oracle_ops(cpuref, R, y, z), (m, qs, "oracle"))
        valu = _forced(gpu, "ZQ_DENSE_VALU", P, y, z, 1)
        assert {(ln["route"], ln["W"]) for ln in info()} == {(1, 0)}
        _same(valu, default, (m, qs, "ZQ_DENSE_VALU against the plan's default"))
        mfma = _forced(gpu, "ZQ_DENSE_MFMA", P, y, z, 2)
        assert {(ln["route"], ln["W"]) for ln in info()} == {(2, W)}
        _same(mfma, default, (m, qs, "ZQ_DENSE_MFMA against the plan's default"))
        scalar = _forced(gpu, "GENERIC_SCALAR", P, y, z, 0)
        assert info() == []
        _same(scalar, default, (m, qs, "GENERIC_SCALAR against the plan's default"))


# ---- what is composed on the transforms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,q", [(23, 47), (257, 9767)])
def test_rlwe_instances_then_valid_instances(gpu, info, m, q):
    assert (q - 1) % m == 0
    P = gpu.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True)
    D = gpu.Plan.for_index(m, [q], dense_gauss=True)
    svar, I, L = 1.0 / m, 3, 4
    bound = gpu.RLWE.errorBound(m, svar, 2.0 ** -25, kind="disc")
    info()
    s, a, b = gpu.RLWE(P).instances("disc", I, L, svar=svar, key=KEY, ctr_s=3, ctr=50)
    fails, _ = gpu.RLWE(P).validInstances("disc", s, a, b, bound=bound)
    lines = info()
    assert lines and {ln["route"] for ln in lines} == {_want_route(P)[0]}
    s0, a0, b0 = gpu.RLWE(D).instances("disc", I, L, svar=svar, key=KEY, ctr_s=3, ctr=50)
    fails0, _ = gpu.RLWE(D).validInstances("disc", s0, a0, b0, bound=bound)
    assert info() == []
    for x, x0 in ((s, s0), (a, a0), (b, b0), (fails, fails0)):
        assert np.array_equal(x.cpu().numpy(), x0.cpu().numpy())
    assert not fails.cpu().numpy().any()
    wrong, _ = gpu.RLWE(P).validInstances("disc", s.roll(1, 0), a, b, bound=bound)
    assert wrong.cpu().numpy().all()


def test_ring_rlwe_on_line_287_with_dense_zq(gpu, info):
    import rlwe_ring_ref as rg
    import torch
    m, q, svar = 179, 2048, 5.6179775280898875e-3
    assert rg.challenge_lines()[287] == ("Disc", m, q, svar)
    r = gpu.RingRLWE(gpu.Plan.for_index(m, [q], dense_gauss=True, dense_zq=True))
    r0 = gpu.RingRLWE(gpu.Plan.for_index(m, [q], dense_gauss=True))
    assert r.ring.plan_Q.dense_zq and r.ring.plan_Q.zqRoute(0) >= 1 and not r0.ring.plan_Q.dense_zq
    assert gpu.RingMul(r.plan, dense_zq=False).plan_Q.zqRoute(0) == 0
    info()
    _, shat = r.secret(key=KEY, ctr=0)
    a, b = r.sampleDisc(shat, 3, svar, key=KEY, ctr=10)
    assert info(), "no dense launch under RingRLWE"
    _, shat0 = r0.secret(key=KEY, ctr=0)
    a0, b0 = r0.sampleDisc(shat0, 3, svar, key=KEY, ctr=10)
    assert info() == []
    assert torch.equal(shat, shat0) and torch.equal(a, a0) and torch.equal(b, b0)
    bound = r.errorBound(m, svar, eps=2.0 ** -25, kind="disc")
    _, other = r.secret(key=KEY, ctr=1)
    assert r.validDisc(bound, shat, a, b).all() and not r.validDisc(bound, other, a, b).any()


@pytest.mark.parametrize("m", [179, 797])
def test_challenges_generate_then_verify(gpu, info, tmp_path, m):
    """one line of the index with a CRT basis where the list has one, cut to 2 instances of 3 samples"""
    from lol_amd import challenges as ch
    text = open(os.path.join(HERE, "golden", "challenge_params.txt")).read()
    recs = [r for r in ch.parse_params(text, num_instances=2) if r.m == m and r.supported]
    with_crt = [r for r in recs if (r.q - 1) % m == 0 and lm.is_prime(r.q)]
    pool = with_crt or recs
    cp = dataclasses.replace(([r for r in pool if r.kind != "RLWR"] or pool)[0], numSamples=3)
    assert ch.large_prime(cp.m)
    info()
    name = ch.generate(cp, str(tmp_path), KEY, beacon=(1478822400, 63), ctr_s=5, ctr=100)
    res = ch.verify(str(tmp_path), name)
    assert info(), "the challenge engine launched no dense kernel"
    assert sorted(res) == [0, 1] and all(ok and f == 0 for ok, f, _ in res.values()), res
    _, _, s, a, b, _ = ch.read_tree(str(tmp_path), name)
    ok, _ = ch.verify_arrays(cp, np.roll(s, 1, axis=0), a, b)
    assert not np.asarray(ok).any()


def test_default_plan_at_17_launches_the_scalar_interpreter(gpu, cpuref, info):
    m, qs = 17, [lm.first_good_q(17, 2 ** 20)]
    D, R = gpu.Plan.for_index(m, qs), _params(m, qs)
    y, z = _inputs(R, np.random.default_rng(17))
    assert [D.zqRoute(w) for w in range(3)] == [0, 0, 0]
    info()
    _same(_gpu_ops(D, y, z), _oracle_ops(cpuref, R, y, z), "default plan")
    assert info() == []
