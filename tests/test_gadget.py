"""Gadget error correction on the device (k_gadget_correct, k_gadget_encode; Plan.gadgetCorrect / gadgetEncode) against
the big-integer restatement tests/gadget_ref.py, bit for bit in u and every e_j.  Shapes: m = 32 (n = 16) with B = 33
and m = 45 (n = 24) with B = 22, both 528 rows: one full 512-row tile and a ragged second one."""
import random

import numpy as np
import pytest

import gadget_ref as gr
from oracle import lolmath as lm

pytestmark = pytest.mark.gpu

Q60 = 2 ** 60 + 147457
Q30 = 1073479681
PAIR = [12289, 7681]
SHAPES = {32: 33, 45: 22}
# (m, moduli, base): every (q, b) of the host list at m = 32, the one modulus with the index 45 there too, the pair at
# bases 0, 2, 16 and TrivGad over one modulus
CASES = [(32, [257], 2), (32, [257], 3), (32, [12289], 4), (32, [12289], 256), (32, [Q30], 2), (45, [Q30], 2),
         (32, [Q60], 2), (32, [Q60], 256), (32, [7681], 7681), (32, [7681], 10000), (32, PAIR, 0), (32, PAIR, 2),
         (45, PAIR, 2), (32, PAIR, 16), (32, [12289], 0)]
_ids = lambda c: f"m{c[0]}-q{'x'.join(map(str, c[1]))}-b{c[2]}"
_plans = {}


def _plan(gpu, m, qs):
    key = (m, tuple(qs))
    if key not in _plans:
        _plans[key] = gpu.Plan(lm.factor_pps(m), list(qs))
    return _plans[key]


def _i64(a):
    return np.array(a, dtype=object).astype(np.int64)


def _ref(base, qs, xs):
    """the restatement over a slab xs [L][B][n][T] -> u [B][n][T], es [L][B][n] as int64"""
    L, B, n, T = xs.shape
    u, es = gr.correct(base, qs, xs.reshape(L, B * n, T))
    return _i64(u).reshape(B, n, T), _i64(es).reshape(L, B, n)


def _residues(rng, qs, shape):
    return np.stack([rng.integers(0, q, size=shape, dtype=np.int64) for q in qs], axis=-1)


def _check(plan, base, qs, xs, **kw):
    u, es = plan.gadgetCorrect(xs, base, **kw)
    wu, wes = _ref(base, qs, xs)
    assert np.array_equal(u, wu)
    assert np.array_equal(es, wes)
    return u, es


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_valid_noisy_encodings(gpu, case):
    m, qs, base = case
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    n, T = plan.n, plan.T
    rng = np.random.default_rng(hash((m, tuple(qs), base)) % 2 ** 32)
    g = plan.gadget(base)
    assert g.tolist() == gr.gadget(base, qs)
    L = len(g)
    s = _residues(rng, qs, (B, n))
    cap = 0 if base == 0 else max(gr.error_cap(base, min(qs)), 0)
    if min(gr.digits(base, q) for q in qs) == 1:
        cap = 0                                               # a one-entry block carries no redundancy: e = [0]
    e = rng.integers(-cap, cap + 1, size=(L, B, n), dtype=np.int64)
    e[:, : B // 2] = np.where(e[:, : B // 2] < 0, -cap, cap)   # half of the rows exactly at the cap
    enc = plan.gadgetEncode(s, base, e)
    want = np.array([[(int(g[j, t]) * s[..., t].astype(object) + e[j].astype(object)) % qs[t] for t in range(T)]
                     for j in range(L)], dtype=object)          # [L][T][B][n]
    assert np.array_equal(enc, _i64(np.moveaxis(want, 1, -1)))
    assert np.array_equal(enc, _i64(gr.encode(base, qs, s.reshape(-1, T), e.reshape(L, -1))).reshape(L, B, n, T))
    assert np.array_equal(plan.gadgetEncode(s, base), _i64(gr.encode(base, qs, s.reshape(-1, T))).reshape(L, B, n, T))
    u, es = _check(plan, base, qs, enc)
    assert np.array_equal(u, s)
    if not (base == 0 and T == 2):                            # TrivGad over a pair defines u alone
        assert np.array_equal(es, e)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_arbitrary_inputs(gpu, case):
    """uniformly random residues, encodings of nothing: the function is defined for every input"""
    m, qs, base = case
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    rng = np.random.default_rng(hash((m, tuple(qs), base, 1)) % 2 ** 32)
    xs = _residues(rng, qs, (plan.decomposeLen(base), B, plan.n))
    _check(plan, base, qs, xs)


def _boundary_rows(q, b, rows, rng):
    """rows [rows][k] of residues at the rounding boundaries of both divisions and with the special residues in every
    position; returns the rows and how many of each kind were built"""
    k, h, g = gr.gadlen(b, q), q // 2, b ** (gr.gadlen(b, q) - 1)
    special = [0, q - 1, h, h + 1, h - 1]
    out, kinds = [], {"w0": 0, "wq": 0, "s0": 0, "sg": 0, "special": 0}
    rnd = lambda: [rng.randrange(q) for _ in range(k)]
    for i in range(k - 1):                                    # (b v_i - v_(i+1) + h) mod q = 0 and q - 1
        for target, kind in ((0, "w0"), (q - 1, "wq")):
            row = rnd()
            row[i + 1] = (b * gr.lift(row[i], q) + h - target) % q
            assert (b * gr.lift(row[i], q) - gr.lift(row[i + 1], q) + h) % q == target
            out.append(row)
            kinds[kind] += 1
    for target, kind in ((0, "s0"), (g - 1, "sg")):           # (v'_(k-1) + floor(g/2)) mod g = 0 and g - 1
        found = 0
        for _ in range(400):
            row, tr = rnd(), {}
            gr.correct1(b, q, row, tr)
            delta = (target - (tr["vp"][-1] + g // 2)) % g
            for d in (delta, delta - g):
                cand = row[:-1] + [(row[-1] + d) % q]
                if gr.lift(cand[-1], q) != gr.lift(row[-1], q) + d:
                    continue                                  # left the lift's range
                tr2 = {}
                gr.correct1(b, q, cand, tr2)
                if (tr2["vp"][-1] + g // 2) % g == target:
                    out.append(cand)
                    found += 1
                    break
            if found == 4:
                break
        assert found, (q, b, kind)
        kinds[kind] += found
    for i in range(k):                                        # 0, q-1, floor(q/2), floor(q/2) +- 1 in every position
        for v in special:
            row = rnd()
            row[i] = v
            out.append(row)
            kinds["special"] += 1
    out += [[v] * k for v in special]
    assert len(out) <= rows
    while len(out) < rows:
        out.append([rng.choice(special + [rng.randrange(q)]) for _ in range(k)])
    return out, kinds


@pytest.mark.parametrize("q,b", [(257, 3), (12289, 4), (Q60, 2), (Q60, 256), (256, 2)])
def test_rounding_boundaries(gpu, q, b):
    plan, B = _plan(gpu, 32, [q]), SHAPES[32]
    rows, kinds = _boundary_rows(q, b, B * plan.n, random.Random(q + b))
    print(q, b, kinds)
    assert all(kinds.values())
    k = gr.gadlen(b, q)
    xs = _i64(rows).T.reshape(k, B, plan.n, 1)                 # [rows][k] -> [k][B][n][1]
    _check(plan, b, [q], np.ascontiguousarray(xs))


def test_rounding_boundaries_pair(gpu):
    """the same boundary rows in each block of the pair, mapped back through the pair's change of entry"""
    qa, qb = PAIR
    plan, B = _plan(gpu, 32, PAIR), SHAPES[32]
    rows, base = B * plan.n, 2
    rng = random.Random(5)
    ra, _ = _boundary_rows(qa, base, rows, rng)
    rb, _ = _boundary_rows(qb, base, rows, rng)
    ka, kb = gr.gadlen(base, qa), gr.gadlen(base, qb)
    xs = np.zeros((ka + kb, rows, 2), dtype=np.int64)
    for r in range(rows):
        for i in range(ka):                                   # entry = q_b^-1 (a - lift beta): a = q_b entry + lift beta
            beta = rng.randrange(qb)
            xs[i, r] = ((qb * ra[r][i] + gr.lift(beta, qb)) % qa, beta)
        for i in range(kb):
            a = rng.randrange(qa)
            xs[ka + i, r] = (a, (qa * rb[r][i] + gr.lift(a, qa)) % qb)
    _check(plan, base, PAIR, xs.reshape(ka + kb, B, plan.n, 2))


@pytest.mark.parametrize("m,qs,base", [(45, [Q30], 2), (45, [Q30], 256), (32, PAIR, 16)], ids=lambda v: str(v))
def test_powerful_and_crt_bases(gpu, m, qs, base):
    import torch
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    assert plan.has_crt
    rng = np.random.default_rng(m + base)
    L = plan.decomposeLen(base)
    xs = torch.from_numpy(_residues(rng, qs, (L, B, plan.n))).cuda()
    dec = xs.clone()
    plan.lInv(dec)                                            # pow -> dec over the L B polynomials
    want = plan.gadgetCorrect(dec, base)
    got = plan.gadgetCorrect(xs, base, basis="pow")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    dec = xs.clone()
    plan.crtInv(dec)
    plan.lInv(dec)
    want = plan.gadgetCorrect(dec, base)
    got = plan.gadgetCorrect(xs, base, basis="crt")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    wu, wes = _ref(base, qs, dec.cpu().numpy())
    assert np.array_equal(got[0].cpu().numpy(), wu) and np.array_equal(got[1].cpu().numpy(), wes)


@pytest.mark.parametrize("m,qs,base", [(45, [Q30], 2), (32, PAIR, 16)], ids=lambda v: str(v))
def test_round_trip_through_the_crt_basis(gpu, m, qs, base):
    """s encoded in the CRT basis, noise from the decoding basis: correct recovers the noise, and u pushed through l and
    crt is the s that was encoded"""
    import torch
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    n, T = plan.n, plan.T
    rng = np.random.default_rng(7 * m + base)
    L = plan.decomposeLen(base)
    # the cap bounds the decoding-basis coefficient of every entry's error
    cap = gr.error_cap(base, min(qs))
    s_crt = torch.from_numpy(_residues(rng, qs, (B, n))).cuda()
    e = rng.integers(-cap, cap + 1, size=(L, B, n), dtype=np.int64)
    noise = torch.from_numpy(np.stack([e % q for q in qs], axis=-1)).cuda()
    plan.l(noise)
    plan.crt(noise)
    q_t = torch.tensor(qs, dtype=torch.int64, device="cuda")
    xs = (plan.gadgetEncode(s_crt, base) + noise) % q_t
    u, es = plan.gadgetCorrect(xs.contiguous(), base, basis="crt")
    assert np.array_equal(es.cpu().numpy(), e)
    plan.l(u)
    plan.crt(u)
    assert torch.equal(u, s_crt)


@pytest.mark.parametrize("m,qs,base", [(32, [Q60], 2), (32, [12289], 4), (45, PAIR, 2)], ids=lambda v: str(v))
def test_non_canonical_inputs_are_taken_mod_q(gpu, m, qs, base):
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    rng = np.random.default_rng(11 * m + base)
    L = plan.decomposeLen(base)
    xs = _residues(rng, qs, (L, B, plan.n))
    shift = rng.integers(-4, 4, size=xs.shape, dtype=np.int64) * np.array(qs, dtype=np.int64)     # |.| <= 4 q < 2^63
    assert (shift < 0).any() and (xs + shift >= np.array(qs)).any()
    want = _check(plan, base, qs, xs)
    got = plan.gadgetCorrect(xs + shift, base)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    s = _residues(rng, qs, (B, plan.n))
    e = rng.integers(-2 ** 62, 2 ** 62, size=(L, B, plan.n), dtype=np.int64)                       # any int64 reduces
    assert np.array_equal(plan.gadgetEncode(s + shift[0], base, e),
                          _i64(gr.encode(base, qs, s.reshape(-1, plan.T), e.reshape(L, -1))).reshape(xs.shape))


@pytest.mark.parametrize("m,qs,base", [(32, [Q60], 256), (32, PAIR, 2)], ids=lambda v: str(v))
def test_without_errors_u_is_unchanged(gpu, m, qs, base):
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    xs = _residues(np.random.default_rng(3), qs, (plan.decomposeLen(base), B, plan.n))
    u, es = plan.gadgetCorrect(xs, base)
    u2, none = plan.gadgetCorrect(xs, base, errors=False)
    assert none is None and np.array_equal(u, u2)


GUARD = 0x5A5A5A5A5A5A5A5A


def _raw_correct(gpu, plan, xs, base, basis, stream=None, misalign=False, errors=True):
    """the C entry on buffers with guard words around u, es and work; xs one word off 16-byte alignment on request"""
    import torch
    L, B = xs.shape[0], xs.shape[1]
    n, T = plan.n, plan.T
    wl = plan.gadgetCorrectWorkLen(base, basis, B)
    dev = "cuda"
    xbuf = torch.empty(xs.size + 2, dtype=torch.int64, device=dev)
    off = 1 if misalign else 0
    assert xbuf.data_ptr() % 16 == 0
    xin = xbuf[off:off + xs.size]
    xin.copy_(torch.from_numpy(np.ascontiguousarray(xs)).reshape(-1))
    bufs = {}
    for nm, words in (("u", B * n * T), ("es", L * B * n), ("work", wl)):
        bufs[nm] = torch.full((words + 4,), GUARD, dtype=torch.int64, device=dev)
    st = 0 if stream is None else stream.cuda_stream
    torch.cuda.synchronize()                                  # the fills above ran on the current stream
    ptr = lambda t: t.data_ptr() + 16
    rc = gpu.lib().lolhip_gadget_correct_batch(plan._h, st, xin.data_ptr(), base, {"dec": 0, "pow": 1, "crt": 2}[basis],
                                               ptr(bufs["u"]), ptr(bufs["es"]) if errors else None,
                                               ptr(bufs["work"]) if wl else None, B)
    assert rc == 0
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    for nm, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all(), nm
    u = bufs["u"][2:-2].cpu().numpy().reshape(B, n, T)
    es = bufs["es"][2:-2].cpu().numpy().reshape(L, B, n)
    if not errors:
        assert (es == GUARD).all()
    return u, es


@pytest.mark.parametrize("m,qs,base,basis", [(32, PAIR, 2, "dec"), (45, PAIR, 16, "pow"), (32, PAIR, 0, "crt"),
                                             (45, [Q30], 256, "crt"), (32, [Q60], 2, "dec")], ids=lambda v: str(v))
def test_launch_variants(gpu, m, qs, base, basis):
    """guard words, the 8-byte route of a misaligned pair slab, a side stream, B = 1, es = NULL"""
    import torch
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    rng = np.random.default_rng(13 * m + base)
    L = plan.decomposeLen(base)
    xs = _residues(rng, qs, (L, B, plan.n))
    want = plan.gadgetCorrect(xs, base, basis=basis)
    if basis == "dec":
        wu, wes = _ref(base, qs, xs)
        assert np.array_equal(want[0], wu) and np.array_equal(want[1], wes)
    side = torch.cuda.Stream()
    for kw in (dict(), dict(misalign=True), dict(stream=side), dict(misalign=True, stream=side)):
        u, es = _raw_correct(gpu, plan, xs, base, basis, **kw)
        assert np.array_equal(u, want[0]) and np.array_equal(es, want[1]), kw
    u, _ = _raw_correct(gpu, plan, xs, base, basis, errors=False)
    assert np.array_equal(u, want[0])
    one = np.ascontiguousarray(xs[:, 5:6])
    u, es = _raw_correct(gpu, plan, one, base, basis)
    assert np.array_equal(u, want[0][5:6]) and np.array_equal(es, want[1][:, 5:6])
    with torch.cuda.stream(side):
        got = plan.gadgetCorrect(torch.from_numpy(xs).cuda(), base, basis=basis, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    # B = 0 is a no-op on a plan with a device
    assert gpu.lib().lolhip_gadget_correct_batch(plan._h, None, None, base, 0, None, None, None, 0) == 0
    assert gpu.lib().lolhip_gadget_encode_batch(plan._h, None, None, base, None, None, 0) == 0
    assert gpu.lib().lolhip_gadget_correct_batch(plan._h, None, None, base, 0, None, None, None, 1) == -1


def test_encode_misaligned_pair_slab(gpu):
    """the 8-byte route of k_gadget_encode: an output slab one word off 16-byte alignment, guard words around it"""
    import torch
    plan, B, base = _plan(gpu, 32, PAIR), SHAPES[32], 16
    rng = np.random.default_rng(17)
    L = plan.decomposeLen(base)
    s = _residues(rng, PAIR, (B, plan.n))
    e = rng.integers(-100, 101, size=(L, B, plan.n), dtype=np.int64)
    want = plan.gadgetEncode(s, base, e)
    ds, de = torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda()
    out = torch.full((want.size + 5,), GUARD, dtype=torch.int64, device="cuda")
    assert out.data_ptr() % 16 == 0
    rc = gpu.lib().lolhip_gadget_encode_batch(plan._h, torch.cuda.current_stream().cuda_stream, ds.data_ptr(), base,
                                              de.data_ptr(), out.data_ptr() + 24, B)
    assert rc == 0
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:3] == GUARD).all() and (h[-2:] == GUARD).all()
    assert np.array_equal(h[3:-2].reshape(want.shape), want)


@pytest.mark.parametrize("m,qs,base", [(32, [Q60], 256), (32, [12289], 4), (45, PAIR, 2), (32, PAIR, 0)], ids=lambda v: str(v))
def test_consistency_with_decompose(gpu, m, qs, base):
    """both directions of the gadget on the device: for e = 0, sum_j g_j decompose(u)_j = u = s"""
    plan, B = _plan(gpu, m, qs), SHAPES[m]
    rng = np.random.default_rng(19 * m + base)
    s = _residues(rng, qs, (B, plan.n))
    u, es = plan.gadgetCorrect(plan.gadgetEncode(s, base), base)
    assert np.array_equal(u, s)
    if not (base == 0 and plan.T == 2):
        assert not es.any()
    digits, g = plan.decompose(u, base).astype(object), plan.gadget(base)
    back = sum(digits[j] * [int(v) for v in g[j]] for j in range(len(g))) % np.array(qs, dtype=object)
    assert np.array_equal(_i64(back), u)
