"""The persistent pipelined poly-mul k_pow2_pipe<L, AR, SQ> (pow2_pipe.hip) on the device (-m gpu), bit-exact.

Every call that is meant to run the pipe runs with LOLHIP_PIPE_INFO=1 and PROVES from the launcher's stderr line that
k_pow2_pipe<L,AR> ran, with the expected grid where one was set: a call that pow2_pipe_ok declined would otherwise pass
on k_pow2's words.  What is compared:

  class ends    both moduli of every arithmetic class (pipe_cases.py) at L = 12, 13, the nine edge rows, a * b and a * a:
                against the oracle, against the rows' closed forms and against the one-polynomial-per-workgroup kernel
  round shapes  grid overrides 1, 2, 3, 5 with batches around them (one, two, three iterations per workgroup, ragged
                last rounds: the tail re-fetch and the last prefetch)
  real grid     the dispatch threshold 2048 and 2047 unforced, 2049 forced
  aliasing      out = a, out = b, in-place squaring, on a small grid and on the real one
  alignment     operands one word off a 16-byte boundary (the pipe runs), the output one word off (it must not)
  side stream   a forced call on a stream of its own
tests/test_pipe_host.py checks the case table and the arithmetic ranges without a GPU.
"""
import re

import numpy as np
import pytest
import torch

from oracle.oracle import Params

import pipe_cases as pc

pytestmark = pytest.mark.gpu

INFO = re.compile(r"k_pow2_pipe<(\d+),(\d+)>: lds (\d+) B, per_cu (\d+), occupancy query (-?\d+) \(err (-?\d+)\), grid (-?\d+)")
GUARD = -0x5A5A5A5A5A5A5A5B
_cache = {}


def plans(gpu, L, q):
    key = ("plan", L, q)
    if key not in _cache:
        _cache[key] = (gpu.Plan([(2, L + 1)], [q]), Params([(2, L + 1)], [q]))
    return _cache[key]


def edge_rows(cpuref, L, q):
    """host rows, their device copies and the oracle's a * b and a * a, computed once per (L, q)"""
    key = ("rows", L, q)
    if key not in _cache:
        R = Params([(2, L + 1)], [q])
        a, b = pc.rows(q, L)
        want = {False: cpuref.polymul(R, a, b).reshape(a.shape), True: cpuref.polymul(R, a, a).reshape(a.shape)}
        _cache[key] = (a, b, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), want)
    return _cache[key]


def round_rows(cpuref, L, q):
    """pc.ROUND_BMAX rows: the edge rows, then random signed ones; the oracle runs once for all batch sizes"""
    key = ("round", L, q)
    if key not in _cache:
        R = Params([(2, L + 1)], [q])
        a, b = pc.rows(q, L)
        rng = np.random.default_rng([7, L, q])
        more = pc.ROUND_BMAX - a.shape[0]
        a = np.concatenate([a, rng.integers(-(q - 1), q, size=(more, R.n, 1))])
        b = np.concatenate([b, rng.integers(-(q - 1), q, size=(more, R.n, 1))])
        a, b = a[::-1].copy(), b[::-1].copy()                  # the edge rows last: small batches see random rows too
        want = {False: torch.from_numpy(cpuref.polymul(R, a, b).reshape(a.shape)).cuda(),
                True: torch.from_numpy(cpuref.polymul(R, a, a).reshape(a.shape)).cuda()}
        _cache[key] = (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), want)
    return _cache[key]


def info_lines(capfd):
    torch.cuda.synchronize()
    return [tuple(int(g) for g in m.groups()) for m in INFO.finditer(capfd.readouterr().err)]


class Pipe:
    """polymul with the route proved: forced() must show one k_pow2_pipe<L,AR> line, other() none"""

    def __init__(self, gpu, capfd, monkeypatch, L, q):
        self.gpu, self.capfd, self.mp, self.L, self.q, self.ar = gpu, capfd, monkeypatch, L, q, pc.arith_class(q)
        self.P, self.R = plans(gpu, L, q)
        self.G = None
        monkeypatch.setenv("LOLHIP_PIPE_INFO", "1")
        monkeypatch.delenv("LOLHIP_PIPE_GRID", raising=False)

    def grid(self, G):
        if G is None:
            self.mp.delenv("LOLHIP_PIPE_GRID", raising=False)
        else:
            self.mp.setenv("LOLHIP_PIPE_GRID", str(G))
        self.G = G

    def _call(self, a, b, out, switch, stream=None):
        info_lines(self.capfd)                                 # drain
        if switch:
            self.gpu.debug_set(switch, True)
        try:
            self.P.polymul(a, b, out=out, stream=stream)
        finally:
            if switch:
                self.gpu.debug_set(switch, False)
        return info_lines(self.capfd)

    def ran_pipe(self, lines, G=None):
        assert len(lines) == 1, f"expected one k_pow2_pipe<{self.L},{self.ar}> launch, stderr showed {lines}"
        L, ar, lds, per_cu, _occ, _err, grid = lines[0]
        assert (L, ar) == (self.L, self.ar), lines
        if G is not None:
            assert grid == G, lines
        else:
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            assert grid == cus * per_cu and per_cu >= 1, (lines, cus)
        return grid

    def forced(self, a, b, out=None, stream=None):
        out = torch.empty_like(a) if out is None else out
        self.ran_pipe(self._call(a, b, out, "FORCE_PIPE", stream), self.G)
        return out

    def no_pipe(self, a, b):
        out = torch.empty_like(a)
        assert self._call(a, b, out, "NO_PIPE") == []
        return out

    def default(self, a, b):
        out = torch.empty_like(a)
        return out, self._call(a, b, out, None)


@pytest.fixture
def pipe(gpu, capfd, monkeypatch):
    return lambda L, q: Pipe(gpu, capfd, monkeypatch, L, q)


def _same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


# ---- class ends and edge rows ---------------------------------------------------------------------------------------
def test_route_cases_are_the_ones_run_below():
    assert sorted(pc.ROUTE_CASES) == sorted((L, q, sq) for L in pc.LS for q in pc.MODULI for sq in (False, True))


@pytest.mark.parametrize("L", pc.LS)
@pytest.mark.parametrize("q", pc.MODULI)
def test_class_ends_and_edge_rows(pipe, cpuref, q, L):
    a, b, da, db, want = edge_rows(cpuref, L, q)
    p = pipe(L, q)
    for sq in (False, True):
        assert (L, q, sq) in pc.ROUTE_CASES
        x, y = (da, da) if sq else (da, db)
        got = p.forced(x, y)
        g = got.cpu().numpy()
        for nm, i in pc.ROW.items():
            assert np.array_equal(g[i], want[sq][i]), (nm, sq, "oracle")
        for nm, v in pc.closed_forms(q, L, a, b, sq).items():
            assert np.array_equal(g[pc.ROW[nm]].reshape(-1), v), (nm, sq, "closed form")
        assert torch.equal(got, p.no_pipe(x, y)), (sq, "pipe vs one-polynomial-per-workgroup kernel")
    assert torch.equal(da, torch.from_numpy(a).cuda()) and torch.equal(db, torch.from_numpy(b).cuda())     # operands intact


# ---- round shapes of the persistent loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("G", pc.ROUND_GRIDS)
@pytest.mark.parametrize("L,q", pc.ROUND_PLANS)
def test_round_shapes(pipe, cpuref, L, q, G):
    da, db, want = round_rows(cpuref, L, q)
    p = pipe(L, q)
    p.grid(G)
    for B in pc.round_batches(G):
        for sq in (False, True):
            x, y = (da[:B], da[:B]) if sq else (da[:B], db[:B])
            out = torch.full((B + 1, 1 << L, 1), GUARD, dtype=torch.int64, device="cuda")
            p.forced(x, y, out=out[:B])
            assert torch.equal(out[:B], want[sq][:B]), (B, sq)
            assert bool((out[B] == GUARD).all()), (B, sq, "wrote past the batch")


# ---- the real grid -----------------------------------------------------------------------------------------------------
def test_real_grid_threshold_and_multiple_plus_one(pipe, cpuref):
    L, q, n = pc.REAL_L, pc.REAL_Q, 1 << pc.REAL_L
    p = pipe(L, q)
    p.grid(None)
    gen = torch.Generator(device="cuda").manual_seed(2048)
    a = torch.randint(-(q - 1), q, (pc.REAL_FORCED, n, 1), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(-(q - 1), q, (pc.REAL_FORCED, n, 1), dtype=torch.int64, device="cuda", generator=gen)
    ref = p.no_pipe(a, b)
    rows = [0, 1, 511, 512, 1023, 1024]

    def check(got, B, what):
        assert torch.equal(got, ref[:B]), what
        rr = rows + [B - 1]
        assert _same(got[rr], cpuref.polymul(p.R, a[rr].cpu().numpy(), b[rr].cpu().numpy()).reshape(len(rr), n, 1)), what

    B = pc.REAL_THRESHOLD
    got, lines = p.default(a[:B], b[:B])
    grid = p.ran_pipe(lines)                                   # the default route from 2048 polynomials up
    check(got, B, "threshold")
    got, lines = p.default(a[:B - 1], b[:B - 1])
    assert lines == [], "2047 polynomials took the pipe unforced"
    check(got, B - 1, "below the threshold")
    del got
    B = pc.REAL_FORCED
    assert B > grid, "the device holds the whole batch in one round"
    check(p.forced(a, b), B, "forced")


# ---- aliasing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,B", [(2, 5), (None, pc.REAL_ALIAS_B)], ids=["grid2_B5", "real_grid_B1100"])
def test_aliasing(pipe, cpuref, G, B):
    L, q, n = pc.REAL_L, pc.REAL_Q, 1 << pc.REAL_L
    p = pipe(L, q)
    p.grid(G)
    gen = torch.Generator(device="cuda").manual_seed(B)
    a = torch.randint(-(q - 1), q, (B, n, 1), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(-(q - 1), q, (B, n, 1), dtype=torch.int64, device="cuda", generator=gen)
    ab, aa = p.forced(a, b), p.forced(a, a)
    assert torch.equal(ab, p.no_pipe(a, b)) and torch.equal(aa, p.no_pipe(a, a))
    if B <= 11:
        ah, bh = a.cpu().numpy(), b.cpu().numpy()
        assert _same(ab, cpuref.polymul(p.R, ah, bh).reshape(B, n, 1)) and _same(aa, cpuref.polymul(p.R, ah, ah).reshape(B, n, 1))
    x = a.clone()
    p.forced(x, b, out=x)
    assert torch.equal(x, ab), "out = a"
    y = b.clone()
    p.forced(a, y, out=y)
    assert torch.equal(y, ab), "out = b"
    x = a.clone()
    p.forced(x, x, out=x)
    assert torch.equal(x, aa), "in-place square"


# ---- alignment -------------------------------------------------------------------------------------------------------
def _off_by(t, words):
    """a copy of t whose first word sits `words` int64 past a 16-byte boundary, between guard words: (view, buffer)"""
    buf = torch.full((t.numel() + 4,), GUARD, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[2 + words:2 + words + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 * words
    return v, buf


def _guards_intact(buf, words, numel):
    return bool((buf[:2 + words] == GUARD).all()) and bool((buf[2 + words + numel:] == GUARD).all())


@pytest.mark.parametrize("off_a,off_b", [(1, 0), (0, 1), (1, 1)], ids=["a_off", "b_off", "both_off"])
def test_operands_one_word_off_still_take_the_pipe(pipe, cpuref, off_a, off_b):
    L, q = 13, pc.TOP[3]
    da, db, want = round_rows(cpuref, L, q)
    B = 5
    p = pipe(L, q)
    p.grid(2)
    a, abuf = _off_by(da[:B], off_a)
    b, bbuf = _off_by(db[:B], off_b)
    out, obuf = _off_by(torch.zeros_like(da[:B]), 0)
    p.forced(a, b, out=out)
    assert torch.equal(out, want[False][:B])
    assert _guards_intact(obuf, 0, out.numel()) and _guards_intact(abuf, off_a, a.numel()) and _guards_intact(bbuf, off_b, b.numel())
    assert torch.equal(a, da[:B]) and torch.equal(b, db[:B])
    if off_a:                                                   # squaring from an operand that is one word off
        out.zero_()
        p.forced(a, a, out=out)
        assert torch.equal(out, want[True][:B]) and _guards_intact(obuf, 0, out.numel())


def test_output_one_word_off_falls_back(pipe, cpuref):
    L, q = 13, pc.TOP[3]
    da, db, want = round_rows(cpuref, L, q)
    B = 5
    p = pipe(L, q)
    p.grid(2)
    out, obuf = _off_by(torch.zeros_like(da[:B]), 1)
    lines = p._call(da[:B], db[:B], out, "FORCE_PIPE")
    assert lines == [], "the pipe stores 16 bytes per lane: it must decline an output that is only 8-byte aligned"
    assert torch.equal(out, want[False][:B]) and _guards_intact(obuf, 1, out.numel())


# ---- side stream -----------------------------------------------------------------------------------------------------
def test_side_stream(pipe, cpuref):
    L, q = 13, pc.TOP[2]
    da, db, want = round_rows(cpuref, L, q)
    B = 5
    p = pipe(L, q)
    p.grid(2)
    out, obuf = _off_by(torch.zeros_like(da[:B]), 0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    p.forced(da[:B], db[:B], out=out, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(out, want[False][:B]) and _guards_intact(obuf, 0, out.numel())
