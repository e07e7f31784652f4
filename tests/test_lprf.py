"""The key-homomorphic lattice PRF on the device (-m gpu; lolhip_lprf_eval_batch / lolhip_lprf_batch, lprf.hip), bit for
bit against the per-input restatement of tests/lprf_ref.py.

Every call runs with LOLHIP_LPRF_INFO set and the route of each node launch is read from the launcher's stderr line, never
assumed: wherever the restated host rule (the certificate, and K at or above the measured crossover) takes the matrix cores
the case runs a second time under the LPRF_VALU switch,
must show only `valu` lines there and only `mfma` lines by default, and must give identical bits.  out and work sit between
guard words and work is poisoned before each call.  Shapes are the smallest that reach each thing: the reference's own
benchmark and example shapes, M, N and K off the 32 / 64 / 128 tiles with several k-steps, W = 8 limbs, a 2-power and a
62-bit modulus, the int8 edge of the gadget base, TrivGad, saturated lazy sums over more than two reduction intervals,
several keys with entries outside [0, q), a one-leaf tree, a side stream and a second window on one family.
"""
import functools
import re

import numpy as np
import pytest

import lprf_ref as lr

pytestmark = pytest.mark.gpu

G = 64
GUARD = 0x7E7E7E7E7E7E
POISON = -0x0123456789ABCDEF
INFO = re.compile(r"k_lprf: route (\w+), M (\d+), N (\d+), K (\d+), W (\d+), slots (\d+)")
Q62 = 2 ** 62 - 57                                                    # the largest prime below 2^62
Q61 = 2 ** 61 - 1
Q56 = 2 ** 56 - 5


@pytest.fixture
def info(monkeypatch, capfd):
    """reads the launcher's lines printed since the last call: [(route, M, N, K, W, slots)]"""
    monkeypatch.setenv("LOLHIP_LPRF_INFO", "1")
    capfd.readouterr()

    def read():
        return [(r,) + tuple(int(v) for v in rest) for r, *rest in INFO.findall(capfd.readouterr().err)]
    return read


def _family(q, base, n, seed):
    rng = np.random.default_rng(seed)
    K = n * lr.ell_of(q, base)
    return tuple(rng.integers(0, q, size=(n, K), dtype=np.int64) for _ in range(2))


@functools.lru_cache(maxsize=None)
def _want_eval(q, base, tree, n, seed, x0, B):
    a0, a1 = _family(q, base, n, seed)
    return lr.eval_window(q, base, list(tree), a0, a1, x0, B)


def _guarded(torch, words, fill):
    return torch.full((G + words + G,), fill, dtype=torch.int64, device="cuda")


def _intact(buf, words, fill):
    return bool((buf[:G] == fill).all()) and bool((buf[G + words:] == fill).all())


class Runner:
    """one family on the device; eval / prf run the raw entries between guards and return (numpy result, info lines)"""

    def __init__(self, gpu, info, q, base, tree, a0, a1):
        import torch
        self.torch, self.gpu, self.info, self.L = torch, gpu, info, gpu.lib()
        self.q, self.base, self.tree, self.a0, self.a1 = q, base, list(tree), a0, a1
        self.f = gpu.LatticePRF(q, base, tree, a0, a1)
        self.admitted = lr.mfma_default(q, base, self.f.K)            # W where the matrix route is the default, else 0

    def _call(self, nkeys, x0, B, words, fn, stream=None):
        torch, f = self.torch, self.f
        wl = f.workLen(nkeys, x0, B)
        assert wl == lr.work_len(self.tree, f.n, f.K, nkeys, x0, B)
        obuf, wbuf = _guarded(torch, words, GUARD), _guarded(torch, wl, POISON)
        self.info()
        st = stream.cuda_stream if stream is not None else None
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        rc = fn(st, obuf.data_ptr() + 8 * G, wbuf.data_ptr() + 8 * G)
        (stream or torch.cuda.current_stream()).synchronize()
        assert rc == 0, rc
        assert _intact(obuf, words, GUARD) and _intact(wbuf, wl, POISON), "a guard word was overwritten"
        return obuf[G:G + words].cpu().numpy(), self.info()

    def eval(self, x0, B, stream=None):
        f = self.f
        fn = lambda st, o, w: self.L.lolhip_lprf_eval_batch(f._h, st, x0, B, o, w)
        out, lines = self._call(0, x0, B, B * f.n * f.K, fn, stream)
        return out.reshape(B, f.n, f.K), lines

    def prf(self, s, p, x0, B, stream=None):
        f, torch = self.f, self.torch
        s = np.ascontiguousarray(np.asarray(s, dtype=np.int64).reshape(-1, f.n))
        ds = torch.from_numpy(s).cuda()
        fn = lambda st, o, w: self.L.lolhip_lprf_batch(f._h, st, ds.data_ptr(), s.shape[0], p, x0, B, o, w)
        out, lines = self._call(s.shape[0], x0, B, s.shape[0] * B * f.K, fn, stream)
        return out.reshape(s.shape[0], B, f.K), lines

    def both_routes(self, run, want, internal=True):
        """run() on the default route and, where the matrix route is admitted, again under LPRF_VALU: the same bits as
        `want`, and the info lines prove which route ran (no line at all for a one-leaf tree or B = 0)"""
        got, lines = run()
        assert np.array_equal(got, want)
        routes = {ln[0] for ln in lines}
        assert routes == (({"mfma"} if self.admitted else {"valu"}) if internal else set()), lines
        if self.admitted and internal:
            assert all(ln[4] == self.admitted and ln[2] == ln[3] == self.f.K for ln in lines), lines
            self.gpu.debug_set("LPRF_VALU", True)
            try:
                got2, lines2 = run()
            finally:
                self.gpu.debug_set("LPRF_VALU", False)
            assert {ln[0] for ln in lines2} == {"valu"} and len(lines2) == len(lines), lines2
            assert np.array_equal(got2, want)
        return lines


def _prf_from(want, s, q, p):
    """rescale <$> s A for the restated A_T of a window: want [B][n][K], s [nkeys][n] -> [nkeys][B][K]"""
    out = np.zeros((s.shape[0], want.shape[0], want.shape[2]), dtype=np.int64)
    for k in range(s.shape[0]):
        for b in range(want.shape[0]):
            out[k, b] = lr.rescale((s[k].astype(object) % q).dot(want[b].astype(object)) % q, q, p).astype(np.int64)
    return out


def _check(gpu, info, q, p, base, n, tree, seed, windows, keysets):
    a0, a1 = _family(q, base, n, seed)
    r = Runner(gpu, info, q, base, tree, a0, a1)
    rng = np.random.default_rng(seed + 1)
    for x0, B in windows:
        want = _want_eval(q, base, tuple(tree), n, seed, x0, B)
        r.both_routes(lambda: r.eval(x0, B), want, internal=B > 0 and len(tree) > 1)
        for nkeys in keysets:
            s = rng.integers(0, q, size=(nkeys, n), dtype=np.int64)
            wantp = _prf_from(want, s, q, p)
            lines = r.both_routes(lambda: r.prf(s, p, x0, B), wantp, internal=B > 0 and len(tree) > 1)
            if lines:                                                  # the keyed root has nkeys rows per slot
                assert lines[-1][5] == B and lines[-1][1] % nkeys == 0, lines
    return r


# ---- the reference's own shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["left", "balanced", "right"])
def test_reference_benchmark_shape(gpu, info, shape):
    """Benchmarks/Default.hs:82-88: Zq 8 -> Zq 2, n = 3, BaseBGad 2, 5 leaves; every input, and partial windows.
    K = 12 is below the crossover: the VALU route is the default here (the info lines say so)"""
    tree = {"left": gpu.left_spine_tree, "balanced": gpu.balanced_tree, "right": gpu.right_spine_tree}[shape](5)
    _check(gpu, info, 8, 2, 2, 3, tree, 1, [(0, 32), (5, 4), (31, 1), (7, 0)], [1])


@pytest.mark.parametrize("nkeys", [1, 3])
def test_reference_example_shape(gpu, info, nkeys):
    """Examples/KHPRF.hs:54-68: n = 3, a balanced tree of 10 leaves, Zq 257 -> Zq 32, BaseBGad 2"""
    _check(gpu, info, 257, 32, 2, 3, gpu.balanced_tree(10), 2, [(0, 8), (1020, 4)], [nkeys])


# ---- tiles, limbs, moduli -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,p,n,K,W", [(5, 2, 33, 99, 1), (8, 2, 16, 64, 1), (257, 32, 7, 63, 2)])
def test_tile_tails(gpu, info, q, p, n, K, W):
    """n = 33, q = 5, base 2: K = 99 and the stacked rows are off every tile edge, the depth takes several k-steps; the
    reference's two moduli at the smallest widths the matrix route takes (ell = 4: four entries per 16-element unit with
    none left over, ell = 9: one entry per unit and seven zeros)"""
    r = _check(gpu, info, q, p, 2, n, [3, 2, 1, 1, 1], 3, [(0, 8)], [2])
    assert r.f.K == K and r.admitted == W


def test_widest_modulus(gpu, info):
    """a prime just below 2^62, base 2 (ell = 62, K = 124, W = 8); p = 2 keeps p q < 2^63, p = 3 does not"""
    r = _check(gpu, info, Q62, 2, 2, 2, [3, 1, 2, 1, 1], 4, [(0, 8), (3, 3)], [2])
    assert (r.f.ell, r.f.K, r.admitted) == (62, 124, 8)
    f, L = r.f, gpu.lib()
    import torch
    obuf = torch.full((8 * f.K,), GUARD, dtype=torch.int64, device="cuda")
    wbuf = torch.zeros((max(f.workLen(1, 0, 8), 1),), dtype=torch.int64, device="cuda")
    s = torch.zeros((f.n,), dtype=torch.int64, device="cuda")
    assert L.lolhip_lprf_batch(f._h, None, s.data_ptr(), 1, 3, 0, 8, obuf.data_ptr(), wbuf.data_ptr()) == gpu.tensor.ERR_MODULUS
    assert L.lolhip_lprf_batch(f._h, None, s.data_ptr(), 1, 1, 0, 8, obuf.data_ptr(), wbuf.data_ptr()) == gpu.tensor.ERR_MODULUS
    assert L.lolhip_lprf_batch(f._h, None, s.data_ptr(), 0, 2, 0, 8, obuf.data_ptr(), wbuf.data_ptr()) == gpu.tensor.ERR_INVALID
    assert L.lolhip_lprf_batch(f._h, None, s.data_ptr(), 1, 2, 5, 4, obuf.data_ptr(), wbuf.data_ptr()) == gpu.tensor.ERR_INVALID
    assert L.lolhip_lprf_batch(f._h, None, None, 1, 2, 0, 8, obuf.data_ptr(), wbuf.data_ptr()) == gpu.tensor.ERR_INVALID
    assert L.lolhip_lprf_eval_batch(f._h, None, 0, 8, None, wbuf.data_ptr()) == gpu.tensor.ERR_INVALID
    assert L.lolhip_lprf_eval_batch(f._h, None, 0, 8, obuf.data_ptr(), None) == gpu.tensor.ERR_INVALID
    assert L.lolhip_lprf_eval_batch(f._h, None, 7, 2, obuf.data_ptr(), wbuf.data_ptr()) == gpu.tensor.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((obuf == GUARD).all())


def test_power_of_two_modulus(gpu, info):
    r = _check(gpu, info, 2 ** 61, 2, 4, 2, [3, 2, 1, 1, 1], 5, [(0, 8), (2, 5)], [1])
    assert r.f.ell == 31 and r.admitted == 8


@pytest.mark.parametrize("base,n,route", [(128, 28, "mfma"), (254, 28, "mfma"), (256, 28, "valu"), (128, 27, "valu")])
def test_route_edges(gpu, info, base, n, route):
    """q = 12289 (ell = 2): digits of base 128 and 254 fit a signed byte (64, 127), those of base 256 reach 128; and
    K = 56 is the first depth the host rule gives to the matrix route, K = 54 the last it keeps on the VALU route"""
    a0, a1 = _family(12289, base, n, 6)
    r = Runner(gpu, info, 12289, base, [3, 1, 2, 1, 1], a0, a1)
    assert (r.admitted > 0) == (route == "mfma") and r.f.K == 2 * n
    lines = r.both_routes(lambda: r.eval(0, 8), _want_eval(12289, base, (3, 1, 2, 1, 1), n, 6, 0, 8))
    assert {ln[0] for ln in lines} == {route}


@pytest.mark.parametrize("q", [257, Q61])
def test_trivgad_takes_the_valu_route(gpu, info, q):
    r = _check(gpu, info, q, 4, 0, 5, [3, 1, 2, 1, 1], 7, [(0, 8), (1, 6)], [2])
    assert r.f.ell == 1 and r.admitted == 0 and (lr.valu_fold(q, 0) == 0) == (q == Q61)


@pytest.mark.parametrize("q,base,n", [(Q56, 2, 5), (Q62, 2, 2), (12289, 2, 10)])
def test_saturated_sums(gpu, info, q, base, n):
    """left operand all q - 1; right entries with every digit at the low end of its range (base 2: v = -(2^m - 1), the
    longest run of -1 digits the lift's range holds), so every term has one sign and full size; K is more than twice the
    VALU route's reduction interval (127 terms at Q56, 8 on the 128-bit path of Q62), and q = 12289 sums 140 such terms
    in the int64 path without any reduction"""
    ell = lr.ell_of(q, base)
    K = n * ell
    fold = lr.valu_fold(q, base)
    assert K >= 2 * (fold or 8) or fold > K
    m = (q // 2).bit_length() - 1
    v = -(2 ** m - 1)
    assert v >= -(q // 2) and m < ell
    a0 = np.full((n, K), q - 1, dtype=np.int64)
    a1 = np.full((n, K), v % q, dtype=np.int64)
    dig = lr.ginv(q, base, a1)
    assert (dig.reshape(n, ell, K)[:, :m] == q - 1).all()                 # digit -1 in every peeled place
    r = Runner(gpu, info, q, base, [2, 1, 1], a0, a1)
    want = lr.eval_window(q, base, [2, 1, 1], a0, a1, 0, 4)
    r.both_routes(lambda: r.eval(0, 4), want)
    s = np.full((2, n), q - 1, dtype=np.int64)
    wantp = _prf_from(want, s, q, 2)
    r.both_routes(lambda: r.prf(s, 2, 0, 4), wantp)


# ---- keys and launches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 2, 5])
def test_keys_outside_the_residue_range(gpu, info, nkeys):
    q, p, base, n = 257, 32, 2, 7
    a0, a1 = _family(q, base, n, 8)
    rng = np.random.default_rng(nkeys)
    s = rng.integers(-2 ** 62, 2 ** 62, size=(nkeys, n), dtype=np.int64)
    s[0, 0], s[-1, -1] = -1, q
    for tree, B in (([1], 2), ([3, 1, 2, 1, 1], 8)):
        r = Runner(gpu, info, q, base, tree, a0, a1)
        r.both_routes(lambda: r.prf(s, p, 0, B), lr.prf_window(q, base, tree, a0, a1, s, p, 0, B), internal=len(tree) > 1)
        if tree == [1]:                                                # A_T = A_x, and one input alone
            r.both_routes(lambda: r.eval(0, 2), np.stack([a0, a1]), internal=False)
            r.both_routes(lambda: r.prf(s, p, 1, 1), lr.prf_window(q, base, tree, a0, a1, s, p, 1, 1), internal=False)


def test_launch_hygiene(gpu, info):
    """a side stream, a second call on the same family with another window, the Python surface, destroy after use"""
    import torch
    q, p, base, n, tree, seed = 257, 32, 2, 7, [4, 2, 1, 1, 2, 1, 1], 9
    a0, a1 = _family(q, base, n, seed)
    r = Runner(gpu, info, q, base, tree, a0, a1)
    side = torch.cuda.Stream()
    for x0, B in ((0, 16), (3, 9)):
        want = _want_eval(q, base, tuple(tree), n, seed, x0, B)
        r.both_routes(lambda: r.eval(x0, B, stream=side), want)
    s = np.arange(2 * n, dtype=np.int64).reshape(2, n) * 37 - 50
    wantp = lr.prf_window(q, base, tree, a0, a1, s, p, 3, 9)
    r.both_routes(lambda: r.prf(s, p, 3, 9, stream=side), wantp)
    f = r.f
    assert np.array_equal(f.eval(3, 9).cpu().numpy(), _want_eval(q, base, tuple(tree), n, seed, 3, 9))
    assert np.array_equal(f(s, p, 3, 9).cpu().numpy(), wantp)
    got = f(torch.from_numpy(s[1]).cuda(), p, 3, 9, stream=side.cuda_stream)
    side.synchronize()                                                 # the call is ordered on `side` alone
    assert np.array_equal(got.cpu().numpy(), wantp[1])
    with pytest.raises(gpu.LolHipError):
        f.eval(10, 7)
    # Gray-code order is the caller's walk over one window call
    full = f(s[0], p, 0, 16).cpu().numpy()
    assert [tuple(full[x]) for x in gpu.gray_code(4)] == [tuple(lr.lattice_prf(q, base, tree, a0, a1, s[0], p, x).astype(np.int64))
                                                          for x in gpu.gray_code(4)]
    del r, f
    torch.cuda.synchronize()
