"""The exact ring product over moduli without a CRT basis on the device (lol_amd.RingMul, lolhip_ringmul_*), bit for
bit against the Python-integer oracle tests/ringmul_ref.py: every transform route, even / odd / 62-bit moduli with the
rounding tie q/2 in every position, a mixed T = 3 tuple, operands that bring the integer product to +-n H^2 next to the
fold's sign threshold prod Q / 2, aliasing and unaligned slabs, the prepared operand, and m = 16384."""

import numpy as np
import pytest

import ringmul_ref as rr
from oracle import lolmath as lm

pytestmark = pytest.mark.gpu
POISON = -0x0123456789ABCDEF


def _full(rng, shape):
    return rng.integers(-2 ** 63, 2 ** 63, size=shape, dtype=np.int64)


_cache = {}


def _ring(gpu, m, qs, Qs=None):
    """RingMul over device plans: plan_Q by the default rule, or over the given primes"""
    key = (m, tuple(qs), None if Qs is None else tuple(Qs))
    if key not in _cache:
        pps = lm.factor_pps(m)
        _cache[key] = gpu.RingMul(gpu.Plan(pps, list(qs)), None if Qs is None else gpu.Plan(pps, list(Qs)))
    return _cache[key]


# ---- 1. one index per transform route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 64, 45, 21, 34])
def test_index_families(gpu, m):
    rng = np.random.default_rng(m)
    for qs in ([2 ** 32], [3 ** 9]):
        rm = _ring(gpu, m, qs)
        a, b = _full(rng, (3, rm.n, 1)), _full(rng, (3, rm.n, 1))
        a[0, 0, 0], b[0, -1, 0] = -2 ** 63, 2 ** 63 - 1
        assert np.array_equal(rm(a, b), rr.mul(m, a, b, qs)), (m, qs)


# ---- 2. moduli -------------------------------------------------------------------------------------------------------------
def _tie_rows(rng, n, q):
    """operands with the tie q/2 (and its neighbours) in every position of a and of b, and everywhere at once"""
    h = q // 2
    a, b = rng.integers(0, q, size=(n + 3, n, 1)).astype(np.int64), rng.integers(0, q, size=(n + 3, n, 1)).astype(np.int64)
    for j in range(n):
        a[j, j, 0], b[j, n - 1 - j, 0] = h, h
    a[n], b[n] = h, h
    a[n + 1], b[n + 1] = h, (h + 1) % q
    a[n + 2], b[n + 2] = (h + q - 1) % q, h
    return a, b


@pytest.mark.parametrize("q,K", [(2, 1), (8, 1), (15, 1), (2 ** 32, 2), (2 ** 61 + 1, 3), (2 ** 62 - 1, 3)])
def test_moduli_and_rounding_ties(gpu, q, K):
    m, rng = 16, np.random.default_rng(q % 1000003)
    rm = _ring(gpu, m, [q])
    assert rm.K == K
    a, b = _tie_rows(rng, rm.n, q)
    assert np.array_equal(rm(a, b), rr.mul(m, a, b, [q]))
    a2, b2 = a - q * (a > q // 3), b - q * (b % 2 == 1)             # other representatives of the same classes
    assert np.array_equal(rm(a2, b2), rr.mul(m, a, b, [q]))


def test_ntt_prime_equals_plan_polymul(gpu):
    m, q = 16, 12289
    rm, rng = _ring(gpu, m, [q]), np.random.default_rng(5)
    assert rm.plan_q.has_crt
    a, b = _tie_rows(rng, rm.n, q)
    got = rm(a, b)
    assert np.array_equal(got, rr.mul(m, a, b, [q]))
    assert np.array_equal(got, rm.plan_q.polymul(a, b))


# ---- 3. a mixed tuple ------------------------------------------------------------------------------------------------------
def test_mixed_tuple_deinterleaves(gpu):
    m, qs = 64, [2 ** 16, 12289, 3 ** 20]
    rm, rng = _ring(gpu, m, qs), np.random.default_rng(64)
    assert (rm.T, rm.K) == (3, 2)
    a, b = _full(rng, (3, rm.n, 3)), _full(rng, (3, rm.n, 3))
    got = rm(a, b)
    assert np.array_equal(got, rr.mul(m, a, b, qs))
    for t, q in enumerate(qs):
        one = _ring(gpu, m, [q])(np.ascontiguousarray(a[..., t:t + 1]), np.ascontiguousarray(b[..., t:t + 1]))
        assert np.array_equal(got[..., t:t + 1], one), t
    pows = [2 ** 16, 2 ** 8, 2 ** 30]                            # every q_t a power of two: the masked route, T = 3
    a, b = _full(rng, (2, rm.n, 3)), _full(rng, (2, rm.n, 3))
    assert np.array_equal(_ring(gpu, m, pows)(a, b), rr.mul(m, a, b, pows))


# ---- 4. next to the fold's threshold ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,Qs", rr.BOUNDARY)
def test_products_next_to_half_the_modulus(gpu, m, Qs):
    n = len(rr.cr.ring(m).expo)
    for odd in (True, False):
        q, _, ratio = rr.boundary_pair(m, Qs, odd)
        H = q // 2
        rm = _ring(gpu, m, [q], Qs)
        plus, minus = H, q - H                                     # residues of the lifts +H and -H (even q: both are -H)
        rows = [(np.full(n, plus), np.full(n, plus)), (np.full(n, plus), np.full(n, minus)),
                (np.full(n, minus), np.full(n, minus))]
        for i, j, sa, sb in ((0, 0, plus, plus), (n - 1, n - 1, plus, minus), (n - 1, 1, minus, minus), (3, n - 3, plus, minus),
                             (n // 2, n // 2, plus, plus)):
            x, y = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            x[i], y[j] = sa, sb
            rows.append((x, y))
        a = np.stack([r[0] for r in rows]).astype(np.int64)[..., None]
        b = np.stack([r[1] for r in rows]).astype(np.int64)[..., None]
        if m == 16 and odd:                                        # the top coefficient of the all-(+H) square is + n H^2
            top = rr.mul_int(m, [H] * n, [H] * n)
            assert max(abs(int(v)) for v in top) == n * H * H == int(top[n - 1]) and 2 * n * H * H < int(np.prod(Qs, dtype=object))
        assert np.array_equal(rm(a, b), rr.mul(m, a, b, [q])), (Qs, q, ratio)


# ---- 5. memory shapes -------------------------------------------------------------------------------------------------------
def _raw_call(gpu, rm, out, a, b, work, B, stream=None):
    import torch
    s = (stream or torch.cuda.current_stream()).cuda_stream
    rc = gpu.lib().lolhip_ringmul_batch(rm._h, s, out.data_ptr(), a.data_ptr(), b.data_ptr(), work.data_ptr(), B)
    assert rc == 0


@pytest.mark.parametrize("m,q", [(16, 2 ** 32), (45, 15), (2, 4), (2, 2 ** 32)])
def test_memory_shapes(gpu, m, q):
    """aliasing, slabs offset by 8 bytes, an odd word count (n = 1), a side stream, B = 0, guards and poisoned scratch"""
    import torch
    rm, rng, B = _ring(gpu, m, [q]), np.random.default_rng(m + 1), 3
    n, words = rm.n, 3 * rm.n
    a, b = _full(rng, (B, n, 1)), _full(rng, (B, n, 1))
    want, want_sq = rr.mul(m, a, b, [q]), rr.mul(m, a, a, [q])
    wl = rm.workLen(B)
    assert wl == 2 * ((words * rm.K + 1) // 2 * 2) and (words % 2 == 1) == (m == 2)
    dev = lambda x: torch.from_numpy(x).cuda()
    G = 4                                                           # guard words around out and work
    side = torch.cuda.Stream()
    for off in (0, 1):                                              # off = 1: every slab 8 bytes off a 16-byte boundary
        def slab(x=None):
            buf = torch.full((G + off + words + G,), POISON, dtype=torch.int64, device="cuda")
            view = buf[G + off:G + off + words]
            assert view.data_ptr() % 16 == 8 * off
            if x is not None:
                view.copy_(dev(x).reshape(-1))
            return buf, view
        wbuf = torch.full((G + wl + G,), POISON, dtype=torch.int64, device="cuda")
        work = wbuf[G:G + wl]
        assert work.data_ptr() % 16 == 0
        for kind in ("plain", "out=a", "out=b", "a is b", "square in place", "side stream"):
            (_, da), (_, db), (obuf, out) = slab(a), slab(b), slab()
            wbuf.fill_(POISON)
            torch.cuda.synchronize()
            if kind == "out=a":
                obuf, out = _, da = slab(a)
            elif kind == "out=b":
                obuf, out = _, db = slab(b)
            elif kind == "a is b":
                db = da
            elif kind == "square in place":
                obuf, out = _, da = slab(a)
                db = da
            if kind == "side stream":
                side.wait_stream(torch.cuda.current_stream())
                _raw_call(gpu, rm, out, da, db, work, B, side)
                side.synchronize()
            else:
                _raw_call(gpu, rm, out, da, db, work, B)
            torch.cuda.synchronize()
            exp = want_sq if db is da else want
            assert np.array_equal(out.cpu().numpy().reshape(B, n, 1), exp), (kind, off)
            assert (obuf[:G + off] == POISON).all() and (obuf[G + off + words:] == POISON).all(), (kind, off)
            assert (wbuf[:G] == POISON).all() and (wbuf[G + wl:] == POISON).all(), (kind, off)
    # B = 0: nothing is read or written
    obuf = torch.full((8,), POISON, dtype=torch.int64, device="cuda")
    assert gpu.lib().lolhip_ringmul_batch(rm._h, None, obuf.data_ptr(), obuf.data_ptr(), obuf.data_ptr(), obuf.data_ptr(), 0) == 0
    assert gpu.lib().lolhip_ringmul_batch(rm._h, None, None, None, None, None, 0) == 0
    torch.cuda.synchronize()
    assert (obuf == POISON).all()
    assert rm(np.zeros((0, n, 1), dtype=np.int64), np.zeros((0, n, 1), dtype=np.int64)).shape == (0, n, 1)


# ---- 6. the prepared operand ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,qs", [(16, [2 ** 32]), (45, [2 ** 20, 15]), (64, [2 ** 62 - 1])])
def test_prepared_operand(gpu, m, qs):
    rm, rng, B = _ring(gpu, m, qs), np.random.default_rng(m + 7), 3
    a, b = _full(rng, (B, rm.n, rm.T)), _full(rng, (B, rm.n, rm.T))
    direct = rm(a, b)
    assert np.array_equal(direct, rr.mul(m, a, b, qs))
    bhat = rm.prepare(b)
    assert bhat.shape == (B * rm.T, rm.n, rm.K)
    assert np.array_equal(rm.mulPrepared(a, bhat), direct)                                       # Bb = B
    one = rm.prepare(b[1:2])
    assert np.array_equal(rm.mulPrepared(a, one), rm(a, np.repeat(b[1:2], B, axis=0)))           # Bb = 1
    with pytest.raises(gpu.LolHipError):
        rm.mulPrepared(a, rm.prepare(b[:2]))                                                     # Bb not in {1, B}


# ---- 7. m = 16384 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,K", [(2 ** 8, 1), (2 ** 32, 2)])
def test_large_two_power(gpu, q, K):
    m, n, H = 16384, 8192, q // 2
    rm, rng, expo = _ring(gpu, m, [q]), np.random.default_rng(K), rr.pow2_expo(16384)
    assert rm.K == K and rm.n == n
    mono = lambda e, v: np.array([v if i == e else 0 for i in range(n)], dtype=np.int64)
    # rows by exponent (x = zeta_m), with their products in closed form over the integers
    k = np.arange(n, dtype=object)
    nat = [(np.full(n, H - 1), np.full(n, H - 1), (2 * k + 2 - n) * ((H - 1) * (H - 1))),      # all lifts +(H - 1)
           (np.full(n, H - 1), np.full(n, H + 1), (2 * k + 2 - n) * (-(H - 1) * (H - 1))),     # ... times all -(H - 1)
           (mono(n - 1, H - 1), mono(n - 1, H - 1), mono(n - 2, 1).astype(object) * (-(H - 1) * (H - 1))),   # x^(n-1) x^(n-1) = -x^(n-2)
           (mono(5, -1), mono(n - 6, 3), mono(n - 1, 1).astype(object) * -3)]                  # x^5 x^(n-6) = x^(n-1)
    rows_a = [x[expo] for x, _, _ in nat] + [_full(rng, n), _full(rng, n)]
    rows_b = [y[expo] for _, y, _ in nat] + [_full(rng, n), _full(rng, n)]
    for lo in (0, 2, 4):                                           # B = 2 per call
        a = np.stack(rows_a[lo:lo + 2]).astype(np.int64)[..., None]
        b = np.stack(rows_b[lo:lo + 2]).astype(np.int64)[..., None]
        got = rm(a, b)
        for r in range(2):
            want = rr.mul_pow2(m, a[r, :, 0], b[r, :, 0], q)
            if lo + r < 4:
                closed = np.array([int(v) % q for v in nat[lo + r][2]], dtype=np.int64)[expo]
                assert np.array_equal(want, closed) and closed.any(), (q, lo + r)
            assert np.array_equal(got[r, :, 0], want), (q, lo + r)
