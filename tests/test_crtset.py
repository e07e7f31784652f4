"""crtSet and the clear-text tunnel on the device (lolhip_crtset, lolhip_pt_tunnel_batch; lol UCyc.hs:540-565, lol-apps
HomomPRF.hs:510-531).  Every comparison is bit for bit.

 - crtSet on the device against the host path for the cases of tests/test_crtset_host.py, and with `cap` rows between
   guard words;
 - PTTunnel over 8 -> 28 -> 182 and 16 -> 56 -> 364, p^e = 8 and 2, B = 1, 3, 257, on zero, all p^e - 1, unit-vector and
   random inputs against the schoolbook evalLin of tests/crtset_ref.py; on a side stream with the output between guard
   words; the unit vectors of O_8 against their closed form, one product of two CRT-set elements each; PTTunnel(x . y) =
   PTTunnel(x) PTTunnel(y) for the coefficient-wise product in O_8; additivity;
 - powBasisPow through lolhip_ext_host.
"""
import numpy as np
import pytest

import crtset_ref as cr
from oracle import lolmath as lm
from test_crtset_host import CASES, IDS, _pps

pytestmark = pytest.mark.gpu

GUARD = 0x6B6B6B6B6B6B
CHAINS = {"8-28-182": [8, 28, 182], "16-56-364": [16, 56, 364]}
_cache = {}


def _tunnel(gpu, name, p, e):
    """(PTTunnel, funcs) of a chain, built once"""
    key = (name, p, e)
    if key not in _cache:
        funcs = cr.tunnel_funcs(CHAINS[name], p, e)
        _cache[key] = (gpu.PTTunnel.for_rings(CHAINS[name], p, e, funcs=funcs), funcs)
    return _cache[key]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_crtset_equals_the_host_path(gpu, case):
    import torch
    m, m2, p, e = case
    got = gpu.crtSet(_pps(m), _pps(m2), p, e)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), gpu.crtSet(_pps(m), _pps(m2), p, e, host=True))


@pytest.mark.parametrize("m,m2,p,e", [(1, 8, 2, 3), (4, 8, 2, 3), (3, 9, 3, 2)])
def test_device_crtset_of_a_p_power_index(gpu, m, m2, p, e):
    """m' a power of p: the set {1}, made on the host (there is no p-free index to plan)"""
    got = gpu.crtSet(_pps(m), _pps(m2), p, e)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), gpu.crtSet(_pps(m), _pps(m2), p, e, host=True))


def test_device_crtset_writes_cap_rows_only(gpu):
    import torch
    from lol_amd.tensor import _pps as arr
    L = gpu.lib()
    (_, a, na), (_, b, nb) = arr([]), arr(_pps(91))
    want = gpu.crtSet([], _pps(91), 2, 3, host=True)
    plan = gpu.Plan(_pps(91), [L.lolhip_crtset_modulus(b, nb, 2, 3)])
    side = torch.cuda.Stream()
    for cap in (1, 4, 6, 9):
        rows = min(cap, 6)
        buf = torch.full((32 + rows * 72 + 32,), GUARD, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert L.lolhip_crtset(plan._h, a, na, b, nb, 2, 3, side.cuda_stream, buf[32:].data_ptr(), cap) == 6
        side.synchronize()
        h = buf.cpu().numpy()
        assert np.array_equal(h[32:32 + rows * 72].reshape(rows, 72), want[:rows])
        assert (h[:32] == GUARD).all() and (h[32 + rows * 72:] == GUARD).all()
    small = gpu.Plan(_pps(91), [lm.first_good_q(91, 100)])                       # a CRT basis, but below the bound
    assert L.lolhip_crtset(small._h, a, na, b, nb, 2, 3, None, None, 0) == -2
    assert L.lolhip_crtset(plan._h, a, na, arr(_pps(7))[1], 1, 2, 3, None, None, 0) == -1   # a plan of another index


def _inputs(rng, n, pe, B, kind):
    if kind == "zero":
        return np.zeros((B, n), dtype=np.int64)
    if kind == "top":
        return np.full((B, n), pe - 1, dtype=np.int64)
    if kind == "unit":
        x = np.zeros((B, n), dtype=np.int64)
        x[np.arange(B), np.arange(B) % n] = 1
        return x
    return rng.integers(0, pe, size=(B, n), dtype=np.int64)


@pytest.mark.parametrize("kind", ["zero", "top", "unit", "rand"])
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("p,e", [(2, 3), (2, 1)], ids=["pe8", "pe2"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_pt_tunnel_is_bit_exact(gpu, name, p, e, B, kind):
    import torch
    rings, pe = CHAINS[name], p ** e
    t, funcs = _tunnel(gpu, name, p, e)
    n0 = lm.totient_pps(_pps(rings[0]))
    x = _inputs(np.random.default_rng(B * 7 + pe), n0, pe, B, kind)
    want = cr.pt_tunnel(rings, funcs, x, pe)
    dx = torch.from_numpy(x).cuda()
    got = t(dx)
    torch.cuda.synchronize()
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(dx.cpu().numpy(), x)                                   # the input is only read
    if kind == "zero":
        assert not want.any()
    if B == 3:
        assert np.array_equal(t(x), want)                                        # numpy in, numpy out
        assert np.array_equal(t(x - pe * (x > 0)), want)                         # any representative mod p^e


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "one-word-off"])
def test_pt_tunnel_side_stream_and_guards(gpu, off):
    """the raw entry on a side stream, out between guard words; one word off a 16-byte boundary takes the 8-byte route of
    k_relift for the first and the last pass"""
    import torch
    rings, p, e, B = CHAINS["8-28-182"], 2, 3, 37
    t, funcs = _tunnel(gpu, "8-28-182", p, e)
    x = np.random.default_rng(off).integers(-8, 9, size=(B, 4), dtype=np.int64)
    want = cr.pt_tunnel(rings, funcs, x, 8)
    xin = torch.zeros(B * 4 + 2, dtype=torch.int64, device="cuda")
    xin[off:off + B * 4] = torch.from_numpy(x).cuda().reshape(-1)
    buf = torch.full((32 + off + want.size + 33,), GUARD, dtype=torch.int64, device="cuda")
    out = buf[32 + off:32 + off + want.size]
    assert out.data_ptr() % 16 == 8 * off
    work = torch.empty((t.workLen(B),), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = gpu.lib().lolhip_pt_tunnel_batch(t._h, side.cuda_stream, xin[off:].data_ptr(), out.data_ptr(), work.data_ptr(), B)
    side.synchronize()
    assert rc == 0
    h = buf.cpu().numpy()
    assert np.array_equal(h[32 + off:32 + off + want.size].reshape(want.shape), want)
    assert (h[:32 + off] == GUARD).all() and (h[32 + off + want.size:] == GUARD).all()


def test_unit_vectors_of_o8_map_to_crt_set_products(gpu):
    """d = (relative decoding basis element i of O_8/O_4) (basis element j0 of O_4): f_0(d) = c0_i j0', and c0_i lies in
    O_7, inside E_1 = O_14, so f_1(f_0(d)) = c0_i f_1(j0') = c0_i c1_i' with i' the relative index of j0' in O_28/O_14"""
    rings, p, e = CHAINS["8-28-182"], 2, 3
    t, funcs = _tunnel(gpu, "8-28-182", p, e)
    got = t(np.eye(4, dtype=np.int64))
    co0 = lm.ext_indices_coeffs(_pps(4), _pps(8))                               # [i][j0] -> index into O_8
    co1 = lm.ext_indices_coeffs(_pps(14), _pps(28))
    co1 = np.array(co1)
    one14 = cr.embed_dec(1, 14, np.array([1], dtype=np.int64), 8)
    c0 = cr.crtset(1, 7, p, e)                                                   # funcs[0] before its embedding
    assert np.array_equal(cr.embed_pow(7, 28, c0), funcs[0])
    R = cr.ring(182)
    seen = set()
    for i in range(2):
        for j0 in range(2):
            unit = np.zeros(2, dtype=np.int64)
            unit[j0] = 1
            up = cr.embed_dec(4, 28, unit, 8)                                    # j0' in the decoding basis of O_28
            ks = [k for k in range(2) if up[co1[k]].any()]                       # its coefficients over O_28/O_14
            assert len(ks) == 1 and np.array_equal(up[co1[ks[0]]], one14)        # a relative basis element times 1
            i1 = ks[0]
            want = R.mul(cr.embed_pow(7, 182, c0[i]), funcs[1][i1], 8)
            assert np.array_equal(got[co0[i][j0]], want)
            seen.add((i, i1))
    assert len(seen) == 4                                                        # four different products


def test_pt_tunnel_multiplies_coefficient_wise_in_o8(gpu):
    """8 -> 28 -> 182 sends the four decoding-basis elements of O_8 to four orthogonal idempotents (the products above),
    so the Z_8 coefficients become slots: PTTunnel(x . y) = PTTunnel(x) PTTunnel(y) for the coefficient-wise product"""
    rings, p, e, B = CHAINS["8-28-182"], 2, 3, 5
    t, _ = _tunnel(gpu, "8-28-182", p, e)
    rng = np.random.default_rng(8)
    RS = cr.ring(182)
    x, y = rng.integers(0, 8, size=(B, 4)), rng.integers(0, 8, size=(B, 4))
    fx, fy, fxy = t(x), t(y), t((x * y) % 8)
    assert fxy.any()
    assert np.array_equal(fxy, np.stack([RS.mul(a, b, 8) for a, b in zip(fx, fy)]))
    one = RS.mul(t(np.ones((1, 4), dtype=np.int64))[0], fx[0], 8)             # the image of (1, 1, 1, 1) acts as 1 on images
    assert np.array_equal(one, fx[0])


@pytest.mark.parametrize("name", list(CHAINS))
def test_pt_tunnel_is_additive(gpu, name):
    rings, p, e, B = CHAINS[name], 2, 3, 5
    t, _ = _tunnel(gpu, name, p, e)
    rng = np.random.default_rng(len(name))
    n0 = lm.totient_pps(_pps(rings[0]))
    x, y = rng.integers(0, 8, size=(B, n0)), rng.integers(0, 8, size=(B, n0))
    assert np.array_equal(t((x + y) % 8), (t(x) + t(y)) % 8)


@pytest.mark.parametrize("m,m2", [(4, 28), (14, 182), (3, 45)])
def test_pow_basis_pow_through_ext_host(gpu, m, m2):
    q = lm.first_good_q(m2, 2 ** 20)
    lo, hi = gpu.Plan(_pps(m), [q]), gpu.Plan(_pps(m2), [q])
    x = gpu.Ext(lo, hi)
    pbp = x.powBasisPow()
    v = np.random.default_rng(m2).integers(0, q, size=(1, hi.n, 1))
    cs = x.coeffs(v)                                                             # [rel][1][n][1]
    acc = np.zeros((1, hi.n, 1), dtype=np.int64)
    for i in range(hi.n // lo.n):
        b = np.zeros((1, hi.n, 1), dtype=np.int64)
        b[0, pbp[i], 0] = 1
        acc = (acc + hi.polymul(x.embedPow(cs[i]), b)) % q
    assert np.array_equal(acc, v)
