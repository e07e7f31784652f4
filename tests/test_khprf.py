"""The key-homomorphic ring PRF on the GPU (lolhip_khprf_eval_batch, lolhip_khprf_batch; lol-apps KeyHomomorphicPRF.hs).

The reference is tests/khprf_ref.py: buildDecTree and ringPRF' restated one input at a time over the CPU oracle, with
none of the device's slot sharing.

    eval_batch      bit-exact A_T(x) (CRT basis) at q = 257 (m = 32, 128), q ~ 2^30 and q ~ 2^60 (two-power m), a
                    mixed index 8*5*7*13 under TrivGad and BaseBGad 32; left-spine, balanced, right-spine, random and
                    one-leaf trees; the full domain, unaligned windows and B = 1
    batch           bit-exact ringPRF for nkeys = 1 and 3
    determinism     [x0, x0 + B) = its two halves; a side stream
    homomorphism    F(s1) + F(s2) - F(s1 + s2) in {-1, 0, 1} per decoding-basis coefficient (= powerful for m = 2^k)
    errors          every status, decided before any launch: the output stays untouched
"""
import numpy as np
import pytest
import torch

import khprf_ref as kr
from oracle import lolmath as lm
from oracle.oracle import Params

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A


def _rtree(rng, k):
    if k == 1:
        return [1]
    a = int(rng.integers(1, k))
    return [k] + _rtree(rng, a) + _rtree(rng, k - a)


class Fam:
    """a device family, its CPU twin, and the restated A_T(x) per x (computed on demand, each input on its own)"""

    def __init__(self, lolhip, m, q, base, tree, seed=0):
        self.rng = np.random.default_rng(seed)
        self.pps = lm.factor_pps(m)
        self.q, self.base, self.tree = q, base, list(tree)
        self.plan = lolhip.Plan(self.pps, [q])
        self.P = Params(self.pps, [q])
        self.nL = self.plan.decomposeLen(base)
        self.a0, self.a1 = (self.rng.integers(0, q, size=(self.nL, self.P.n), dtype=np.int64) for _ in range(2))
        self.f = lolhip.KHPRF(self.plan, base, self.tree, self.a0, self.a1)
        self._A = {}

    def A(self, cpu, x):
        if x not in self._A:
            self._A[x] = kr.eval_tree(cpu, self.P, self.base, self.tree, self.a0, self.a1, x)
        return self._A[x]

    def want_eval(self, cpu, x0, B):
        return np.stack([self.A(cpu, x) for x in range(x0, x0 + B)])

    def want_prf(self, cpu, s, p, x0, B):
        out = []
        for x in range(x0, x0 + B):
            A = self.A(cpu, x)
            sA = cpu.mul(self.P, A.reshape(self.nL, self.P.n, 1),
                         np.ascontiguousarray(np.broadcast_to(s.reshape(1, self.P.n, 1), (self.nL, self.P.n, 1))))
            out.append(kr.rescale_dec(cpu, self.P, sA.reshape(self.nL, self.P.n), p))
        return np.stack(out)


def _windows(k, rng):
    dom = 2 ** k
    w = [(0, dom), (dom - 1, 1), (0, 1)]
    if dom > 4:
        a = int(rng.integers(1, dom // 2))
        w.append((a, int(rng.integers(2, dom - a + 1))))               # unaligned
    return w


def _trees(lolhip, k, rng):
    return [lolhip.left_spine_tree(k), lolhip.balanced_tree(k), lolhip.right_spine_tree(k), _rtree(rng, k)]


@pytest.mark.parametrize("m,k", [(32, 4), (128, 5)])
def test_eval_q257_every_tree(gpu, cpuref, m, k):
    rng = np.random.default_rng(m)
    for i, tree in enumerate(_trees(gpu, k, rng)):
        F = Fam(gpu, m, 257, 2, tree, seed=i)
        for x0, B in _windows(k, rng):
            got = F.f.eval(x0, B).cpu().numpy()
            assert np.array_equal(got, F.want_eval(cpuref, x0, B)), (tree, x0, B)


def test_eval_one_leaf_tree(gpu, cpuref):
    F = Fam(gpu, 64, 257, 2, [1])
    assert np.array_equal(F.f.eval(0, 2).cpu().numpy(), np.stack([F.a0, F.a1]))
    assert np.array_equal(F.f.eval(1, 1).cpu().numpy(), F.a1[None])
    s = np.random.default_rng(1).integers(0, 257, size=(F.P.n,), dtype=np.int64)
    assert np.array_equal(F.f(s, 32, 0, 2).cpu().numpy(), F.want_prf(cpuref, s, 32, 0, 2))


@pytest.mark.parametrize("bits,base,k", [(30, 2, 4), (60, 256, 4), (60, 2, 2)])
def test_eval_wide_moduli(gpu, cpuref, bits, base, k):
    """q ~ 2^30 (64-bit sums folded every few digits) and q ~ 2^60 (128-bit sums)"""
    q = lm.first_good_q(64, 2 ** (bits - 1))
    rng = np.random.default_rng(bits + base)
    for i, tree in enumerate([gpu.balanced_tree(k), _rtree(rng, k)]):
        F = Fam(gpu, 64, q, base, tree, seed=i)
        for x0, B in [(0, 2 ** k), (1, 2)]:
            got = F.f.eval(x0, B).cpu().numpy()
            assert np.array_equal(got, F.want_eval(cpuref, x0, B)), (bits, base, tree, x0, B)


@pytest.mark.parametrize("base", [0, 32])
def test_eval_mixed_index(gpu, cpuref, base):
    m = 8 * 5 * 7 * 13
    q = lm.first_good_q(m, 2 ** 20)
    rng = np.random.default_rng(base)
    for i, tree in enumerate([gpu.balanced_tree(3), gpu.left_spine_tree(3), [1]]):
        F = Fam(gpu, m, q, base, tree, seed=i)
        k = tree[0]
        for x0, B in [(0, 2 ** k), (2 ** k - 1, 1)]:
            got = F.f.eval(x0, B).cpu().numpy()
            assert np.array_equal(got, F.want_eval(cpuref, x0, B)), (base, tree, x0, B)


@pytest.mark.parametrize("m,q,p,base", [(128, 257, 32, 2), (8 * 5 * 7 * 13, None, 64, 32)])
def test_batch_matches_restated_ring_prf(gpu, cpuref, m, q, p, base):
    q = q or lm.first_good_q(m, 2 ** 20)
    rng = np.random.default_rng(7)
    tree = gpu.balanced_tree(4) if m == 128 else gpu.right_spine_tree(3)
    F = Fam(gpu, m, q, base, tree, seed=3)
    k = tree[0]
    s = rng.integers(0, q, size=(3, F.P.n), dtype=np.int64)
    for x0, B in [(0, 2 ** k), (3, 2)]:
        got1 = F.f(s[0], p, x0, B).cpu().numpy()
        assert np.array_equal(got1, F.want_prf(cpuref, s[0], p, x0, B)), (x0, B)
        got3 = F.f(torch.from_numpy(s).cuda(), p, x0, B).cpu().numpy()
        assert got3.shape == (3, B, F.nL, F.P.n)
        for j in range(3):
            assert np.array_equal(got3[j], F.want_prf(cpuref, s[j], p, x0, B)), (j, x0, B)


def test_range_split_and_side_stream(gpu):
    q = lm.first_good_q(256, 2 ** 29)
    for tree in (gpu.balanced_tree(9), gpu.left_spine_tree(8), gpu.right_spine_tree(8)):
        F = Fam(gpu, 256, q, 2, tree, seed=5)
        dom = 2 ** tree[0]
        whole = F.f.eval(0, dom)
        for cut in (1, dom // 2, dom // 3 + 1, dom - 1):
            parts = torch.cat([F.f.eval(0, cut), F.f.eval(cut, dom - cut)])
            assert torch.equal(whole, parts), (tree, cut)
        x0, B = 37, dom // 2 - 11
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = F.f.eval(x0, B, stream=side.cuda_stream)
        side.synchronize()
        assert torch.equal(got, whole[x0:x0 + B])
        s = torch.randint(0, q, (2, F.P.n), dtype=torch.int64, device="cuda")
        ref = F.f(s, 64, x0, B)
        with torch.cuda.stream(side):
            got = F.f(s, 64, x0, B, stream=side.cuda_stream)
        side.synchronize()
        assert torch.equal(got, ref)


@pytest.mark.parametrize("m,q,p", [(128, 257, 32), (2048, None, 2 ** 10), (8 * 5 * 7 * 13, None, 32)])
def test_key_homomorphism_on_device(gpu, m, q, p):
    """F(s1) + F(s2) - F(s1 + s2) in {-1, 0, 1} per decoding-basis coefficient (prop_keyHomom; for m = 2^k the
    decoding basis is the powerful basis, the reference's own check)"""
    q = q or lm.first_good_q(m, 2 ** 30)
    rng = np.random.default_rng(m)
    k = 5
    F = Fam(gpu, m, q, 2, _rtree(rng, k), seed=11)
    s1, s2 = (torch.from_numpy(rng.integers(0, q, size=(F.P.n,), dtype=np.int64)).cuda() for _ in range(2))
    s = torch.stack([s1, s2, (s1 + s2) % q])
    out = F.f(s, p, 0, 2 ** k)
    d = (out[2] - out[0] - out[1]) % p
    d = torch.where(2 * d < p, d, d - p)
    assert int(d.abs().max()) <= 1
    assert int((out >= 0).all()) and int((out < p).all())


def test_statuses_leave_output_untouched(gpu):
    T = gpu.tensor
    L = gpu.lib()
    q = lm.first_good_q(64, 2 ** 40)
    F = Fam(gpu, 64, q, 2, gpu.balanced_tree(4))
    nL, n = F.nL, F.P.n
    out = torch.full((2, 16, nL, n), SENT, dtype=torch.int64, device="cuda")
    work = torch.zeros((F.f.workLen(0, 16),), dtype=torch.int64, device="cuda")
    s = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    o, w, sp = out.data_ptr(), work.data_ptr(), s.data_ptr()
    h = F.f._h
    assert L.lolhip_khprf_eval_batch(h, None, -1, 1, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_eval_batch(h, None, 0, -1, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_eval_batch(h, None, 15, 2, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_eval_batch(h, None, 0, 16, None, w) == T.ERR_INVALID
    assert L.lolhip_khprf_eval_batch(h, None, 0, 16, o, None) == T.ERR_INVALID
    assert L.lolhip_khprf_batch(h, None, sp, 0, 32, 0, 16, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_batch(h, None, sp, 1, 32, 9, 8, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_batch(h, None, None, 1, 32, 0, 16, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_batch(h, None, sp, 1, 1, 0, 16, o, w) == T.ERR_MODULUS
    assert L.lolhip_khprf_batch(h, None, sp, 1, q, 0, 16, o, w) == T.ERR_MODULUS
    assert L.lolhip_khprf_batch(h, None, sp, 2, 2 ** 23, 0, 16, o, w) == T.ERR_MODULUS
    assert L.lolhip_khprf_eval_batch(h, None, 0, 0, None, None) == T.OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    with pytest.raises(gpu.LolHipError):
        F.f.eval(8, 9)
    with pytest.raises(gpu.LolHipError):
        F.f(s, 2 ** 23, 0, 16)
