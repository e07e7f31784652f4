"""The lifted key-homomorphic ring PRF on the device (lolhip_khprf_create_lifted, q = 2^k), bit-exact against the CPU
restatement of tests/khprf_lifted_ref.py, which computes every product independently of the device method.

 - eval (A_T(x), powerful basis mod q) and ringPRF over q = 8 at m = 128 with 5- and 10-leaf trees, q = 32, and q = 8
   at m = 8*5*7*13 (where lInv sits between the product and the rounding);
 - full domains and unaligned windows, nkeys = 1 and 3, TrivGad and BaseBGad 2 / 4;
 - exactness at the smallest Q creation certifies, with rows and keys of the largest magnitude;
 - a window equals its two halves and the same call on a side stream (numpy and CUDA keys); host statuses leave the
   output untouched.
"""
import numpy as np
import pytest

import khprf_lifted_ref as klr
from oracle import lolmath as lm

pytestmark = pytest.mark.gpu


def _rtree(rng, k):
    if k == 1:
        return [1]
    a = int(rng.integers(1, k))
    return [k] + _rtree(rng, a) + _rtree(rng, k - a)


def _setup(lolhip, cpuref, m, q, base, tree, seed, smallest_Q=False):
    rng = np.random.default_rng(seed)
    need = klr.bound(m, q, base)
    Q = lm.first_good_q(m, need + 1 if smallest_Q else max(need + 1, 2 ** 30))
    Pq, PQ = lolhip.Plan.for_index(m, [q]), lolhip.Plan.for_index(m, [Q])
    nL = Pq.decomposeLen(base)
    a0, a1 = (rng.integers(0, q, size=(nL, Pq.n), dtype=np.int64) for _ in range(2))
    f = lolhip.KHPRF.lifted(Pq, PQ, base, tree, a0, a1)
    R = klr.LiftedRing(cpuref, m, q)
    assert R.Qp != Q
    f.Q = Q
    return f, R, a0, a1, rng


@pytest.mark.parametrize("m,q,base,tname,p", [(128, 8, 2, "balanced10", 2), (128, 32, 2, "right4", 4),
                                              (8 * 5 * 7 * 13, 8, 2, "balanced3", 4)])
def test_lifted_is_exact_at_the_smallest_certified_Q(lolhip, cpuref, m, q, base, tname, p):
    """Q is the first NTT prime above the bound (2689 at F128, q = 8, BaseBGad 2): node and key products stay exact;
    keys and rows of extreme residues (-q/2 everywhere) push the products towards it"""
    tree = _tree(lolhip, np.random.default_rng(m), tname)
    f, R, a0, a1, rng = _setup(lolhip, cpuref, m, q, base, tree, 21, smallest_Q=True)
    assert f.Q <= 2 * klr.bound(m, q, base)
    keys = np.stack([rng.integers(0, q, size=(R.n,), dtype=np.int64), np.full(R.n, q // 2, dtype=np.int64)])
    B = min(1 << tree[0], 40)
    x0 = (1 << tree[0]) - B
    got = f.eval(x0, B).cpu().numpy()
    y = f(keys, p, x0, B).cpu().numpy()
    for b in range(B):
        A = klr.eval_tree(R, base, tree, a0, a1, x0 + b)
        assert np.array_equal(got[b], A), (tree, x0 + b)
        for k in range(2):
            assert np.array_equal(y[k, b], klr.rescale_dec(R, R.mul(A, keys[k]), p)), (tree, x0 + b, k)
    # a family whose rows are all -q/2: every digit of the right values and every left entry at its largest magnitude
    big = np.full((f.L, R.n), q // 2, dtype=np.int64)
    g = lolhip.KHPRF.lifted(f.plan, f.plan_Q, base, tree, big, big)
    got = g.eval(x0, B).cpu().numpy()
    y = g(keys[1], p, x0, B).cpu().numpy()
    for b in range(0, B, 7):
        A = klr.eval_tree(R, base, tree, big, big, x0 + b)
        assert np.array_equal(got[b], A)
        assert np.array_equal(y[b], klr.rescale_dec(R, R.mul(A, keys[1]), p))


CASES = [  # m, q, base, tree, windows
    (128, 8, 2, "balanced5", [(0, 32), (5, 9), (31, 1)]),
    (128, 8, 2, "random10", [(0, 12), (1011, 13), (437, 5)]),
    (128, 32, 2, "random6", [(0, 64), (17, 20)]),
    (128, 8, 0, "right5", [(0, 32)]),
    (64, 16, 4, "left4", [(0, 16), (3, 6)]),
    (8 * 5 * 7 * 13, 8, 2, "balanced3", [(0, 8), (3, 2)]),
]


def _tree(lolhip, rng, name):
    k = int("".join(c for c in name if c.isdigit()))
    if name.startswith("balanced"):
        return lolhip.balanced_tree(k)
    if name.startswith("right"):
        return lolhip.right_spine_tree(k)
    if name.startswith("left"):
        return lolhip.left_spine_tree(k)
    return _rtree(rng, k)


@pytest.mark.parametrize("m,q,base,tname,wins", CASES)
def test_lifted_eval_is_bit_exact(lolhip, cpuref, m, q, base, tname, wins):
    import torch
    tree = _tree(lolhip, np.random.default_rng(m + q), tname)
    f, R, a0, a1, rng = _setup(lolhip, cpuref, m, q, base, tree, 11)
    for x0, B in wins:
        got = f.eval(x0, B).cpu().numpy()
        torch.cuda.synchronize()
        assert got.min() >= 0 and got.max() < q
        for b in range(B):
            want = klr.eval_tree(R, base, tree, a0, a1, x0 + b)
            assert np.array_equal(got[b], want), (tree, x0 + b)


@pytest.mark.parametrize("m,q,base,tname,wins", CASES)
def test_lifted_ring_prf_is_bit_exact(lolhip, cpuref, m, q, base, tname, wins):
    tree = _tree(lolhip, np.random.default_rng(m + q), tname)
    f, R, a0, a1, rng = _setup(lolhip, cpuref, m, q, base, tree, 12)
    p = 2 if q == 8 else 4
    keys = rng.integers(0, q, size=(3, R.n), dtype=np.int64)
    for x0, B in wins:
        many = f(keys, p, x0, B).cpu().numpy()
        one = f(keys[1], p, x0, B).cpu().numpy()
        assert np.array_equal(one, many[1])
        for b in range(B):
            A = klr.eval_tree(R, base, tree, a0, a1, x0 + b)
            for k in range(3):
                want = klr.rescale_dec(R, R.mul(A, keys[k]), p)
                assert np.array_equal(many[k, b], want), (tree, x0 + b, k)


def test_lifted_one_leaf_family(lolhip, cpuref):
    f, R, a0, a1, rng = _setup(lolhip, cpuref, 128, 8, 2, [1], 3)
    got = f.eval(0, 2).cpu().numpy()
    assert np.array_equal(got[0], a0) and np.array_equal(got[1], a1)
    s = rng.integers(0, 8, size=(R.n,), dtype=np.int64)
    y = f(s, 2, 1, 1).cpu().numpy()
    assert np.array_equal(y[0], klr.rescale_dec(R, R.mul(a1, s), 2))


def test_lifted_windows_split_and_side_stream(lolhip, cpuref):
    import torch
    tree = lolhip.balanced_tree(10)
    f, R, a0, a1, rng = _setup(lolhip, cpuref, 128, 8, 2, tree, 4)
    keys = rng.integers(0, 8, size=(2, R.n), dtype=np.int64)
    whole = f.eval(100, 300).cpu().numpy()
    halves = np.concatenate([f.eval(100, 117).cpu().numpy(), f.eval(217, 183).cpu().numpy()])
    assert np.array_equal(whole, halves)
    y = f(keys, 2, 0, 1024).cpu().numpy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y2 = f(keys, 2, 0, 1024, stream=side.cuda_stream)
        e2 = f.eval(100, 300, stream=side.cuda_stream)
    y3 = f(torch.from_numpy(keys).cuda(), 2, 0, 1024, stream=side.cuda_stream)   # a CUDA key, lifted on the device
    side.synchronize()
    assert np.array_equal(y, y2.cpu().numpy())
    assert np.array_equal(y, y3.cpu().numpy())
    assert np.array_equal(whole, e2.cpu().numpy())
    # spot checks of the full domain, x = 0 and x = 1023 included
    for x in (0, 1, 511, 1023):
        want = klr.rescale_dec(R, R.mul(klr.eval_tree(R, 2, tree, a0, a1, x), keys[0]), 2)
        assert np.array_equal(y[0, x], want)


def test_lifted_statuses_leave_the_output_untouched(lolhip, cpuref):
    import torch
    T = lolhip.tensor
    L = lolhip.lib()
    f, R, a0, a1, rng = _setup(lolhip, cpuref, 128, 8, 2, lolhip.balanced_tree(5), 5)
    out = torch.full((2, 32, f.L, R.n), 0x5A5A, dtype=torch.int64, device="cuda")
    work = torch.zeros((max(f.workLen(0, 32), 1),), dtype=torch.int64, device="cuda")
    s = torch.zeros((2, R.n), dtype=torch.int64, device="cuda")
    o, w, sp = out.data_ptr(), work.data_ptr(), s.data_ptr()
    assert L.lolhip_khprf_eval_batch(f._h, None, 0, 33, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_eval_batch(f._h, None, 0, 32, o, None) == T.ERR_INVALID
    assert L.lolhip_khprf_batch(f._h, None, sp, 2, 8, 0, 32, o, w) == T.ERR_MODULUS
    assert L.lolhip_khprf_batch(f._h, None, sp, 0, 2, 0, 32, o, w) == T.ERR_INVALID
    assert L.lolhip_khprf_batch(f._h, None, sp, 2, 2, 30, 3, o, w) == T.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())
