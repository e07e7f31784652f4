"""Host side of the key-homomorphic ring PRF (include/lolhip.h lolhip_khprf_*; lol-apps KeyHomomorphicPRF.hs): no GPU.

 - the new entries are exported and declared, and lol_amd exports KHPRF and the tree helpers;
 - the helpers restate balancedTree / leftSpineTree / rightSpineTree / grayCode;
 - malformed trees, T != 1 and bad bases are refused; q without a CRT basis gives LOLHIP_ERR_NO_CRT;
 - work_len follows the U_v formula of the header;
 - every status of the two compute entries on a host-only family, the output untouched;
 - the restatement of tests/khprf_ref.py passes the reference's prop_keyHomom (m = 32, q = 257, p = 32, BaseBGad 2).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import khprf_ref as kr
from oracle import lolmath as lm
from oracle.oracle import Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_khprf_create", "lolhip_khprf_destroy", "lolhip_khprf_work_len", "lolhip_khprf_eval_batch",
       "lolhip_khprf_batch")
SENT = 0x5A5A5A5A


def _family(lolhip, m, q, base, tree, host_only=True):
    P = lolhip.Plan.for_index(m, [q], host_only=host_only)
    nL = P.decomposeLen(base)
    z = np.zeros((nL, P.n), dtype=np.int64)
    return P, lolhip.KHPRF(P, base, tree, z, z)


def test_khprf_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"
    for nm in ("KHPRF", "balanced_tree", "left_spine_tree", "right_spine_tree", "gray_code"):
        assert nm in lolhip.__all__ and hasattr(lolhip, nm)


def test_tree_helpers_match_the_reference_shapes(lolhip):
    # balancedTree 5 = I 5 (I 4 (I 2 L L) (I 2 L L)) L ... the left subtree takes min(4, 5 - 2) = 3 leaves
    assert lolhip.balanced_tree(5) == [5, 3, 2, 1, 1, 1, 2, 1, 1]
    assert lolhip.balanced_tree(4) == [4, 2, 1, 1, 2, 1, 1]
    assert lolhip.balanced_tree(3) == [3, 2, 1, 1, 1]
    assert lolhip.balanced_tree(1) == [1]
    assert lolhip.left_spine_tree(3) == [3, 2, 1, 1, 1]
    assert lolhip.right_spine_tree(3) == [3, 1, 2, 1, 1]
    assert lolhip.right_spine_tree(1) == lolhip.left_spine_tree(1) == [1]
    assert lolhip.gray_code(1) == [0, 1]
    assert lolhip.gray_code(3) == [0, 1, 3, 2, 6, 7, 5, 4]
    g = lolhip.gray_code(6)
    assert sorted(g) == list(range(64))
    assert all(bin(a ^ b).count("1") == 1 for a, b in zip(g, g[1:]))
    for k in range(1, 20):
        for t in (lolhip.balanced_tree(k), lolhip.left_spine_tree(k), lolhip.right_spine_tree(k)):
            assert len(t) == 2 * k - 1 and t[0] == k
            assert kr.leaves(kr.parse(t)) == k


@pytest.mark.parametrize("tree", [[], [2, 1], [3, 1, 1, 1], [2, 1, 1, 1], [0], [3, 2, 1, 1], [2, 0, 2], [-1],
                                  [63], [4, 1, 1, 2, 1, 1]])
def test_malformed_trees_are_refused(lolhip, tree):
    P = lolhip.Plan.for_index(32, [257], host_only=True)
    z = np.zeros((P.decomposeLen(2), P.n), dtype=np.int64)
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.KHPRF(P, 2, tree, z, z)
    assert e.value.code == lolhip.tensor.ERR_INVALID


def test_create_statuses(lolhip):
    T = lolhip.tensor
    P2 = lolhip.Plan.for_index(32, [257, 353], host_only=True)           # T = 2
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.KHPRF(P2, 2, [1], np.zeros((0, 16)), np.zeros((0, 16)))
    assert e.value.code == T.ERR_INVALID
    P = lolhip.Plan.for_index(32, [257], host_only=True)
    z = np.zeros((9, P.n), dtype=np.int64)
    L = lolhip.lib()
    h = C.c_void_p()
    tr = (C.c_int32 * 1)(1)
    ptr = z.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.lolhip_khprf_create(P._h, 1, tr, 1, ptr, ptr, C.byref(h)) == T.ERR_INVALID          # base 1
    assert L.lolhip_khprf_create(P._h, 2, tr, 1, None, ptr, C.byref(h)) == T.ERR_INVALID
    assert L.lolhip_khprf_create(None, 2, tr, 1, ptr, ptr, C.byref(h)) == T.ERR_INVALID
    # the reference's own toy modulus: Zq 8 has no CRT basis for m = 32
    P8 = lolhip.Plan.for_index(32, [8], host_only=True)
    z8 = np.zeros((P8.decomposeLen(2), P8.n), dtype=np.int64)
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.KHPRF(P8, 2, lolhip.balanced_tree(5), z8, z8)
    assert e.value.code == T.ERR_NO_CRT
    # a one-leaf tree and the largest domain are fine
    _family(lolhip, 32, 257, 2, [1])
    _family(lolhip, 32, 257, 0, lolhip.left_spine_tree(62))
    with pytest.raises(lolhip.LolHipError):
        _family(lolhip, 32, 257, 0, lolhip.left_spine_tree(63))


def _nodes(tree):
    """(c, s, is_leaf, is_internal_right_child) per node: s = leaves to the node's right"""
    out = []

    def rec(t, s, right):
        if t[0] == "L":
            out.append((1, s, True, False))
            return
        _, c, lt, rt = t
        out.append((c, s, False, right))
        rec(lt, s + kr.leaves(rt), False)
        rec(rt, s, True)

    rec(kr.parse(tree), 0, False)
    return out


def _work_len(tree, nL, n, x0, B):
    if B == 0:
        return 0
    tot = 0
    for c, s, leaf, rchild in _nodes(tree):
        if leaf:
            continue
        U = min(2 ** c, ((x0 + B - 1) >> s) - (x0 >> s) + 1)
        tot += U * nL * n + (nL * U * nL * n if rchild else 0)
    return tot


def test_work_len_follows_the_slot_formula(lolhip):
    rng = np.random.default_rng(3)
    for base in (0, 2, 16):
        for tree in (lolhip.balanced_tree(7), lolhip.left_spine_tree(6), lolhip.right_spine_tree(6), [3, 1, 2, 1, 1],
                     [1], [2, 1, 1]):
            P, f = _family(lolhip, 32, 257, base, tree)
            k, nL = tree[0], P.decomposeLen(base)
            wins = [(0, 2 ** k), (0, 1), (2 ** k - 1, 1), (0, 0)] + \
                   [(int(a), int(rng.integers(0, 2 ** k - a + 1))) for a in rng.integers(0, 2 ** k, 6)]
            for x0, B in wins:
                assert f.workLen(x0, B) == _work_len(tree, nL, P.n, x0, B), (tree, base, x0, B)
    # the balanced full-domain tree does about 2^k node products: the root's U = 2^k dominates
    P, f = _family(lolhip, 32, 257, 2, lolhip.balanced_tree(12))
    assert f.workLen(0, 4096) == _work_len(lolhip.balanced_tree(12), 9, 16, 0, 4096)
    L = lolhip.lib()
    assert L.lolhip_khprf_work_len(f._h, -1, 1) == -1
    assert L.lolhip_khprf_work_len(f._h, 0, -1) == -1
    assert L.lolhip_khprf_work_len(f._h, 4000, 97) == -1
    assert L.lolhip_khprf_work_len(None, 0, 1) == -1


def test_statuses_on_a_host_only_family(lolhip):
    T = lolhip.tensor
    L = lolhip.lib()
    q = lm.first_good_q(32, 2 ** 40)
    P, f = _family(lolhip, 32, q, 2, lolhip.balanced_tree(3))
    nL = P.decomposeLen(2)
    out = np.full((2, 8, nL, P.n), SENT, dtype=np.int64)
    work = np.zeros(max(f.workLen(0, 8), 1), dtype=np.int64)
    s = np.zeros((2, P.n), dtype=np.int64)
    o, w, sp = out.ctypes.data, work.ctypes.data, s.ctypes.data
    ev = lambda x0, B: L.lolhip_khprf_eval_batch(f._h, None, x0, B, o, w)
    pr = lambda nk, p, x0, B: L.lolhip_khprf_batch(f._h, None, sp, nk, p, x0, B, o, w)
    assert ev(-1, 1) == T.ERR_INVALID
    assert ev(0, -1) == T.ERR_INVALID
    assert ev(7, 2) == T.ERR_INVALID                                    # x0 + B > 2^k
    assert ev(0, 8) == T.ERR_NO_DEVICE
    assert L.lolhip_khprf_eval_batch(None, None, 0, 1, o, w) == T.ERR_INVALID
    assert pr(0, 32, 0, 8) == T.ERR_INVALID                             # nkeys < 1
    assert pr(1, 32, 5, 4) == T.ERR_INVALID
    assert pr(1, 1, 0, 8) == T.ERR_MODULUS                              # p < 2
    assert pr(1, q, 0, 8) == T.ERR_MODULUS                              # p >= q
    assert pr(1, 2 ** 23, 0, 8) == T.ERR_MODULUS                        # p q >= 2^63
    assert pr(2, 2 ** 22 - 3, 0, 8) == T.ERR_NO_DEVICE                  # p q < 2^63
    assert (out == SENT).all()
    with pytest.raises(lolhip.NoDeviceError):
        f.eval(0, 8)
    with pytest.raises(lolhip.NoDeviceError):
        f(s, 32, 0, 8)


@pytest.mark.parametrize("size", [3, 5])
def test_restatement_is_key_homomorphic(cpuref, size):
    """prop_keyHomom (KHPRFTests.hs) at the reference's shape: m = 32 (decoding = powerful basis), Zq 257 -> Zp 32,
    BaseBGad 2, a random tree and family, every input of the domain"""
    rng = np.random.default_rng(size)
    q, p, base = 257, 32, 2
    P = Params([(2, 5)], [q])
    nL = 9
    a0, a1 = (rng.integers(0, q, size=(nL, P.n), dtype=np.int64) for _ in range(2))
    s1, s2 = (rng.integers(0, q, size=(P.n,), dtype=np.int64) for _ in range(2))
    s3 = (s1 + s2) % q

    def rtree(k):
        if k == 1:
            return [1]
        a = int(rng.integers(1, k))
        return [k] + rtree(a) + rtree(k - a)

    tree = rtree(size)
    for x in range(2 ** size):
        f1, f2, f3 = (kr.ring_prf(cpuref, P, base, tree, a0, a1, s, p, x) for s in (s1, s2, s3))
        d = (f3 - f1 - f2) % p
        d = np.where(2 * d < p, d, d - p)
        assert np.abs(d).max() <= 1, (tree, x)
