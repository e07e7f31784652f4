"""Host side of the key-homomorphic lattice PRF (include/lolhip.h lolhip_lprf_*; lol-apps KeyHomomorphicPRF.hs
latticePRF'): no GPU.

 - the entries are exported and declared, lol_amd exports LatticePRF, the LPRF_VALU switch exists;
 - every status of create / work_len / eval_batch / batch on a host-only family, the output untouched;
 - work_len against the restated layout over every window of every tree with <= 4 leaves (khprf_cases.EXHAUSTIVE);
 - the restatement of tests/lprf_ref.py itself: G G^-1(A) = A, a 2-leaf tree against a plain matrix product, key
   homomorphism as KHPRFTests.hs:45-62 at 3 and 5 leaves, and the anchor to the merged ring PRF at n = 1 where the
   oracle accepts that index;
 - both exactness certificates: max|digit| by brute force over all residues, the i32 bound at its edge.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import khprf_cases as kc
import lprf_ref as lr
from oracle import she_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lolhip_lprf_create", "lolhip_lprf_destroy", "lolhip_lprf_n", "lolhip_lprf_ell", "lolhip_lprf_work_len",
       "lolhip_lprf_eval_batch", "lolhip_lprf_batch")
SENT = 0x5A5A5A5A
P61 = 2 ** 61 - 1
I64P = C.POINTER(C.c_int64)


def _family(lolhip, q, base, n, tree):
    z = np.zeros((n, n * lr.ell_of(q, base)), dtype=np.int64)
    return lolhip.LatticePRF(q, base, tree, z, z)


def test_lprf_entries_are_exported_and_declared(lolhip):
    hdr = open(os.path.join(ROOT, "include", "lolhip.h")).read()
    names = set(re.findall(r"LOLHIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", hdr))
    raw = C.CDLL(lolhip.lib_path())
    for nm in NEW:
        assert nm in names, f"include/lolhip.h does not declare {nm}"
        assert hasattr(raw, nm), f"liblolhip.so does not export {nm}"
        assert nm in lolhip._abi.ABI
    assert "LatticePRF" in lolhip.__all__ and hasattr(lolhip, "LatticePRF")
    assert "LPRF_VALU" in hdr
    L = lolhip.lib()
    assert L.lolhip_debug_set(b"LPRF_VALU", 1) == 0 and L.lolhip_debug_set(b"LPRF_VALU", 0) == 0


def test_family_shape(lolhip):
    for q, base, n, ell in ((8, 2, 3, 4), (257, 2, 3, 9), (5, 2, 33, 3), (257, 0, 5, 1), (2 ** 61, 4, 2, 31),
                            (12289, 2, 4, 14)):
        f = _family(lolhip, q, base, n, [2, 1, 1])
        assert (f.n, f.ell, f.K, f.k) == (n, ell, n * ell, 2)
    with pytest.raises(ValueError):
        lolhip.LatticePRF(257, 2, [1], np.zeros((3, 26), dtype=np.int64), np.zeros((3, 26), dtype=np.int64))


@pytest.mark.parametrize("tree", [[], [2, 1], [3, 1, 1, 1], [2, 1, 1, 1], [0], [3, 2, 1, 1], [2, 0, 2], [-1], [63],
                                  [4, 1, 1, 2, 1, 1]])
def test_malformed_trees_are_refused(lolhip, tree):
    z = np.zeros((3, 27), dtype=np.int64)
    with pytest.raises(lolhip.LolHipError) as e:
        lolhip.LatticePRF(257, 2, tree, z, z)
    assert e.value.code == lolhip.tensor.ERR_INVALID


def test_create_statuses(lolhip):
    T, L = lolhip.tensor, lolhip.lib()
    z = np.zeros((3, 27), dtype=np.int64)
    ptr, h, tr = z.ctypes.data_as(I64P), C.c_void_p(), (C.c_int32 * 3)(2, 1, 1)
    mk = lambda q=257, base=2, n=3, t=tr, nt=3, a0=ptr, a1=ptr, out=C.byref(h): L.lolhip_lprf_create(q, base, n, t, nt, a0, a1, out)
    assert mk(n=0) == T.ERR_INVALID
    assert mk(base=1) == T.ERR_INVALID
    assert mk(base=-2) == T.ERR_INVALID
    assert mk(a0=None) == T.ERR_INVALID
    assert mk(a1=None) == T.ERR_INVALID
    assert mk(t=None) == T.ERR_INVALID
    assert mk(out=None) == T.ERR_INVALID
    assert mk(nt=2) == T.ERR_INVALID
    assert mk(q=1) == T.ERR_MODULUS
    assert mk(q=0) == T.ERR_MODULUS
    assert mk(q=-5) == T.ERR_MODULUS
    assert mk(q=2 ** 62) == T.ERR_MODULUS
    # even, 2-power and the widest moduli, TrivGad, one leaf, the largest domain
    _family(lolhip, 2, 2, 1, [1])
    _family(lolhip, 8, 2, 3, lolhip.balanced_tree(5))
    _family(lolhip, 2 ** 62 - 1, 0, 2, [2, 1, 1])
    _family(lolhip, 2 ** 62 - 57, 2, 2, lolhip.left_spine_tree(62))
    with pytest.raises(lolhip.LolHipError):
        _family(lolhip, 257, 2, 3, lolhip.left_spine_tree(63))


def test_work_len_follows_the_layout(lolhip):
    fams = {}
    for tree, x0, B in kc.EXHAUSTIVE:
        for q, base, n in ((8, 2, 3), (257, 0, 2)):
            key = (tuple(tree), q, base, n)
            if key not in fams:
                fams[key] = _family(lolhip, q, base, n, tree)
            f = fams[key]
            for nkeys in (0, 1, 3):
                assert f.workLen(nkeys, x0, B) == lr.work_len(tree, f.n, f.K, nkeys, x0, B), (tree, q, nkeys, x0, B)
    # no per-slot K x K term: a wide family over the full window of a 10-leaf tree stays below B n K words in all
    tree = lolhip.balanced_tree(10)
    f = _family(lolhip, 12289, 2, 16, tree)
    assert f.workLen(0, 0, 1024) == lr.work_len(tree, 16, f.K, 0, 0, 1024) < 1024 * 16 * f.K
    assert f.workLen(2, 0, 0) == 0
    assert _family(lolhip, 257, 2, 3, [1]).workLen(4, 0, 2) == 0
    L = lolhip.lib()
    assert L.lolhip_lprf_work_len(f._h, 0, -1, 1) == -1
    assert L.lolhip_lprf_work_len(f._h, 0, 0, -1) == -1
    assert L.lolhip_lprf_work_len(f._h, 0, 1000, 25) == -1
    assert L.lolhip_lprf_work_len(f._h, -1, 0, 1) == -1
    assert L.lolhip_lprf_work_len(None, 0, 0, 1) == -1


def test_statuses_on_a_host_only_family(lolhip):
    T, L = lolhip.tensor, lolhip.lib()
    if lolhip.device_count() > 0:
        return              # a family made with a device present is not host-only: test_lprf.py checks the statuses there
    q = 2 ** 40 + 15
    f = _family(lolhip, q, 2, 2, lolhip.balanced_tree(3))
    out = np.full((2, 8, f.n, f.K), SENT, dtype=np.int64)
    work = np.zeros(max(f.workLen(2, 0, 8), 1), dtype=np.int64)
    s = np.zeros((2, f.n), dtype=np.int64)
    o, w, sp = out.ctypes.data, work.ctypes.data, s.ctypes.data
    ev = lambda x0, B: L.lolhip_lprf_eval_batch(f._h, None, x0, B, o, w)
    pr = lambda nk, p, x0, B: L.lolhip_lprf_batch(f._h, None, sp, nk, p, x0, B, o, w)
    assert ev(-1, 1) == T.ERR_INVALID
    assert ev(0, -1) == T.ERR_INVALID
    assert ev(7, 2) == T.ERR_INVALID                                    # x0 + B > 2^k
    assert ev(0, 8) == T.ERR_NO_DEVICE
    assert L.lolhip_lprf_eval_batch(None, None, 0, 1, o, w) == T.ERR_INVALID
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


# ---- the restatement itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,base", [(8, 2), (257, 2), (257, 0), (12289, 4), (2 ** 61, 4), (P61, 2), (1000, 10), (97, 128)])
def test_gadget_times_ginv_is_the_identity(q, base):
    rng = np.random.default_rng(q % 1000 + base)
    n, ell = 3, lr.ell_of(q, base)
    A = rng.integers(0, q, size=(n, n * ell), dtype=np.int64)
    D = lr.ginv(q, base, A)                                             # [K][K]
    g = sr.gadget(lr.one_mod(q), base).reshape(ell).astype(object)      # [ell]
    G = np.zeros((n, n * ell), dtype=object)                            # I_n (x) g^t
    for i in range(n):
        G[i, i * ell:(i + 1) * ell] = g
    assert np.array_equal(G.dot(D) % q, A.astype(object))


def test_two_leaf_tree_is_a_plain_matrix_product():
    rng = np.random.default_rng(11)
    q, base, n = 257, 2, 3
    K = n * lr.ell_of(q, base)
    a0, a1 = (rng.integers(0, q, size=(n, K), dtype=np.int64) for _ in range(2))
    a = (a0, a1)
    for x in range(4):
        want = a[x >> 1].astype(object).dot(lr.ginv(q, base, a[x & 1])) % q
        assert np.array_equal(lr.eval_tree(q, base, [2, 1, 1], a0, a1, x), want)
    assert np.array_equal(lr.eval_tree(q, base, [1], a0, a1, 1), a1.astype(object))


@pytest.mark.parametrize("size", [3, 5])
def test_restatement_is_key_homomorphic(size):
    """prop_keyHomom (KHPRFTests.hs:45-62) at the lattice example's shape: n = 3, Zq 257 -> Zq 32, BaseBGad 2, a random
    tree and family, every input of the domain: prf(s1 + s2) - prf(s1) - prf(s2), centred mod p, lies in {-1, 0, 1}"""
    rng = np.random.default_rng(size)
    q, p, base, n = 257, 32, 2, 3
    K = n * lr.ell_of(q, base)
    a0, a1 = (rng.integers(0, q, size=(n, K), dtype=np.int64) for _ in range(2))
    s1, s2 = (rng.integers(0, q, size=(n,), dtype=np.int64) for _ in range(2))

    def rtree(k):
        if k == 1:
            return [1]
        a = int(rng.integers(1, k))
        return [k] + rtree(a) + rtree(k - a)

    tree = rtree(size)
    for x in range(2 ** size):
        f1, f2, f3 = (lr.lattice_prf(q, base, tree, a0, a1, s, p, x) for s in (s1, s2, (s1 + s2) % q))
        d = (f3 - f1 - f2) % p
        d = np.where(2 * d < p, d, d - p)
        assert np.abs(d).max() <= 1, (tree, x)


def test_restatement_at_n_1_is_the_ring_prf_over_z(cpuref):
    """index 2 is R = Z (n = 1): where the CPU oracle and khprf_ref take it, latticePRF at n = 1 is ringPRF there"""
    import khprf_ref as kr
    from oracle.oracle import Params
    q, p, base = 257, 32, 2
    P = Params([(2, 1)], [q])                                           # accepted: a refusal would raise here, not skip
    assert P.n == 1
    rng = np.random.default_rng(5)
    ell = lr.ell_of(q, base)
    a0, a1 = (rng.integers(0, q, size=(1, ell), dtype=np.int64) for _ in range(2))
    s = rng.integers(0, q, size=(1,), dtype=np.int64)
    tree = [4, 1, 3, 2, 1, 1, 1]
    for x in range(16):
        ring = kr.ring_prf(cpuref, P, base, tree, a0.reshape(ell, 1), a1.reshape(ell, 1), s, p, x)
        assert np.array_equal(ring.reshape(ell), lr.lattice_prf(q, base, tree, a0, a1, s, p, x).astype(np.int64)), x


# ---- the certificates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 3, 8, 97, 255, 256, 257, 1000, 12289])
@pytest.mark.parametrize("base", [0, 2, 3, 4, 10, 128, 256, 300])
def test_max_digit_by_brute_force(q, base):
    """the range-end formula bounds every digit of every residue, and is reached whenever there is a remainder digit"""
    got, bound = lr.brute_max_digit(q, base), lr.max_digit(q, base)
    if base == 0 or lr.ell_of(q, base) >= 2:
        assert got == bound
    else:                                                               # base > q: the one digit is the lift itself
        assert got == q // 2 <= bound


def test_route_certificates_at_their_edges():
    # int8 digits: base 254 reaches 127, base 256 reaches 128; TrivGad only below q = 256
    assert lr.max_digit(12289, 254) == 127 and lr.mfma_limbs(12289, 254, 6) > 0
    assert lr.max_digit(12289, 256) == 128 and lr.mfma_limbs(12289, 256, 6) == 0
    assert lr.mfma_limbs(255, 0, 5) == 2 and lr.mfma_limbs(257, 0, 5) == 0
    # the i32 sum: K 128 D < 2^31 holds up to K = 2^17 at D = 127 and fails right above
    assert 2 ** 17 * 128 * 127 < 2 ** 31 <= (2 ** 17 + 1100) * 128 * 127
    assert lr.mfma_limbs(12289, 254, 2 ** 17) > 0 and lr.mfma_limbs(12289, 254, 2 ** 17 + 1100) == 0
    assert lr.mfma_limbs(12289, 2, 2 ** 24 - 1) > 0 and lr.mfma_limbs(12289, 2, 2 ** 24) == 0
    # the host rule adds the measured crossover: the matrix route from K = 56 on
    assert lr.mfma_default(12289, 2, 56) == 2 and lr.mfma_default(12289, 2, 55) == 0 and lr.mfma_default(12289, 256, 56) == 0
    # limbs: the least W with q - 1 <= 127 (256^W - 1) / 255
    assert [lr.mfma_limbs(q, 2, 8) for q in (8, 128, 129, 12289, 32640, 32641, 2 ** 61, 2 ** 62 - 57)] == [1, 1, 2, 2, 2, 3, 8, 8]
    for W in range(1, 9):
        top = 127 * ((256 ** W - 1) // 255)
        assert top + sum(128 * 256 ** j for j in range(W)) < 256 ** W       # x + C keeps W bytes
    # the VALU route's lazy sums never leave int64
    for q, base in ((8, 2), (257, 0), (12289, 2), (2 ** 56 - 5, 2), (2 ** 61, 4), (2 ** 62 - 57, 2), (P61, 0)):
        F, D = lr.valu_fold(q, base), lr.max_digit(q, base)
        assert F == 0 or (F >= 8 and (q - 1) + F * (q - 1) * D <= 2 ** 63 - 1)
    assert lr.valu_fold(2 ** 62 - 57, 2) == 0 and lr.valu_fold(P61, 0) == 0 and lr.valu_fold(2 ** 56 - 5, 2) == 127
