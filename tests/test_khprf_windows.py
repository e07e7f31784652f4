"""The slot planner of the key-homomorphic ring PRF on the device, window by window (lolhip_khprf_eval_batch and
lolhip_khprf_batch through the raw C ABI; khprf.hip k_khprf_node, khprf_api.cpp view / layout / eval_node).

The case table is tests/khprf_cases.py; tests/test_khprf_windows_host.py proves without a GPU that it reaches every
class of (root, full, leaf children, full children, slots per right slot against KG, ragged last group) that any tree
with up to six leaves reaches, and every shape of the entry groups (ell mod JG; ell below, at, above JG).  The reference
is the per-input restatement of khprf_ref.py / khprf_lifted_ref.py, computed once per family for the whole domain.

Every call gets `out` with exactly B L n words and `work` with exactly lolhip_khprf_work_len words, each between 32
guard words, `work` filled with a poison pattern: the result must equal the reference slice bit for bit and every guard
word must survive.

    plain, every window     the 9 trees with k <= 4 leaves x every window, at ell = 1, 2, 3, 4, 9
    plain, COVER            the k = 5, 6 cases at ell = 3 and 9
    batch                   the five k = 4 trees, every window, two keys (one as representatives in (-q, 0]), p = 32
    lifted                  q = 8: k <= 3 in full and every second window of k = 4; eval, and batch at p = 2 and 3
    mixed index             8*5*7*13, base 32: lInv on the route of batch
    8-byte route            one COVER case per family kind with out and work one word off a 16-byte boundary, on a side
                            stream: identical words
    index 2                 n = 1: odd word counts (the tail word of k_khprf_lift) and slabs of odd length inside work
"""
import numpy as np
import pytest
import torch

import khprf_cases as kc
import khprf_lifted_ref as klr
import khprf_ref as kr
from oracle import lolmath as lm
from oracle.oracle import Params

pytestmark = pytest.mark.gpu

GUARD_WORDS = 32
GUARD = 0x6A6A6A6A6A6A6A6A
POISON = 0x7E7E7E7E7E7E
SENT = 0x5A5A5A5A5A5A5A5A


class Slab:
    """`cap` payload words of device memory behind GUARD_WORDS guard words; arm(words, fill) leaves exactly `words`
    payload words and guard words everywhere else.  off = 1 puts the payload one word off a 16-byte boundary."""

    def __init__(self, cap, off=0):
        self.buf = torch.empty((off + cap + 2 * GUARD_WORDS,), dtype=torch.int64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.start, self.words = GUARD_WORDS + off, 0
        self.ptr = self.buf.data_ptr() + 8 * self.start
        assert self.ptr % 16 == 8 * off

    def arm(self, words, fill):
        self.words = int(words)
        self.buf.fill_(GUARD)
        self.buf[self.start:self.start + self.words].fill_(fill)

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.words]

    def intact(self):
        return bool((self.buf[:self.start] == GUARD).all() & (self.buf[self.start + self.words:] == GUARD).all())


def tid(x):
    return "-".join(str(v) for v in x) if isinstance(x, (list, tuple)) else str(x)


# ---- families and their references, one per (family, tree), kept for the whole session ---------------------------------
_FAMS = {}


class PlainFam:
    def __init__(self, gpu, cpu, fam, tree):
        m, q, base = fam
        rng = np.random.default_rng([m, q, base] + list(tree))
        pps = lm.factor_pps(m)
        self.q, self.tree, self.dom = q, list(tree), 1 << tree[0]
        self.plan, self.P = gpu.Plan(pps, [q]), Params(pps, [q])
        self.ell, self.n = self.plan.decomposeLen(base), self.P.n
        a0, a1 = (rng.integers(0, q, size=(self.ell, self.n), dtype=np.int64) for _ in range(2))
        self.f = gpu.KHPRF(self.plan, base, self.tree, a0, a1)
        A = np.stack([kr.eval_tree(cpu, self.P, base, self.tree, a0, a1, x) for x in range(self.dom)])
        self.A, self.A_dev = A, torch.from_numpy(A).cuda()
        self.keys = rng.integers(1, q, size=(2, self.n), dtype=np.int64)
        self.cpu, self._prf = cpu, {}
        wire = self.keys.copy()
        wire[1] -= q                                            # the second key as representatives in (-q, 0)
        self.keys_dev = torch.from_numpy(wire).cuda()

    def prf_dev(self, p):
        """[nkeys][dom][ell][n] ringPRF of every input, restated"""
        if p not in self._prf:
            rows = self.A.reshape(-1, self.n, 1)
            want = []
            for s in self.keys:
                sA = self.cpu.mul(self.P, rows, np.ascontiguousarray(np.broadcast_to(s.reshape(1, self.n, 1), rows.shape)))
                want.append(kr.rescale_dec(self.cpu, self.P, sA.reshape(self.A.shape), p))
            self._prf[p] = torch.from_numpy(np.stack(want)).cuda()
        return self._prf[p]


class LiftedFam:
    def __init__(self, gpu, cpu, fam, tree, Q=None):
        m, q, base = fam
        rng = np.random.default_rng([m, q, base, 7] + list(tree))
        self.q, self.tree, self.dom = q, list(tree), 1 << tree[0]
        self.Q = Q or lm.first_good_q(m, klr.bound(m, q, base) + 1)       # the smallest modulus creation certifies
        self.plan, self.plan_Q = gpu.Plan.for_index(m, [q]), gpu.Plan.for_index(m, [self.Q])
        self.ell, self.n = self.plan.decomposeLen(base), self.plan.n
        a0, a1 = (rng.integers(0, q, size=(self.ell, self.n), dtype=np.int64) for _ in range(2))
        a0[0, 0], a1[-1, -1] = q // 2, q // 2 - 1                         # the extremes of the centred lift
        self.a0, self.a1 = a0, a1
        self.f = gpu.KHPRF.lifted(self.plan, self.plan_Q, base, self.tree, a0, a1)
        self.R = klr.LiftedRing(cpu, m, q)
        assert self.R.Qp != self.Q
        A = np.stack([klr.eval_tree(self.R, base, self.tree, a0, a1, x) for x in range(self.dom)])
        self.A, self.A_dev = A, torch.from_numpy(A).cuda()
        self.keys = rng.integers(0, q, size=(2, self.n), dtype=np.int64)
        self.keys[1, : self.n // 2] = q // 2                              # lifts to -q/2
        self.keys_dev = self.f._key_crt(self.keys, 2)                     # centred lift mod Q, CRT basis of Q
        torch.cuda.synchronize()
        self._prf = {}

    def prf_dev(self, p):
        if p not in self._prf:
            want = [[klr.rescale_dec(self.R, self.R.mul(self.A[x], s), p) for x in range(self.dom)] for s in self.keys]
            self._prf[p] = torch.from_numpy(np.asarray(want, dtype=np.int64)).cuda()
        return self._prf[p]


def family(kind, gpu, cpu, fam, tree):
    key = (kind.__name__, tuple(fam), tuple(tree))
    if key not in _FAMS:
        _FAMS[key] = kind(gpu, cpu, fam, tree)
    return _FAMS[key]


# ---- one guarded call ---------------------------------------------------------------------------------------------------
def slabs(F, nkeys=1, off=0):
    """an out and a work slab large enough for every window of the family's tree"""
    ln = F.ell * F.n
    cap = max(kc.work_len(F.tree, F.ell, F.n, x0, B) for x0, B in kc.windows(F.tree[0]))
    return Slab(nkeys * F.dom * ln, off), Slab(cap, off)


def guarded_eval(gpu, F, out, work, x0, B, stream=None):
    wl = F.f.workLen(x0, B)
    assert wl == kc.work_len(F.tree, F.ell, F.n, x0, B)
    out.arm(B * F.ell * F.n, SENT)
    work.arm(wl, POISON)
    rc = gpu.lib().lolhip_khprf_eval_batch(F.f._h, stream, x0, B, out.ptr, work.ptr)
    assert rc == 0, (F.tree, x0, B, rc)
    assert torch.equal(out.payload, F.A_dev[x0:x0 + B].reshape(-1)), ("eval", F.tree, x0, B)
    assert out.intact() and work.intact(), ("eval guards", F.tree, x0, B)


def guarded_batch(gpu, F, out, work, p, x0, B, stream=None):
    wl = F.f.workLen(x0, B)
    out.arm(2 * B * F.ell * F.n, SENT)
    work.arm(wl, POISON)
    rc = gpu.lib().lolhip_khprf_batch(F.f._h, stream, F.keys_dev.data_ptr(), 2, p, x0, B, out.ptr, work.ptr)
    assert rc == 0, (F.tree, p, x0, B, rc)
    assert torch.equal(out.payload, F.prf_dev(p)[:, x0:x0 + B].reshape(-1)), ("batch", F.tree, p, x0, B)
    assert out.intact() and work.intact(), ("batch guards", F.tree, p, x0, B)


# ---- C.1 / C.2: the plain family ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", kc.SWEEP_FAMILIES, ids=tid)
@pytest.mark.parametrize("tree", kc.TREES_K4, ids=tid)
def test_eval_every_window(gpu, cpuref, tree, fam):
    F = family(PlainFam, gpu, cpuref, fam, tree)
    out, work = slabs(F)
    for x0, B in kc.windows(tree[0]):
        guarded_eval(gpu, F, out, work, x0, B)


COVER_TREES = sorted({tuple(t) for t, _, _ in kc.COVER})


@pytest.mark.parametrize("fam", kc.COVER_FAMILIES, ids=tid)
@pytest.mark.parametrize("tree", COVER_TREES, ids=tid)
def test_eval_cover_cases(gpu, cpuref, tree, fam):
    F = family(PlainFam, gpu, cpuref, fam, tree)
    out, work = slabs(F)
    for t, x0, B in kc.COVER:
        if tuple(t) == tree:
            guarded_eval(gpu, F, out, work, x0, B)


# ---- C.3: ringPRF over the windows: the root's value lives in work ----------------------------------------------------------
@pytest.mark.parametrize("tree", kc.all_trees(4), ids=tid)
def test_batch_every_window(gpu, cpuref, tree):
    F = family(PlainFam, gpu, cpuref, (32, 257, 2), tree)
    out, work = slabs(F, nkeys=2)
    for x0, B in kc.windows(4):
        guarded_batch(gpu, F, out, work, 32, x0, B)


@pytest.mark.parametrize("tree", [t for t in kc.TREES_K4 if t[0] <= 3], ids=tid)
def test_mixed_index_every_window(gpu, cpuref, tree):
    """m = 8*5*7*13: the stage programs instead of the two-power kernels, and lInv between crtInv and the rounding"""
    F = family(PlainFam, gpu, cpuref, (kc.M_MIXED, kc.Q_MIXED, 32), tree)
    out, work = slabs(F, nkeys=2)
    for x0, B in kc.windows(tree[0]):
        guarded_eval(gpu, F, out, work, x0, B)
        guarded_batch(gpu, F, out, work, 64, x0, B)


# ---- C.4: the lifted family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", kc.TREES_K4, ids=tid)
def test_lifted_windows(gpu, cpuref, tree):
    F = family(LiftedFam, gpu, cpuref, (32, 8, 2), tree)
    out, work = slabs(F, nkeys=2)
    for t, x0, B in kc.LIFTED:
        if t == tree:
            guarded_eval(gpu, F, out, work, x0, B)
            guarded_batch(gpu, F, out, work, 2, x0, B)
            guarded_batch(gpu, F, out, work, 3, x0, B)


# ---- C.5: slabs that are only 8-byte aligned -------------------------------------------------------------------------------
ROUTE8 = [(PlainFam, (32, 257, 8), kc.T6_LEFT, 3, 58, 32), (PlainFam, (kc.M_MIXED, kc.Q_MIXED, 32), [3, 1, 2, 1, 1], 1, 6, 64),
          (LiftedFam, (32, 8, 2), kc.T6_MID, 3, 26, 3), (LiftedFam, (kc.M_MIXED, 8, 2), [3, 2, 1, 1, 1], 1, 6, 2)]


@pytest.mark.parametrize("kind,fam,tree,x0,B,p", ROUTE8, ids=lambda v: getattr(v, "__name__", None) or tid(v))
def test_eight_byte_aligned_slabs_on_a_side_stream(gpu, cpuref, kind, fam, tree, x0, B, p):
    """the int64_t* of the ABI promise 8-byte alignment only: every pass on the route (node, keymul, round, lift,
    decompose, crt / crtInv, lInv) takes its access width from the pointers it is given"""
    F = family(kind, gpu, cpuref, fam, tree)
    got = []
    side = torch.cuda.Stream()
    for off in (0, 1):
        out, work = slabs(F, nkeys=2, off=off)
        assert out.ptr % 16 == 8 * off and work.ptr % 16 == 8 * off
        with torch.cuda.stream(side):
            guarded_eval(gpu, F, out, work, x0, B, stream=side.cuda_stream)
            e = out.payload.clone()
            guarded_batch(gpu, F, out, work, p, x0, B, stream=side.cuda_stream)
            got.append((e, out.payload.clone()))
        side.synchronize()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---- C.6: index 2, where R_q = Z_q -------------------------------------------------------------------------------------------
def _z_decompose(v, q, base, ell):
    """centred base-`base` digits of the residue v over Z_q (TrivGad for base 0: the lift itself), as residues"""
    x = v - q if 2 * v >= q else v
    if base == 0:
        return [x % q]
    out = []
    for _ in range(ell - 1):
        x, r = (x + base // 2) // base, (x + base // 2) % base - base // 2
        out.append(r % q)
    return out + [x % q]


def _z_eval(tree, q, base, a0, a1, x):
    """A_T(x) over Z_q in Python integers: [ell]"""
    ell = len(a0)

    def sub(x, t):
        if t[0] == "L":
            return list(a1 if x else a0)
        _, _, lt, rt = t
        cr = kr.leaves(rt)
        lv, rv = sub(x >> cr, lt), sub(x & ((1 << cr) - 1), rt)
        dig = [_z_decompose(rv[j], q, base, ell) for j in range(ell)]          # dig[j][i]: digit i of entry j
        return [sum(lv[i] * dig[j][i] for i in range(ell)) % q for j in range(ell)]

    return sub(x, kr.parse(tree))


@pytest.mark.parametrize("base", [0, 2])
def test_index_two_every_window(gpu, cpuref, base):
    """m = 2, n = 1: B L n is odd for odd B L (the tail word of k_khprf_lift), and the node values inside work start at
    odd word offsets"""
    tree, m, q = [3, 2, 1, 1, 1], 2, 8
    Q = lm.first_good_q(m, klr.bound(m, q, base) + 1)
    F = LiftedFam(gpu, cpuref, (m, q, base), tree, Q=Q)
    assert F.n == 1 and F.ell == (1 if base == 0 else 4)        # TrivGad: every odd B is an odd word count
    # R_q = Z_q: the restatement of khprf_lifted_ref against plain integer arithmetic, every input
    l0, l1 = ([int(v) for v in a[:, 0]] for a in (F.a0, F.a1))
    for x in range(8):
        assert [int(v) for v in F.A[x, :, 0]] == _z_eval(tree, q, base, l0, l1, x), x
    for p in (2, 3):
        for j, s in enumerate(F.keys[:, 0]):
            for x in range(8):
                z = [int(a) * int(s) % q for a in F.A[x, :, 0]]
                want = [((p * (v - q if 2 * v >= q else v) + q // 2) // q) % p for v in z]
                assert [int(v) for v in F.prf_dev(p)[j, x, :, 0].cpu()] == want, (p, j, x)
    out, work = slabs(F, nkeys=2)
    for x0, B in kc.windows(3):
        guarded_eval(gpu, F, out, work, x0, B)
        for p in (2, 3):
            guarded_batch(gpu, F, out, work, p, x0, B)
