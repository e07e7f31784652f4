"""Case table of the key-homomorphic ring PRF's slot planner (khprf.hip, khprf_api.cpp): plain data and a restatement
of the slot scheme shared by test_khprf_windows_host.py (coverage and semantics, no GPU), test_khprf_windows.py and
test_khprf_round.py (the kernels themselves).  Pure Python, no imports.

The scheme, as include/lolhip.h (lolhip_khprf_work_len) and the header of khprf.hip document it
    node v with c_v leaves and s_v leaves to its right sees w_v = x >> s_v, of which (x >> s_v) & (2^c_v - 1) matters;
    over the window [x0, x0 + B) it takes U_v = min(2^c_v, ((x0 + B - 1) >> s_v) - (x0 >> s_v) + 1) values and is
    "full" when U_v = 2^c_v; a leaf always holds its two vectors (U = 2, full)
    slot k of v stands for w_v = k (full) or (x0 >> s_v) + k; a child's prefix is w_v >> (s_child - s_v) and its slot
    is prefix & (2^c_child - 1) when the child is full, prefix - (x0 >> s_child) otherwise
    when the right child r is full, slots k, k + R, k + 2R, ... (R = 2^c_r) share one right slot; otherwise R = U_v.
    A thread of k_khprf_node takes KG of the per = ceil(U_v / R) slots of one right slot and JG of the ell entries
    work: U_v ell n words per internal node other than the root, ell U_r ell n per internal right child (its digits),
    and B ell n for the root (lolhip_khprf_batch keeps it there; lolhip_khprf_eval_batch writes it to `out`)

Trees     preorder lists of leaf counts; all_trees(k) generates every full binary tree with k leaves
Classes   class_key(): what the planner and the node kernel branch on, per internal node and window
EXHAUSTIVE  the 9 trees with k <= 4 leaves x every window (x0, B >= 1): 765 windows
COVER       (tree, x0, B) with k = 5 and 6, which with EXHAUSTIVE reach every class that any tree with k <= 6 leaves
            reaches under any window (test_khprf_windows_host.py proves it by enumeration)
FAMILIES    (m, q, base) with gadget lengths 1, 2, 3, 4, 5, 7, 9: every ell mod JG and ell below, at and above JG
"""
KG = 4                                                          # khprf.hip: slots per thread sharing one right slot
JG = 4                                                          # khprf.hip: output entries per thread


# ---- trees ------------------------------------------------------------------------------------------------------------
def all_trees(k):
    """every full binary tree with k leaves, preorder leaf counts, left subtree sizes ascending"""
    if k == 1:
        return [[1]]
    return [[k] + lt + rt for a in range(1, k) for lt in all_trees(a) for rt in all_trees(k - a)]


class Node:
    """one node: c leaves, s leaves to its right, children l, r (indices into the preorder list; -1 for a leaf)"""
    __slots__ = ("c", "s", "l", "r")

    def __init__(self, c, s):
        self.c, self.s, self.l, self.r = c, s, -1, -1

    @property
    def leaf(self):
        return self.l < 0


def parse(tree):
    """preorder leaf counts -> [Node] in preorder (index 0 is the root)"""
    nodes = []

    def rec(pos, s):
        c = tree[pos]
        me = len(nodes)
        nodes.append(Node(c, s))
        if c == 1:
            return pos + 1
        cl = tree[pos + 1]                                      # the left subtree's root follows its parent
        assert 1 <= cl < c, tree
        nodes[me].l = len(nodes)
        nxt = rec(pos + 1, s + (c - cl))
        nodes[me].r = len(nodes)
        nxt = rec(nxt, s)
        assert nodes[nodes[me].r].c == c - cl, tree
        return nxt

    assert rec(0, 0) == len(tree), tree
    return nodes


# ---- the view of a window ---------------------------------------------------------------------------------------------
def view(v, x0, B):
    """(U, lo, full) of node v over [x0, x0 + B), B >= 1"""
    lo = x0 >> v.s
    if v.leaf:
        return 2, lo, True
    U = min(1 << v.c, ((x0 + B - 1) >> v.s) - lo + 1)
    return U, lo, U == 1 << v.c


def prefix(v, x0, B, k):
    """the w_v that slot k of node v stands for"""
    U, lo, full = view(v, x0, B)
    return k if full else lo + k


def child_slot(ch, shift, x0, B, w_v):
    """slot of child ch (s_ch - s_v = shift) for the parent's prefix w_v"""
    _, lo, full = view(ch, x0, B)
    w = w_v >> shift
    return w & ((1 << ch.c) - 1) if full else w - lo


def shared_R(nodes, i, x0, B):
    """R of internal node i: slots k, k + R, ... have one right slot"""
    v = nodes[i]
    r = nodes[v.r]
    return 1 << r.c if view(r, x0, B)[2] else view(v, x0, B)[0]


def slot_maps(nodes, i, x0, B):
    """[(left slot, right slot)] for every slot k < U of internal node i"""
    v = nodes[i]
    l, r = nodes[v.l], nodes[v.r]
    out = []
    for k in range(view(v, x0, B)[0]):
        w = prefix(v, x0, B, k)
        out.append((child_slot(l, r.c, x0, B, w), child_slot(r, 0, x0, B, w)))
    return out


def thread_groups(U, R):
    """the slot groups the threads of k_khprf_node take: per right-slot class k0 < min(R, U), runs of up to KG slots
    k0 + t R of the per = ceil(U / R) that share it (those at or past U dropped)"""
    per = -(-U // R)
    out = []
    for k0 in range(min(R, U)):
        for tg in range(-(-per // KG)):
            kb = k0 + tg * KG * R
            g = [kb + t * R for t in range(KG) if kb + t * R < U]
            if g:
                out.append(g)
    return out


# ---- classes ----------------------------------------------------------------------------------------------------------
def class_key(nodes, i, x0, B):
    """(root?, v full, l leaf, l full, r leaf, r full, per against KG, ragged) of internal node i:
    per against KG is '<', '=' (a positive multiple of KG) or '>' (above KG with a tail); ragged: U % R != 0"""
    v = nodes[i]
    l, r = nodes[v.l], nodes[v.r]
    U, _, full = view(v, x0, B)
    R = shared_R(nodes, i, x0, B)
    per = -(-U // R)
    pk = "<" if per < KG else "=" if per % KG == 0 else ">"
    return (i == 0, full, l.leaf, view(l, x0, B)[2], r.leaf, view(r, x0, B)[2], pk, U % R != 0)


def classes_of(tree, x0, B, nodes=None):
    nodes = nodes or parse(tree)
    return {class_key(nodes, i, x0, B) for i, v in enumerate(nodes) if not v.leaf}


def windows(k):
    """every (x0, B >= 1) inside the domain of k leaves"""
    dom = 1 << k
    return [(x0, B) for x0 in range(dom) for B in range(1, dom - x0 + 1)]


def ell_class(ell):
    """(ell mod JG, ell against JG) of a gadget length: the entry groups of k_khprf_node"""
    return ell % JG, "<" if ell < JG else "=" if ell == JG else ">"


ELL_RESIDUES = {0, 1, 2, 3}
ELL_SIDES = {"<", "=", ">"}


# ---- the work layout --------------------------------------------------------------------------------------------------
def layout(tree, ell, n, x0, B, nodes=None):
    """({node: value offset}, {right child: digit offset}, total) in int64 words; B >= 1.  Values of the internal nodes
    other than the root, then the digits of the internal right children, then the root's value"""
    nodes = nodes or parse(tree)
    ln = ell * n
    val, dig, total = {}, {}, 0
    for i, v in enumerate(nodes):
        if i and not v.leaf:
            val[i] = total
            total += view(v, x0, B)[0] * ln
    for i, v in enumerate(nodes):
        if not v.leaf and not nodes[v.r].leaf:
            dig[v.r] = total
            total += ell * view(nodes[v.r], x0, B)[0] * ln
    if not nodes[0].leaf:
        val[0] = total
        total += B * ln
    return val, dig, total


def work_len(tree, ell, n, x0, B):
    return layout(tree, ell, n, x0, B)[2] if B > 0 else 0


# ---- the per-input recursion, on symbols ------------------------------------------------------------------------------
def symbolic(nodes, i, bits):
    """A_v(bits) as a nested tuple of the sub-input bits each leaf reads: A_leaf(b) = b, A_(I l r)(x) = (A_l(x >> c_r),
    A_r(x & (2^c_r - 1)))"""
    v = nodes[i]
    if v.leaf:
        return bits
    cr = nodes[v.r].c
    return symbolic(nodes, v.l, bits >> cr), symbolic(nodes, v.r, bits & ((1 << cr) - 1))


def slot_values(nodes, i, x0, B):
    """what a node kernel that follows slot_maps would hold in every slot of node i, bottom up from the leaves' (a0, a1)"""
    v = nodes[i]
    if v.leaf:
        return [0, 1]
    lv, rv = slot_values(nodes, v.l, x0, B), slot_values(nodes, v.r, x0, B)
    return [(lv[a], rv[b]) for a, b in slot_maps(nodes, i, x0, B)]


# ---- the tables -------------------------------------------------------------------------------------------------------
TREES_K4 = [t for k in range(1, 5) for t in all_trees(k)]       # 1 + 1 + 2 + 5 = 9 trees
EXHAUSTIVE = [(t, x0, B) for t in TREES_K4 for x0, B in windows(t[0])]

# Chosen by greedy set cover over the enumeration of every tree with 5 and 6 leaves under every window, after the
# classes EXHAUSTIVE reaches were taken out, then filled up with one full-domain and a few unaligned windows per shape.
T6_RIGHT = [6, 1, 5, 4, 2, 1, 1, 2, 1, 1, 1]
T6_LEFT = [6, 4, 2, 1, 1, 2, 1, 1, 2, 1, 1]
T6_MID = [6, 1, 5, 3, 1, 2, 1, 1, 2, 1, 1]
T5_BAL = [5, 3, 1, 2, 1, 1, 2, 1, 1]
T5_RIGHT = [5, 1, 4, 2, 1, 1, 2, 1, 1]
COVER = [
    (T6_RIGHT, 0, 7), (T6_RIGHT, 1, 8), (T6_RIGHT, 7, 18), (T6_RIGHT, 0, 25), (T6_RIGHT, 1, 30), (T6_RIGHT, 0, 1),
    (T6_LEFT, 7, 42), (T6_LEFT, 0, 13), (T6_LEFT, 0, 16), (T6_LEFT, 0, 20), (T6_LEFT, 3, 58), (T6_LEFT, 1, 60),
    (T6_MID, 0, 13), (T6_MID, 0, 16), (T6_MID, 0, 17), (T6_MID, 0, 20), (T6_MID, 3, 26), (T6_MID, 1, 28),
    # not needed for the cover: full domains, the last input alone, and the 5-leaf shapes of the same classes
    (T6_RIGHT, 0, 64), (T6_LEFT, 0, 64), (T6_MID, 0, 64), (T6_MID, 63, 1),
    (T5_BAL, 0, 16), (T5_BAL, 3, 26), (T5_BAL, 1, 28), (T5_BAL, 0, 32), (T5_RIGHT, 0, 1), (T5_RIGHT, 5, 17),
    (T5_RIGHT, 0, 32), (T5_RIGHT, 31, 1),
]

# (m, q, base): index 32 (n = 16) has ell = 1, 2, 3, 4, 5, 9 at q = 257 and 7 at q = 97; the mixed index puts lInv on
# the route of lolhip_khprf_batch (q = the first prime = 1 mod m above 2^20, ell = 5)
M_MIXED = 8 * 5 * 7 * 13
Q_MIXED = 1051961
FAMILIES = [(32, 257, 0), (32, 257, 17), (32, 257, 8), (32, 257, 6), (32, 257, 4), (32, 97, 2), (32, 257, 2),
            (M_MIXED, Q_MIXED, 32)]
FAMILY_ELL = {(32, 257, 0): 1, (32, 257, 17): 2, (32, 257, 8): 3, (32, 257, 6): 4, (32, 257, 4): 5, (32, 97, 2): 7,
              (32, 257, 2): 9, (M_MIXED, Q_MIXED, 32): 5}
# the families test_khprf_windows.py sweeps over every window: ell = 2, 3, 4, 9 reach every ell class but (1, "<")
# and ell = 1 adds that one
SWEEP_FAMILIES = [(32, 257, 0), (32, 257, 17), (32, 257, 8), (32, 257, 6), (32, 257, 2)]
COVER_FAMILIES = [(32, 257, 8), (32, 257, 2)]                   # ell = 3 and 9

# the lifted sweep: every window of the trees with k <= 3 leaves, every second window of the five with k = 4
LIFTED = [c for c in EXHAUSTIVE if c[0][0] <= 3] + \
         [c for t in all_trees(4) for c in [(t, x0, B) for x0, B in windows(4)][1::2]]
