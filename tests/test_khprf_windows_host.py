"""What tests/test_khprf_windows.py relies on, checked without a GPU (-m "not gpu").

  classes    every tree with k <= 6 leaves under every window, classified by khprf_cases.class_key (what the planner of
             khprf_api.cpp and k_khprf_node branch on): 36 classes up to k = 4, 54 up to k = 5, 60 up to k = 6, and
             EXHAUSTIVE + COVER reach every one of them; the lifted sweep reaches all 36 of k <= 4
  families   FAMILIES has the gadget lengths it claims, on the library's own decomposeLen: every ell mod JG, and ell
             below, at and above JG; so do the subsets the GPU file sweeps
  work       lolhip_khprf_work_len of a host-only plain and lifted family equals the restated layout total at every case
  slots      the restated slot maps name valid child slots, are injective per node, agree inside every thread group
             on the right slot, and a node kernel that followed them would compute the per-input recursion: checked on
             symbols (A_v = the tuple of sub-input bits its leaves read) at every case
"""
import numpy as np
import pytest

import khprf_cases as kc
import khprf_lifted_ref as klr
from oracle import lolmath as lm

CASES = kc.EXHAUSTIVE + kc.COVER


def test_tables_have_the_stated_shape():
    assert [len(kc.all_trees(k)) for k in range(1, 7)] == [1, 1, 2, 5, 14, 42]            # Catalan numbers
    assert len(kc.TREES_K4) == 9 and len(kc.EXHAUSTIVE) == 765
    assert len({(tuple(t), x0, B) for t, x0, B in kc.EXHAUSTIVE}) == 765
    for t in kc.TREES_K4:
        assert {(x0, B) for tt, x0, B in kc.EXHAUSTIVE if tt == t} == set(kc.windows(t[0]))
    assert {t[0] for t, _, _ in kc.COVER} == {5, 6}
    for t, x0, B in kc.COVER:
        assert t in kc.all_trees(t[0]) and 0 <= x0 and 1 <= B <= (1 << t[0]) - x0
    assert max(B for _, _, B in CASES) <= 64
    import lol_amd
    for k in range(1, 7):                                   # the library's own shapes are among the generated ones
        for t in (lol_amd.balanced_tree(k), lol_amd.left_spine_tree(k), lol_amd.right_spine_tree(k)):
            assert t in kc.all_trees(k)


def test_case_table_reaches_every_planner_class():
    """the enumeration is the authority: no class that any tree with k <= 6 leaves reaches under any window is left out"""
    upto = {}
    seen = set()
    for k in range(1, 7):
        for t in kc.all_trees(k):
            nodes = kc.parse(t)
            for x0, B in kc.windows(k):
                seen |= kc.classes_of(t, x0, B, nodes)
        upto[k] = len(seen)
    assert upto == {1: 0, 2: 3, 3: 15, 4: 36, 5: 54, 6: 60}
    exhaustive = set().union(*(kc.classes_of(*c) for c in kc.EXHAUSTIVE))
    assert len(exhaustive) == 36
    table = exhaustive | set().union(*(kc.classes_of(*c) for c in kc.COVER))
    assert seen - table == set() and table == seen
    # every field of the key takes both (all three) of its values
    for f in range(6):
        assert {c[f] for c in seen} == {False, True}, f
    assert {c[6] for c in seen} == {"<", "=", ">"} and {c[7] for c in seen} == {False, True}
    # the lifted sweep (k <= 3 in full, every second window of k = 4) reaches what EXHAUSTIVE reaches
    assert {t[0] for t, _, _ in kc.LIFTED} == {1, 2, 3, 4} and len(kc.LIFTED) == 85 + 5 * 68
    assert [c for c in kc.EXHAUSTIVE if c[0][0] <= 3] == kc.LIFTED[:85]
    assert set().union(*(kc.classes_of(*c) for c in kc.LIFTED)) == exhaustive


def test_families_reach_every_entry_group_shape(lolhip):
    assert kc.Q_MIXED == lm.first_good_q(kc.M_MIXED, 2 ** 20)
    ells = {}
    for m, q, base in kc.FAMILIES:
        assert q % m == 1 and lm.is_prime(q)
        ells[(m, q, base)] = lolhip.Plan.for_index(m, [q], host_only=True).decomposeLen(base)
    assert ells == kc.FAMILY_ELL
    assert sorted(set(ells.values())) == [1, 2, 3, 4, 5, 7, 9]
    for fams in (kc.FAMILIES, kc.SWEEP_FAMILIES):
        got = {kc.ell_class(ells[f]) for f in fams}
        assert {r for r, _ in got} == kc.ELL_RESIDUES and {s for _, s in got} == kc.ELL_SIDES
    assert len(kc.SWEEP_FAMILIES) >= 3 and set(kc.SWEEP_FAMILIES) <= set(kc.FAMILIES)
    assert [ells[f] for f in kc.COVER_FAMILIES] == [3, 9]
    assert kc.ell_class(3) == (3, "<") and kc.ell_class(4) == (0, "=") and kc.ell_class(9) == (1, ">")
    # the mixed index has an lInv program (powerful != decoding basis); the two-power index has none
    assert len(lm.factor_pps(kc.M_MIXED)) == 4 and lm.factor_pps(32) == [(2, 5)]


@pytest.mark.parametrize("kind", ["plain", "lifted"])
def test_work_len_equals_the_restated_layout(lolhip, kind):
    if kind == "plain":
        m, q, base = kc.COVER_FAMILIES[0]
        P = lolhip.Plan.for_index(m, [q], host_only=True)
        make = lambda tree, z: lolhip.KHPRF(P, base, tree, z, z)
    else:
        m, q, base = 32, 8, 2
        P = lolhip.Plan.for_index(m, [q], host_only=True)
        PQ = lolhip.Plan.for_index(m, [lm.first_good_q(m, klr.bound(m, q, base) + 1)], host_only=True)
        make = lambda tree, z: lolhip.KHPRF.lifted(P, PQ, base, tree, z, z)
    ell, n = P.decomposeLen(base), P.n
    z = np.zeros((ell, n), dtype=np.int64)
    fams = {}
    for tree, x0, B in CASES:
        f = fams.get(tuple(tree)) or fams.setdefault(tuple(tree), make(tree, z))
        assert f.workLen(x0, B) == kc.work_len(tree, ell, n, x0, B), (tree, x0, B)
    assert all(f.workLen(0, 0) == 0 for f in fams.values())
    assert fams[(1,)].workLen(0, 2) == 0 == kc.work_len([1], ell, n, 0, 2)


def test_layout_regions_are_disjoint_and_fill_the_total():
    for tree, x0, B in CASES:
        nodes = kc.parse(tree)
        val, dig, total = kc.layout(tree, 3, 16, x0, B, nodes)
        spans = [(o, o + (B if i == 0 else kc.view(nodes[i], x0, B)[0]) * 48) for i, o in val.items()]
        spans += [(o, o + 3 * kc.view(nodes[i], x0, B)[0] * 48) for i, o in dig.items()]
        spans.sort()
        assert [a for a, _ in spans] == [0] * bool(spans) + [b for _, b in spans][:-1], (tree, x0, B)
        assert (spans[-1][1] if spans else 0) == total
        internal = [i for i, v in enumerate(nodes) if not v.leaf]
        assert set(val) == set(internal)
        assert set(dig) == {nodes[i].r for i in internal if not nodes[nodes[i].r].leaf}


def test_slot_maps_compute_the_per_input_recursion():
    checked = 0
    for tree, x0, B in CASES:
        nodes = kc.parse(tree)
        for i, v in enumerate(nodes):
            U, lo, full = kc.view(v, x0, B)
            if v.leaf:
                assert (U, full) == (2, True)
                continue
            l, r = nodes[v.l], nodes[v.r]
            assert (l.s, r.s, l.c + r.c) == (v.s + r.c, v.s, v.c)
            if i == 0:
                assert (U, lo, v.s) == (B, x0, 0)               # the root's slots are the window itself
            if full:                                            # a full node has full children
                assert kc.view(l, x0, B)[2] and kc.view(r, x0, B)[2]
            maps = kc.slot_maps(nodes, i, x0, B)
            Ul, Ur = kc.view(l, x0, B)[0], kc.view(r, x0, B)[0]
            assert all(0 <= a < Ul and 0 <= b < Ur for a, b in maps), (tree, x0, B, i)
            # injective: no two slots stand for the same sub-input, and no two read the same pair of child slots
            mask = (1 << v.c) - 1
            subs = [kc.prefix(v, x0, B, k) & mask for k in range(U)]
            assert len(set(subs)) == U and len(set(maps)) == U, (tree, x0, B, i)
            # the sub-inputs are those the window holds
            assert set(subs) == {(x >> v.s) & mask for x in range(x0, x0 + B)}
            # the thread groups partition the slots, and a group has one right slot
            R = kc.shared_R(nodes, i, x0, B)
            groups = kc.thread_groups(U, R)
            assert sorted(k for g in groups for k in g) == list(range(U))
            assert all(len({maps[k][1] for k in g}) == 1 for g in groups), (tree, x0, B, i)
            # a node kernel that follows the maps holds A_v(sub-input) in every slot
            got = kc.slot_values(nodes, i, x0, B)
            assert got == [kc.symbolic(nodes, i, s) for s in subs], (tree, x0, B, i)
            checked += U
        # the root, slot by slot: x0 + k
        if not nodes[0].leaf:
            assert kc.slot_values(nodes, 0, x0, B) == [kc.symbolic(nodes, 0, x) for x in range(x0, x0 + B)]
    assert checked > 10000                                      # slots of internal nodes gone through


def test_symbolic_recursion_reads_every_bit_once():
    """the symbols are what khprf_ref.eval_tree recurses on: leaf number j from the right reads bit j of x"""
    def flat(t):
        return [t] if isinstance(t, int) else flat(t[0]) + flat(t[1])
    for k in range(1, 7):
        for tree in kc.all_trees(k):
            nodes = kc.parse(tree)
            for x in (0, 1, (1 << k) - 1, 0b101101 & ((1 << k) - 1)):
                assert flat(kc.symbolic(nodes, 0, x)) == [(x >> (k - 1 - j)) & 1 for j in range(k)]
