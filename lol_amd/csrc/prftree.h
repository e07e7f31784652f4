// lol_amd/csrc/prftree.h — the tree and the window planner both key-homomorphic PRF families share (khprf_api.cpp: the
// ring PRF, lprf_api.cpp: the lattice PRF; lol-apps KeyHomomorphicPRF.hs FullBinTree, buildDecTree): the parser of the
// preorder leaf-count encoding, a node's view of an input window and the work layout of one call.  Pure host C++.
#pragma once
#include <stdint.h>

#include <vector>

namespace lolhip {

struct PrfNode {
  int c;        // leaves
  int s;        // leaves to its right: the node sees (x >> s) & (2^c - 1)
  int l, r;     // children (-1 for a leaf)
};

// preorder leaf counts -> nodes; returns the index after the subtree at pos, or -1
inline int prf_parse(const int32_t* tree, int ntree, int pos, int s, std::vector<PrfNode>& out, int depth) {
  if (pos >= ntree || depth > 64) return -1;
  const int c = tree[pos];
  const int me = (int)out.size();
  out.push_back(PrfNode{c, s, -1, -1});
  if (c == 1) return pos + 1;
  if (c < 1) return -1;
  // the right subtree's size is known only after the left one is parsed: shifts of the left subtree are fixed after
  const int lpos = pos + 1;
  const int l = (int)out.size();
  int next = prf_parse(tree, ntree, lpos, 0, out, depth + 1);
  if (next < 0) return -1;
  const int cl = out[l].c;
  if (cl >= c) return -1;
  const int cr = c - cl;
  const int r = (int)out.size();
  next = prf_parse(tree, ntree, next, s, out, depth + 1);
  if (next < 0 || out[r].c != cr) return -1;
  out[me].l = l;
  out[me].r = r;
  // the left subtree was parsed with shift 0: it sits cr + s leaves from the right
  for (int i = l; i < r; ++i) out[i].s += s + cr;
  return next;
}

// the whole encoding -> nodes (preorder, nodes[0] the root): false for a malformed tree or more than 62 leaves
inline bool prf_tree(const int32_t* tree, int ntree, std::vector<PrfNode>& out) {
  return tree && ntree >= 1 && ntree <= 123 && prf_parse(tree, ntree, 0, 0, out, 0) == ntree && out[0].c <= 62;
}

inline bool prf_is_leaf(const PrfNode& v) { return v.l < 0; }

// the node's view of the window [x0, x0 + B), B >= 1
struct PrfView { int64_t U, lo; bool full; };
inline PrfView prf_view(const PrfNode& v, int64_t x0, int64_t B) {
  PrfView w;
  w.lo = x0 >> v.s;
  const int64_t span = ((x0 + B - 1) >> v.s) - w.lo + 1;
  const int64_t all = (int64_t)1 << v.c;
  w.U = span < all ? span : all;
  w.full = w.U == all;
  if (v.l < 0) { w.U = 2; w.full = true; }                // a leaf: its two values a0, a1
  return w;
}

// [x0, x0 + B) lies in the domain of a tree of k leaves
inline bool prf_range_ok(int k, int64_t x0, int64_t B) {
  if (x0 < 0 || B < 0) return false;
  const int64_t dom = (int64_t)1 << k;
  return x0 <= dom && B <= dom - x0;
}

// the largest |digit| of decompose over the centred lift mod q with k digits: remainders in [-b/2, b/2], the last digit
// f^(k-1)(v) for v in [-(q div 2), (q - 1) div 2] with f v = floor((v + b/2) / b) monotone; TrivGad (base 0): q div 2
inline uint64_t prf_max_digit(uint64_t q, int64_t base, int k) {
  if (base == 0) return q / 2;
  auto fl = [&](int64_t a) { const int64_t d = a + base / 2; return d >= 0 ? d / base : -((-d + base - 1) / base); };
  int64_t lo = -(int64_t)(q / 2), hi = (int64_t)((q - 1) / 2);
  for (int i = 0; i + 1 < k; ++i) { lo = fl(lo); hi = fl(hi); }
  uint64_t m = (uint64_t)(base / 2);
  if ((uint64_t)(lo < 0 ? -lo : lo) > m) m = (uint64_t)(lo < 0 ? -lo : lo);
  if ((uint64_t)(hi < 0 ? -hi : hi) > m) m = (uint64_t)(hi < 0 ? -hi : hi);
  return m;
}

// work offsets of one call: a value region per internal node below the root (U_v slot words each), a digit region per
// internal right child (dig_mult U_r slot words; none for dig_mult = 0), then root words for the root's region
struct PrfLayout {
  std::vector<int64_t> val, dig;   // per node, -1 where none
  int64_t total = 0;
};
inline PrfLayout prf_layout(const std::vector<PrfNode>& nodes, int64_t x0, int64_t B, int64_t slot, int64_t dig_mult,
                            int64_t root) {
  PrfLayout L;
  const size_t N = nodes.size();
  L.val.assign(N, -1);
  L.dig.assign(N, -1);
  if (B == 0) return L;
  for (size_t i = 1; i < N; ++i) {
    const PrfNode& v = nodes[i];
    if (prf_is_leaf(v)) continue;
    L.val[i] = L.total;
    L.total += prf_view(v, x0, B).U * slot;
  }
  for (size_t i = 0; dig_mult > 0 && i < N; ++i) {
    const PrfNode& v = nodes[i];
    if (prf_is_leaf(v) || prf_is_leaf(nodes[v.r])) continue;
    L.dig[v.r] = L.total;
    L.total += dig_mult * prf_view(nodes[v.r], x0, B).U * slot;
  }
  if (!prf_is_leaf(nodes[0])) {
    L.val[0] = L.total;
    L.total += root;
  }
  return L;
}

}  // namespace lolhip
