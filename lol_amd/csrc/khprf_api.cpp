// lol_amd/csrc/khprf_api.cpp — the C ABI of the key-homomorphic ring PRF (include/lolhip.h; lol-apps
// KeyHomomorphicPRF.hs buildDecTree / ringPRF'): the family and the launch plan over the existing crt / crtInv / lInv /
// decompose and the kernels of khprf.hip.  The tree and the slot planner over an input window are prftree.h's, shared
// with the lattice PRF (lprf_api.cpp).
//
// The lifted family (lolhip_khprf_create_lifted) runs over q = 2^k, which has no CRT basis: every node product is
// computed exactly over the integers in the CRT basis mod an NTT prime Q (certified at creation) and brought back to
// Z_q before it is used again.  The Q-side values sit where the one-modulus family keeps its CRT values; decompose and
// lInv run on the plan mod q.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "prftree.h"
#include "she_host.h"

using namespace lolhip;

struct lolhip_khprf {
  const lolhip_plan* pq = nullptr;
  const lolhip_plan* pQ = nullptr;  // the lifted family: products mod Q in its CRT basis; nullptr otherwise
  KhprfLift lc{};                // the lifted family: Q, q = 2^qbits
  int64_t base = 0;
  int ell = 0;                   // gadget length L
  int k = 0;                     // leaves
  std::vector<PrfNode> nodes;    // preorder; nodes[0] is the root
  DecompParams dp{};
  ModCtx mc{};
  int fold = 1;                  // Q32 digits per 64-bit sum of k_khprf_node
  DevBuf<int64_t> d_leaf;        // [2][L][n]: a0, a1 (CRT basis)
  DevBuf<int64_t> d_leafdig;     // [L][2][L][n]: crt(G^-1(a0)), crt(G^-1(a1)) interleaved as decompose writes them
  DevBuf<int64_t> d_leafpow;     // the lifted family: [2][L][n] a0, a1 in the powerful basis mod q (a one-leaf A_T)
};

namespace {

using KNode = PrfNode;
using View = PrfView;
using Layout = PrfLayout;
bool is_leaf(const KNode& v) { return prf_is_leaf(v); }
View view(const KNode& v, int64_t x0, int64_t B) { return prf_view(v, x0, B); }

// work offsets of one call: values of every internal node (root last) and digits of every internal right child
Layout layout(const lolhip_khprf& f, int64_t x0, int64_t B) {
  const int64_t ln = (int64_t)f.ell * f.pq->P.n;
  return prf_layout(f.nodes, x0, B, ln, f.ell, B * ln);
}

bool range_ok(const lolhip_khprf* f, int64_t x0, int64_t B) { return f && prf_range_ok(f->k, x0, B); }

bool q_below31(const Plan& P) { return P.qs[0] < ((u64)1 << 31); }

// LOLHIP_OK, or why the family cannot compute on the calling thread's current device (both plans of a lifted one)
int need_device(const lolhip_khprf* f) {
  const int rc = lolhip::need_device(f->pq);
  return rc || !f->pQ ? rc : lolhip::need_device(f->pQ);
}

// Q32 digits per 64-bit sum of k_khprf_node for products mod q: (q-1) + fold (q-1)^2 < 2^64
int fold_for(u64 q, int ell) {
  if (q >= ((u64)1 << 32)) return 8;
  const u64 q1 = q - 1, sq = q1 * q1;
  const u64 F = (~(u64)0 - q1) / sq;
  return (int)(F < (u64)ell ? F : (u64)ell);
}

// A_v for every slot of node i into dst ([U][L][n]), post-order
// the lifted family: `rows` node values mod Q, CRT basis -> crtInv -> reduce mod q -> lift_q mod Q -> crt, in place
int requantize(const lolhip_khprf& f, hipStream_t s, int64_t* y, int64_t rows) {
  const Plan& PQ = f.pQ->P;
  int rc = do_crt(PQ, s, y, rows, true); if (rc) return rc;
  if (launch_khprf_lift(s, y, y, rows * PQ.n, LIFT_FROM_Q | LIFT_TO_Q, f.lc) != hipSuccess) return LOLHIP_ERR_HIP;
  return do_crt(PQ, s, y, rows, false);
}

int eval_node(const lolhip_khprf& f, hipStream_t s, int i, int64_t x0, int64_t B, const Layout& lay, int64_t* work,
              int64_t* dst) {
  const Plan& P = f.pq->P;
  const Plan& PC = f.pQ ? f.pQ->P : P;                     // where the products and their crt / crtInv live
  const KNode& v = f.nodes[i];
  const KNode& l = f.nodes[v.l];
  const KNode& r = f.nodes[v.r];
  const int64_t ln = (int64_t)f.ell * P.n;
  const View vv = view(v, x0, B), vl = view(l, x0, B), vr = view(r, x0, B);
  if (!is_leaf(l)) {
    int rc = eval_node(f, s, v.l, x0, B, lay, work, work + lay.val[v.l]); if (rc) return rc;
    if (f.pQ) { rc = requantize(f, s, work + lay.val[v.l], vl.U * f.ell); if (rc) return rc; }
  }
  const int64_t* D = f.d_leafdig;
  if (!is_leaf(r)) {
    int64_t* rv = work + lay.val[v.r];
    int64_t* rd = work + lay.dig[v.r];
    int rc = eval_node(f, s, v.r, x0, B, lay, work, rv); if (rc) return rc;
    // G^-1: crtInv of the U_r L entries, their digits [L][U_r L][n], crt of the L U_r L digit polynomials
    rc = do_crt(PC, s, rv, vr.U * f.ell, true); if (rc) return rc;
    if (f.pQ && launch_khprf_lift(s, rv, rv, vr.U * ln, LIFT_FROM_Q, f.lc) != hipSuccess) return LOLHIP_ERR_HIP;
    if (launch_decompose(s, rv, rd, vr.U * f.ell, P.n, f.dp, P.d_mod, q_below31(P)) != hipSuccess) return LOLHIP_ERR_HIP;
    const int64_t drows = (int64_t)f.ell * vr.U * f.ell;
    if (f.pQ && launch_khprf_lift(s, rd, rd, drows * P.n, LIFT_TO_Q, f.lc) != hipSuccess) return LOLHIP_ERR_HIP;
    rc = do_crt(PC, s, rd, drows, false); if (rc) return rc;
    D = rd;
  }
  KhprfNode nd{};
  nd.U = i == 0 ? B : vv.U;
  nd.lo = vv.lo;
  nd.full = vv.full ? 1 : 0;
  nd.ell = f.ell;
  nd.n = P.n;
  nd.R = vr.full ? ((int64_t)1 << r.c) : nd.U;
  nd.d_digit = vr.U * ln;
  nd.l = KhprfChild{vl.lo, ((int64_t)1 << l.c) - 1, vl.full ? 1 : 0, r.c};
  nd.r = KhprfChild{vr.lo, ((int64_t)1 << r.c) - 1, vr.full ? 1 : 0, 0};
  const int64_t* Lv = is_leaf(l) ? f.d_leaf : work + lay.val[v.l];
  return hip_status(launch_khprf_node(s, Lv, D, dst, nd, f.mc, f.fold));
}

// A_T(x) for the window into dst [B][L][n] (B >= 1): CRT basis, or powerful basis mod q for the lifted family
int eval_root(const lolhip_khprf& f, hipStream_t s, int64_t x0, int64_t B, int64_t* work, int64_t* dst) {
  const int64_t ln = (int64_t)f.ell * f.pq->P.n;
  if (is_leaf(f.nodes[0])) {
    const int64_t* src = (f.pQ ? f.d_leafpow : f.d_leaf) + x0 * ln;
    return hip_status(hipMemcpyAsync(dst, src, sizeof(int64_t) * (size_t)(B * ln), hipMemcpyDeviceToDevice, s));
  }
  const Layout lay = layout(f, x0, B);
  int rc = eval_node(f, s, 0, x0, B, lay, work, dst);
  if (rc || !f.pQ) return rc;
  rc = do_crt(f.pQ->P, s, dst, B * f.ell, true); if (rc) return rc;
  return hip_status(launch_khprf_lift(s, dst, dst, B * ln, LIFT_FROM_Q, f.lc));
}

// a0 | a1 -> d_leaf; crtInv, decompose and crt into d_leafdig (on a private stream, synchronised)
int upload(lolhip_khprf* f, const std::vector<int64_t>& a) {
  const Plan& P = f->pq->P;
  const size_t words = a.size();                           // 2 L n
  DevBuf<int64_t> tmp;
  if (f->d_leaf.alloc(words) || f->d_leafdig.alloc((size_t)f->ell * words) || tmp.alloc(words)) return LOLHIP_ERR_HIP;
  ScopedStream s;                                          // after every buffer it touches: drained before tmp is freed
  if (!s.ok()) return LOLHIP_ERR_HIP;
  int rc = LOLHIP_OK;
  if (hipMemcpyAsync(f->d_leaf, a.data(), words * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(tmp, f->d_leaf, words * sizeof(int64_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = LOLHIP_ERR_HIP;
  if (!rc) rc = do_crt(P, s, tmp, 2 * f->ell, true);
  if (!rc && launch_decompose(s, tmp, f->d_leafdig, 2 * f->ell, P.n, f->dp, P.d_mod, q_below31(P)) != hipSuccess)
    rc = LOLHIP_ERR_HIP;
  if (!rc) rc = do_crt(P, s, f->d_leafdig, 2 * (int64_t)f->ell * f->ell, false);
  const int rs = s.sync();                                 // a is read until here
  return rc ? rc : rs;
}

// the lifted family: a0 | a1 (powerful, [0, q)) -> d_leafpow; crt_Q (lift_q a) -> d_leaf; decompose mod q, lift_q and
// crt_Q into d_leafdig (on a private stream, synchronised)
int upload_lifted(lolhip_khprf* f, const std::vector<int64_t>& a) {
  const Plan& P = f->pq->P;
  const Plan& PQ = f->pQ->P;
  const size_t words = a.size();                           // 2 L n
  const int64_t dwords = (int64_t)f->ell * (int64_t)words;
  if (f->d_leafpow.alloc(words) || f->d_leaf.alloc(words) || f->d_leafdig.alloc((size_t)dwords)) return LOLHIP_ERR_HIP;
  ScopedStream s;
  if (!s.ok()) return LOLHIP_ERR_HIP;
  int rc = LOLHIP_OK;
  if (hipMemcpyAsync(f->d_leafpow, a.data(), words * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
      launch_khprf_lift(s, f->d_leafpow, f->d_leaf, (int64_t)words, LIFT_TO_Q, f->lc) != hipSuccess ||
      launch_decompose(s, f->d_leafpow, f->d_leafdig, 2 * f->ell, P.n, f->dp, P.d_mod, q_below31(P)) != hipSuccess ||
      launch_khprf_lift(s, f->d_leafdig, f->d_leafdig, dwords, LIFT_TO_Q, f->lc) != hipSuccess)
    rc = LOLHIP_ERR_HIP;
  if (!rc) rc = do_crt(PQ, s, f->d_leaf, 2 * f->ell, false);
  if (!rc) rc = do_crt(PQ, s, f->d_leafdig, 2 * (int64_t)f->ell * f->ell, false);
  const int rs = s.sync();
  return rc ? rc : rs;
}

}  // namespace

extern "C" {

int lolhip_khprf_create(const lolhip_plan* pq, int64_t base, const int32_t* tree, int ntree, const int64_t* a0_crt,
                        const int64_t* a1_crt, lolhip_khprf** out) {
  if (!pq || !tree || !a0_crt || !a1_crt || !out || ntree < 1 || ntree > 123) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (P.T != 1) return LOLHIP_ERR_INVALID;
  std::unique_ptr<lolhip_khprf> f(new lolhip_khprf);
  f->pq = pq;
  f->base = base;
  int rc = make_decomp(P, base, f->dp);
  if (!rc && !prf_tree(tree, ntree, f->nodes)) rc = LOLHIP_ERR_INVALID;
  if (!rc && !P.has_crt) rc = LOLHIP_ERR_NO_CRT;
  if (rc) return rc;
  f->ell = f->dp.L;
  f->k = f->nodes[0].c;
  const u64 q = P.qs[0];
  f->mc = make_modctx(q);
  f->fold = fold_for(q, f->ell);
  rc = need_device(pq);
  if (rc == LOLHIP_ERR_NO_DEVICE) { *out = f.release(); return LOLHIP_OK; }      // host-only: validation and work lengths
  if (rc) return rc;
  const int64_t ln = (int64_t)f->ell * P.n;
  std::vector<int64_t> a((size_t)(2 * ln));
  for (int64_t i = 0; i < ln; ++i) {
    a[i] = (int64_t)canon(a0_crt[i], q);
    a[ln + i] = (int64_t)canon(a1_crt[i], q);
  }
  rc = upload(f.get(), a);
  if (rc) return rc;
  *out = f.release();
  return LOLHIP_OK;
}

int lolhip_khprf_create_lifted(const lolhip_plan* pq, const lolhip_plan* pQ, int64_t base, const int32_t* tree,
                               int ntree, const int64_t* a0_pow, const int64_t* a1_pow, lolhip_khprf** out) {
  if (!pq || !pQ || !tree || !a0_pow || !a1_pow || !out || ntree < 1 || ntree > 123) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  const Plan& PQ = pQ->P;
  if (P.T != 1 || PQ.T != 1 || !same_index(P, PQ)) return LOLHIP_ERR_INVALID;
  std::unique_ptr<lolhip_khprf> f(new lolhip_khprf);
  f->pq = pq;
  f->pQ = pQ;
  f->base = base;
  int rc = make_decomp(P, base, f->dp);
  if (!rc && !prf_tree(tree, ntree, f->nodes)) rc = LOLHIP_ERR_INVALID;
  const u64 q = P.qs[0], Q = PQ.qs[0];
  if (!rc && (q < 2 || (q & (q - 1)) != 0)) rc = LOLHIP_ERR_MODULUS;
  if (!rc && !PQ.has_crt) rc = LOLHIP_ERR_NO_CRT;
  if (rc) return rc;
  f->ell = f->dp.L;
  f->k = f->nodes[0].c;
  // exactness over Z: |sum_i L_i digit_i| <= L C_m (q/2) max|digit| and |s A| <= C_m (q/2)^2 below Q/2
  auto sat = [](u128 a, u128 b) -> u128 { const u128 cap = (u128)1 << 100; return a >= cap || b >= cap || a * b >= cap ? cap : a * b; };
  const u128 C = growth(P.pps), h = q / 2;
  const u128 node = sat(sat(sat((u128)f->ell, C), h), prf_max_digit(q, base, f->dp.k[0]));
  const u128 key = sat(sat(C, h), h);
  if (2 * std::max(node, key) >= (u128)Q) return LOLHIP_ERR_MODULUS;
  f->lc.Q = Q;
  f->lc.qbits = __builtin_ctzll(q);
  f->mc = make_modctx(Q);
  f->fold = fold_for(Q, f->ell);
  rc = need_device(f.get());
  if (rc == LOLHIP_ERR_NO_DEVICE) { *out = f.release(); return LOLHIP_OK; }      // host-only: validation and work lengths
  if (rc) return rc;
  const int64_t ln = (int64_t)f->ell * P.n;
  std::vector<int64_t> a((size_t)(2 * ln));
  for (int64_t i = 0; i < ln; ++i) {
    a[i] = (int64_t)((u64)a0_pow[i] & (q - 1));
    a[ln + i] = (int64_t)((u64)a1_pow[i] & (q - 1));
  }
  rc = upload_lifted(f.get(), a);
  if (rc) return rc;
  *out = f.release();
  return LOLHIP_OK;
}

void lolhip_khprf_destroy(lolhip_khprf* f) { delete f; }

int64_t lolhip_khprf_work_len(const lolhip_khprf* f, int64_t x0, int64_t B) {
  if (!range_ok(f, x0, B)) return LOLHIP_ERR_INVALID;
  return layout(*f, x0, B).total;
}

int lolhip_khprf_eval_batch(const lolhip_khprf* f, void* stream, int64_t x0, int64_t B, int64_t* out, int64_t* work) {
  if (!range_ok(f, x0, B)) return LOLHIP_ERR_INVALID;
  int rc = need_device(f); if (rc) return rc;
  if (B > 0 && (!out || (!work && layout(*f, x0, B).total > 0))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  return eval_root(*f, (hipStream_t)stream, x0, B, work, out);
}

// s A_T(x) for every key (CRT basis) -> crtInv -> lInv -> rescaleMod to Z_p, all in out
int lolhip_khprf_batch(const lolhip_khprf* f, void* stream, const int64_t* s_crt, int nkeys, int64_t p, int64_t x0,
                       int64_t B, int64_t* out, int64_t* work) {
  if (!range_ok(f, x0, B) || nkeys < 1) return LOLHIP_ERR_INVALID;
  const u64 q = f->pq->P.qs[0];
  if (p < 2 || (u64)p >= q || (unsigned __int128)(u64)p * q >= ((unsigned __int128)1 << 63)) return LOLHIP_ERR_MODULUS;
  int rc = need_device(f); if (rc) return rc;
  const Layout lay = layout(*f, x0, B);
  if (B > 0 && (!s_crt || !out || (!work && lay.total > 0))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  const Plan& P = f->pq->P;
  hipStream_t s = (hipStream_t)stream;
  const int64_t ln = (int64_t)f->ell * P.n;
  const int64_t* A = f->d_leaf + x0 * ln;                  // a one-leaf tree: a0 / a1 themselves
  if (!is_leaf(f->nodes[0])) {
    int64_t* root = work + lay.val[0];
    rc = eval_node(*f, s, 0, x0, B, lay, work, root); if (rc) return rc;
    if (f->pQ) { rc = requantize(*f, s, root, B * f->ell); if (rc) return rc; }
    A = root;
  }
  const int64_t rows = (int64_t)nkeys * B * f->ell;
  if (launch_khprf_keymul(s, A, s_crt, out, nkeys, B * f->ell, P.n, f->mc) != hipSuccess) return LOLHIP_ERR_HIP;
  const bool linv = !P.prog_linv.stages.empty();
  if (f->pQ) {
    // exact s A mod Q -> Z_q (fused with the 2-power rounding when there is no lInv between them)
    rc = do_crt(f->pQ->P, s, out, rows, true); if (rc) return rc;
    KhprfLift lc = f->lc;
    lc.p = (u64)p;
    if (linv) {
      if (launch_khprf_lift(s, out, out, rows * P.n, LIFT_FROM_Q, lc) != hipSuccess) return LOLHIP_ERR_HIP;
      rc = run_prog(P, P.prog_linv, s, out, rows, nullptr); if (rc) return rc;
    }
    return hip_status(launch_khprf_lift(s, out, out, rows * P.n, (linv ? 0 : LIFT_FROM_Q) | LIFT_ROUND, lc));
  }
  rc = do_crt(P, s, out, rows, true); if (rc) return rc;
  rc = run_prog_or_copy(P, P.prog_linv, s, out, rows); if (rc) return rc;
  return hip_status(launch_khprf_round(s, out, rows * P.n, p, f->mc));
}

}  // extern "C"
