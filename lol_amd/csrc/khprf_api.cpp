// lol_amd/csrc/khprf_api.cpp — the C ABI of the key-homomorphic ring PRF (include/lolhip.h; lol-apps
// KeyHomomorphicPRF.hs buildDecTree / ringPRF'): the tree, the slot planner over an input window and the launch plan
// over the existing crt / crtInv / lInv / decompose and the kernels of khprf.hip.
#include <hip/hip_runtime_api.h>

#include <vector>

#include "capi_internal.h"
#include "pipeline.h"

using namespace lolhip;

namespace {

struct KNode {
  int c;        // leaves
  int s;        // leaves to its right: the node sees (x >> s) & (2^c - 1)
  int l, r;     // children (-1 for a leaf)
};

}  // namespace

struct lolhip_khprf {
  const lolhip_plan* pq = nullptr;
  int64_t base = 0;
  int ell = 0;                   // gadget length L
  int k = 0;                     // leaves
  std::vector<KNode> nodes;      // preorder; nodes[0] is the root
  DecompParams dp{};
  ModCtx mc{};
  int fold = 1;                  // Q32 digits per 64-bit sum of k_khprf_node
  int64_t* d_leaf = nullptr;     // [2][L][n]: a0, a1 (CRT basis)
  int64_t* d_leafdig = nullptr;  // [L][2][L][n]: crt(G^-1(a0)), crt(G^-1(a1)) interleaved as decompose writes them
};

namespace {

// preorder leaf counts -> nodes; returns the index after the subtree at pos, or -1
int parse(const int32_t* tree, int ntree, int pos, int s, std::vector<KNode>& out, int depth) {
  if (pos >= ntree || depth > 64) return -1;
  const int c = tree[pos];
  const int me = (int)out.size();
  out.push_back(KNode{c, s, -1, -1});
  if (c == 1) return pos + 1;
  if (c < 1) return -1;
  // the right subtree's size is known only after the left one is parsed: shifts of the left subtree are fixed after
  const int lpos = pos + 1;
  const int l = (int)out.size();
  int next = parse(tree, ntree, lpos, 0, out, depth + 1);
  if (next < 0) return -1;
  const int cl = out[l].c;
  if (cl >= c) return -1;
  const int cr = c - cl;
  const int r = (int)out.size();
  next = parse(tree, ntree, next, s, out, depth + 1);
  if (next < 0 || out[r].c != cr) return -1;
  out[me].l = l;
  out[me].r = r;
  // the left subtree was parsed with shift 0: it sits cr + s leaves from the right
  for (int i = l; i < r; ++i) out[i].s += s + cr;
  return next;
}

bool is_leaf(const KNode& v) { return v.l < 0; }

// the node's view of the window [x0, x0 + B), B >= 1
struct View { int64_t U, lo; bool full; };
View view(const KNode& v, int64_t x0, int64_t B) {
  View w;
  w.lo = x0 >> v.s;
  const int64_t span = ((x0 + B - 1) >> v.s) - w.lo + 1;
  const int64_t all = (int64_t)1 << v.c;
  w.U = span < all ? span : all;
  w.full = w.U == all;
  if (v.l < 0) { w.U = 2; w.full = true; }                // a leaf: its two vectors a0, a1
  return w;
}

// work offsets of one call: values of every internal node (root last) and digits of every internal right child
struct Layout {
  std::vector<int64_t> val, dig;   // per node, -1 where none
  int64_t total = 0;
};
Layout layout(const lolhip_khprf& f, int64_t x0, int64_t B) {
  Layout L;
  const size_t N = f.nodes.size();
  L.val.assign(N, -1);
  L.dig.assign(N, -1);
  if (B == 0) return L;
  const int64_t ln = (int64_t)f.ell * f.pq->P.n;
  for (size_t i = 1; i < N; ++i) {
    const KNode& v = f.nodes[i];
    if (is_leaf(v)) continue;
    const int64_t U = view(v, x0, B).U;
    L.val[i] = L.total;
    L.total += U * ln;
  }
  for (size_t i = 0; i < N; ++i) {
    const KNode& v = f.nodes[i];
    if (is_leaf(v) || is_leaf(f.nodes[v.r])) continue;
    const int64_t Ur = view(f.nodes[v.r], x0, B).U;
    L.dig[v.r] = L.total;
    L.total += (int64_t)f.ell * Ur * ln;
  }
  if (!is_leaf(f.nodes[0])) {
    L.val[0] = L.total;
    L.total += B * ln;
  }
  return L;
}

bool range_ok(const lolhip_khprf* f, int64_t x0, int64_t B) {
  if (!f || x0 < 0 || B < 0) return false;
  const int64_t dom = (int64_t)1 << f->k;
  return x0 <= dom && B <= dom - x0;
}

bool q_below31(const Plan& P) { return P.qs[0] < ((u64)1 << 31); }

// A_v for every slot of node i into dst ([U][L][n]), post-order
int eval_node(const lolhip_khprf& f, hipStream_t s, int i, int64_t x0, int64_t B, const Layout& lay, int64_t* work,
              int64_t* dst) {
  const Plan& P = f.pq->P;
  const KNode& v = f.nodes[i];
  const KNode& l = f.nodes[v.l];
  const KNode& r = f.nodes[v.r];
  const int64_t ln = (int64_t)f.ell * P.n;
  if (!is_leaf(l)) { int rc = eval_node(f, s, v.l, x0, B, lay, work, work + lay.val[v.l]); if (rc) return rc; }
  const View vv = view(v, x0, B), vl = view(l, x0, B), vr = view(r, x0, B);
  const int64_t* D = f.d_leafdig;
  if (!is_leaf(r)) {
    int64_t* rv = work + lay.val[v.r];
    int64_t* rd = work + lay.dig[v.r];
    int rc = eval_node(f, s, v.r, x0, B, lay, work, rv); if (rc) return rc;
    // G^-1: crtInv of the U_r L entries, their digits [L][U_r L][n], crt of the L U_r L digit polynomials
    rc = capi_do_crt(P, s, rv, vr.U * f.ell, true); if (rc) return rc;
    if (launch_decompose(s, rv, rd, vr.U * f.ell, P.n, f.dp, P.d_mod, q_below31(P)) != hipSuccess) return LOLHIP_ERR_HIP;
    rc = capi_do_crt(P, s, rd, (int64_t)f.ell * vr.U * f.ell, false); if (rc) return rc;
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
  return launch_khprf_node(s, Lv, D, dst, nd, f.mc, f.fold) == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP;
}

// A_T(x) for the window into dst [B][L][n] (B >= 1)
int eval_root(const lolhip_khprf& f, hipStream_t s, int64_t x0, int64_t B, int64_t* work, int64_t* dst) {
  const int64_t ln = (int64_t)f.ell * f.pq->P.n;
  if (is_leaf(f.nodes[0]))
    return hipMemcpyAsync(dst, f.d_leaf + x0 * ln, sizeof(int64_t) * (size_t)(B * ln), hipMemcpyDeviceToDevice, s)
                   == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP;
  const Layout lay = layout(f, x0, B);
  return eval_node(f, s, 0, x0, B, lay, work, dst);
}

void free_dev(lolhip_khprf* f) {
  if (f->d_leaf) (void)hipFree(f->d_leaf);
  if (f->d_leafdig) (void)hipFree(f->d_leafdig);
  f->d_leaf = f->d_leafdig = nullptr;
}

// a0 | a1 -> d_leaf; crtInv, decompose and crt into d_leafdig (on a private stream, synchronised)
int upload(lolhip_khprf* f, const std::vector<int64_t>& a) {
  const Plan& P = f->pq->P;
  const size_t words = a.size();                           // 2 L n
  if (hipMalloc(&f->d_leaf, words * sizeof(int64_t)) != hipSuccess) return LOLHIP_ERR_HIP;
  if (hipMalloc(&f->d_leafdig, (size_t)f->ell * words * sizeof(int64_t)) != hipSuccess) return LOLHIP_ERR_HIP;
  int64_t* tmp = nullptr;
  if (hipMalloc(&tmp, words * sizeof(int64_t)) != hipSuccess) return LOLHIP_ERR_HIP;
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipFree(tmp); return LOLHIP_ERR_HIP; }
  int rc = LOLHIP_OK;
  if (hipMemcpyAsync(f->d_leaf, a.data(), words * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(tmp, f->d_leaf, words * sizeof(int64_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = LOLHIP_ERR_HIP;
  if (!rc) rc = capi_do_crt(P, s, tmp, 2 * f->ell, true);
  if (!rc && launch_decompose(s, tmp, f->d_leafdig, 2 * f->ell, P.n, f->dp, P.d_mod, q_below31(P)) != hipSuccess)
    rc = LOLHIP_ERR_HIP;
  if (!rc) rc = capi_do_crt(P, s, f->d_leafdig, 2 * (int64_t)f->ell * f->ell, false);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = LOLHIP_ERR_HIP;
  (void)hipStreamDestroy(s);
  (void)hipFree(tmp);
  return rc;
}

}  // namespace

extern "C" {

int lolhip_khprf_create(const lolhip_plan* pq, int64_t base, const int32_t* tree, int ntree, const int64_t* a0_crt,
                        const int64_t* a1_crt, lolhip_khprf** out) {
  if (!pq || !tree || !a0_crt || !a1_crt || !out || ntree < 1 || ntree > 123) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (P.T != 1) return LOLHIP_ERR_INVALID;
  lolhip_khprf* f = new lolhip_khprf;
  f->pq = pq;
  f->base = base;
  int rc = capi_make_decomp(P, base, f->dp);
  if (!rc && (parse(tree, ntree, 0, 0, f->nodes, 0) != ntree || f->nodes[0].c > 62)) rc = LOLHIP_ERR_INVALID;
  if (!rc && !P.has_crt) rc = LOLHIP_ERR_NO_CRT;
  if (rc) { delete f; return rc; }
  f->ell = f->dp.L;
  f->k = f->nodes[0].c;
  const u64 q = P.qs[0];
  f->mc = make_modctx(q);
  if (q < ((u64)1 << 32)) {                                // (q-1) + fold (q-1)^2 < 2^64
    const u64 q1 = q - 1, sq = q1 * q1;
    const u64 F = (~(u64)0 - q1) / sq;
    f->fold = (int)(F < (u64)f->ell ? F : (u64)f->ell);
  } else {
    f->fold = 8;
  }
  rc = capi_need_device(pq);
  if (rc == LOLHIP_ERR_NO_DEVICE) { *out = f; return LOLHIP_OK; }      // host-only: validation and work lengths
  if (rc) { delete f; return rc; }
  const int64_t ln = (int64_t)f->ell * P.n;
  std::vector<int64_t> a((size_t)(2 * ln));
  for (int64_t i = 0; i < ln; ++i) {
    const int64_t x0 = a0_crt[i] % (int64_t)q, x1 = a1_crt[i] % (int64_t)q;
    a[i] = x0 < 0 ? x0 + (int64_t)q : x0;
    a[ln + i] = x1 < 0 ? x1 + (int64_t)q : x1;
  }
  rc = upload(f, a);
  if (rc) { free_dev(f); delete f; return rc; }
  *out = f;
  return LOLHIP_OK;
}

void lolhip_khprf_destroy(lolhip_khprf* f) {
  if (!f) return;
  free_dev(f);
  delete f;
}

int64_t lolhip_khprf_work_len(const lolhip_khprf* f, int64_t x0, int64_t B) {
  if (!range_ok(f, x0, B)) return LOLHIP_ERR_INVALID;
  return layout(*f, x0, B).total;
}

int lolhip_khprf_eval_batch(const lolhip_khprf* f, void* stream, int64_t x0, int64_t B, int64_t* out, int64_t* work) {
  if (!range_ok(f, x0, B)) return LOLHIP_ERR_INVALID;
  int rc = capi_need_device(f->pq); if (rc) return rc;
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
  int rc = capi_need_device(f->pq); if (rc) return rc;
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
    A = root;
  }
  const int64_t rows = (int64_t)nkeys * B * f->ell;
  if (launch_khprf_keymul(s, A, s_crt, out, nkeys, B * f->ell, P.n, f->mc) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = capi_do_crt(P, s, out, rows, true); if (rc) return rc;
  if (!P.prog_linv.stages.empty()) { rc = capi_run_prog(P, P.prog_linv, s, out, rows, nullptr); if (rc) return rc; }
  return launch_khprf_round(s, out, rows * P.n, p, f->mc) == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP;
}

}  // extern "C"
