// lol_amd/csrc/lprf_api.cpp — the C ABI of the key-homomorphic lattice PRF (include/lolhip.h lolhip_lprf_*; lol-apps
// KeyHomomorphicPRF.hs latticePRF' over buildDecTree / evalTree): the family, the exactness certificates of the two
// routes of a node product, the work layout over the planner of prftree.h and the launch plan over lprf.hip.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <memory>
#include <vector>

#include "lprf.h"
#include "prftree.h"
#include "she_host.h"

using namespace lolhip;

struct lolhip_lprf {
  u64 q = 0;
  int64_t base = 0;
  int n = 0, ell = 0, K = 0;     // A in Z_q^(n x K), K = n ell
  int k = 0;                     // leaves
  std::vector<PrfNode> nodes;    // preorder; nodes[0] is the root
  LprfMod md{};
  bool device = false;
  int device_id = -1;
  DevBuf<int64_t> d_leaf;        // [2][n][K]: A0, A1
};

namespace {

bool is_leaf(const PrfNode& v) { return prf_is_leaf(v); }

// the certificates and constants of both routes from (q, base, ell, K); false when K is beyond a launch's reach
//   VALU    signed 64-bit sums: (q - 1) + fold (q - 1) D <= 2^63 - 1 with D = max|digit|; below 8 terms per sum the
//           kernel keeps 128-bit sums of residues instead (fold = 0)
//   matrix  D <= 127 (int8 digits) and K 128 D < 2^31 (an i32 sum of K products of a limb in [-128, 127] and a digit);
//           W = the least count of balanced base-256 limbs that hold q - 1: q - 1 <= 127 (256^W - 1) / 255
void certify(lolhip_lprf& f) {
  LprfMod& md = f.md;
  const u64 D = prf_max_digit(f.q, f.base, f.ell);
  const u128 top = ((u128)1 << 63) - 1 - (f.q - 1), term = (u128)(f.q - 1) * D;
  const u128 F = term ? top / term : top;
  md.fold = F < 8 ? 0 : (int)(F < ((u128)1 << 30) ? F : ((u128)1 << 30));
  if (md.fold && (u128)(f.q - 1) + (u128)md.fold * term > ((u128)1 << 63) - 1) abort();   // the derivation above is wrong
  md.W = 0;
  md.off = 0;
  if (D <= 127 && (u128)f.K * 128 * D < ((u128)1 << 31)) {
    int W = 1;
    while (W < 8 && (u128)(f.q - 1) > (u128)127 * ((((u128)1 << (8 * W)) - 1) / 255)) ++W;
    md.W = W;
    md.off = (((u64)1 << 31) + f.q - 1) / f.q * f.q;
  }
}

int need_device(const lolhip_lprf* f) {
  if (!f->device) return LOLHIP_ERR_NO_DEVICE;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LOLHIP_ERR_HIP;
  return dev == f->device_id ? LOLHIP_OK : LOLHIP_ERR_DEVICE;
}

// the scratch of one call: A_v [U_v][n][K] per internal node below the root, then s A_l [U_l][nkeys][K] of a keyed root
PrfLayout layout(const lolhip_lprf& f, int nkeys, int64_t x0, int64_t B) {
  const int64_t nK = (int64_t)f.n * f.K;
  int64_t root = 0;
  if (B > 0 && nkeys > 0 && !is_leaf(f.nodes[0])) root = prf_view(f.nodes[f.nodes[0].l], x0, B).U * nkeys * f.K;
  return prf_layout(f.nodes, x0, B, nK, 0, root);
}

// the route of a node product: the matrix cores where the certificate admits them and the depth K is at least the
// smallest at which they measured faster on the MI355X (1.3x at K = 56, 6x at K = 3584; at K = 12 and 27 a call is
// bound by its launches and the VALU route was 0 to 6 % ahead: profiles/lprf_bench.jsonl)
constexpr int LPRF_MFMA_MIN_K = 56;
bool use_mfma(const lolhip_lprf& f) { return f.md.W > 0 && f.K >= LPRF_MFMA_MIN_K && !sw(SW_LPRF_VALU); }

struct Call {
  const lolhip_lprf& f;
  hipStream_t s;
  int64_t x0, B;
  const PrfLayout& lay;
  int64_t* work;
  bool info;
  const int64_t* value(int i) const { return is_leaf(f.nodes[i]) ? f.d_leaf.get() : work + lay.val[i]; }
};

// node i from its children's values: Lv [U_l][M][K] (the left child's value, or s times it), rows of slot k at
// dst + k o_slot + i o_row
int product(const Call& c, int i, const int64_t* Lv, int M, int64_t* dst, int64_t o_slot, int64_t o_row, u64 p) {
  const lolhip_lprf& f = c.f;
  const PrfNode& v = f.nodes[i];
  const PrfNode& l = f.nodes[v.l];
  const PrfNode& r = f.nodes[v.r];
  const PrfView vv = prf_view(v, c.x0, c.B), vl = prf_view(l, c.x0, c.B), vr = prf_view(r, c.x0, c.B);
  LprfNode nd{};
  nd.U = i == 0 ? c.B : vv.U;
  nd.lo = vv.lo;
  nd.full = vv.full ? 1 : 0;
  nd.n = f.n; nd.ell = f.ell; nd.M = M; nd.K = f.K;
  nd.R = vr.full ? ((int64_t)1 << r.c) : nd.U;
  nd.o_slot = o_slot; nd.o_row = o_row;
  nd.p = p;
  nd.l = KhprfChild{vl.lo, ((int64_t)1 << l.c) - 1, vl.full ? 1 : 0, r.c};
  nd.r = KhprfChild{vr.lo, ((int64_t)1 << r.c) - 1, vr.full ? 1 : 0, 0};
  return hip_status(launch_lprf_node(c.s, Lv, c.value(v.r), dst, nd, f.md, use_mfma(f), c.info));
}

// A_v for every slot of the internal node i below the root into its work region, post-order
int eval_sub(const Call& c, int i) {
  const PrfNode& v = c.f.nodes[i];
  if (is_leaf(v)) return LOLHIP_OK;
  int rc = eval_sub(c, v.l); if (rc) return rc;
  rc = eval_sub(c, v.r); if (rc) return rc;
  const int64_t nK = (int64_t)c.f.n * c.f.K;
  return product(c, i, c.value(v.l), c.f.n, c.work + c.lay.val[i], nK, c.f.K, 0);
}

}  // namespace

extern "C" {

int lolhip_lprf_create(int64_t q, int64_t base, int n, const int32_t* tree, int ntree, const int64_t* a0,
                       const int64_t* a1, lolhip_lprf** out) {
  if (!tree || !a0 || !a1 || !out || n < 1 || (base != 0 && base < 2)) return LOLHIP_ERR_INVALID;
  if (q < 2 || q >= ((int64_t)1 << 62)) return LOLHIP_ERR_MODULUS;
  std::unique_ptr<lolhip_lprf> f(new lolhip_lprf);
  if (!prf_tree(tree, ntree, f->nodes)) return LOLHIP_ERR_INVALID;
  f->q = (u64)q;
  f->base = base;
  f->n = n;
  f->k = f->nodes[0].c;
  f->ell = 1;
  if (base) { f->ell = 0; for (u64 t = f->q; t != 0; t /= (u64)base) ++f->ell; }   // gadlen (ZqBasic.hs:238-240)
  if ((int64_t)n * f->ell * n >= ((int64_t)1 << 31)) return LOLHIP_ERR_INVALID;
  f->K = n * f->ell;
  LprfMod& md = f->md;
  md.mc = make_modctx(f->q);
  md.dp = DecompParams{};
  md.dp.T = 1; md.dp.L = f->ell; md.dp.base = base; md.dp.k[0] = f->ell;
  md.dp.magic = 1; md.dp.sh1 = md.dp.sh2 = 0;
  md.lg = -1;
  if (base >= 2) {
    inv_div((u64)base, md.dp.magic, md.dp.sh1, md.dp.sh2);
    if ((base & (base - 1)) == 0) md.lg = __builtin_ctzll((u64)base);
  }
  certify(*f);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { *out = f.release(); return LOLHIP_OK; }   // host-only
  if (hipGetDevice(&f->device_id) != hipSuccess) return LOLHIP_ERR_HIP;
  const int64_t nK = (int64_t)n * f->K;
  std::vector<int64_t> a((size_t)(2 * nK));
  for (int64_t i = 0; i < nK; ++i) {
    a[(size_t)i] = (int64_t)canon(a0[i], f->q);
    a[(size_t)(nK + i)] = (int64_t)canon(a1[i], f->q);
  }
  if (int rc = f->d_leaf.upload(a)) return rc;
  f->device = true;
  *out = f.release();
  return LOLHIP_OK;
}

void lolhip_lprf_destroy(lolhip_lprf* f) { delete f; }
int lolhip_lprf_n(const lolhip_lprf* f) { return f ? f->n : LOLHIP_ERR_INVALID; }
int lolhip_lprf_ell(const lolhip_lprf* f) { return f ? f->ell : LOLHIP_ERR_INVALID; }

int64_t lolhip_lprf_work_len(const lolhip_lprf* f, int nkeys, int64_t x0, int64_t B) {
  if (!f || nkeys < 0 || !prf_range_ok(f->k, x0, B)) return LOLHIP_ERR_INVALID;
  return layout(*f, nkeys, x0, B).total;
}

int lolhip_lprf_eval_batch(const lolhip_lprf* f, void* stream, int64_t x0, int64_t B, int64_t* out, int64_t* work) {
  if (!f || !prf_range_ok(f->k, x0, B)) return LOLHIP_ERR_INVALID;
  int rc = need_device(f); if (rc) return rc;
  const PrfLayout lay = layout(*f, 0, x0, B);
  if (B > 0 && (!out || (!work && lay.total > 0))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nK = (int64_t)f->n * f->K;
  if (is_leaf(f->nodes[0]))
    return hip_status(hipMemcpyAsync(out, f->d_leaf + x0 * nK, sizeof(int64_t) * (size_t)(B * nK), hipMemcpyDeviceToDevice, s));
  const Call c{*f, s, x0, B, lay, work, getenv("LOLHIP_LPRF_INFO") != nullptr};
  const PrfNode& root = f->nodes[0];
  rc = eval_sub(c, root.l); if (rc) return rc;
  rc = eval_sub(c, root.r); if (rc) return rc;
  return product(c, 0, c.value(root.l), f->n, out, nK, f->K, 0);
}

int lolhip_lprf_batch(const lolhip_lprf* f, void* stream, const int64_t* keys, int nkeys, int64_t p, int64_t x0, int64_t B,
                      int64_t* out, int64_t* work) {
  if (!f || !prf_range_ok(f->k, x0, B) || nkeys < 1) return LOLHIP_ERR_INVALID;
  if (p < 2 || (u64)p >= f->q || (u128)(u64)p * f->q >= ((u128)1 << 63)) return LOLHIP_ERR_MODULUS;
  int rc = need_device(f); if (rc) return rc;
  const PrfLayout lay = layout(*f, nkeys, x0, B);
  if (B > 0 && (!keys || !out || (!work && lay.total > 0))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nK = (int64_t)f->n * f->K;
  if (is_leaf(f->nodes[0]))                                  // a one-leaf tree: s A_x, rounded
    return hip_status(launch_lprf_keymul(s, f->d_leaf + x0 * nK, keys, out, B, nkeys, f->n, f->K, f->K, B * f->K, (u64)p,
                                         f->md.mc));
  const Call c{*f, s, x0, B, lay, work, getenv("LOLHIP_LPRF_INFO") != nullptr};
  const PrfNode& root = f->nodes[0];
  rc = eval_sub(c, root.l); if (rc) return rc;
  rc = eval_sub(c, root.r); if (rc) return rc;
  // (s A_l) G^-1(A_r): s A_l per left slot first, so the root has nkeys rows per slot and rounds as it writes
  int64_t* sa = work + lay.val[0];
  const int64_t Ul = prf_view(f->nodes[root.l], x0, B).U;
  if (launch_lprf_keymul(s, c.value(root.l), keys, sa, Ul, nkeys, f->n, f->K, (int64_t)nkeys * f->K, f->K, 0, f->md.mc) !=
      hipSuccess)
    return LOLHIP_ERR_HIP;
  return product(c, 0, sa, nkeys, out, f->K, B * f->K, (u64)p);
}

}  // extern "C"
