// lol_amd/csrc/pttunnel_api.cpp — the C ABI of crtSetDec / crtSet and of the clear-text tunnel (include/lolhip.h; lol-cpp
// CPP/Extension.hs:143-164, lol UCyc.hs:540-565, lol-apps HomomPRF.hs:510-531).  The number theory is crtset.cpp's; this
// file validates, certifies the exactness bounds and lays the launch plans over the existing l / lInv / crt / crtInv /
// poly-mul / evalLin and the two kernels of pttunnel.hip.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "crtset.h"
#include "pttunnel.h"
#include "she_host.h"

using namespace lolhip;

struct lolhip_pt_tunnel {
  int nhops = 0;
  std::vector<const lolhip_ext*> er, es;
  Relift rl{};                       // p^e; Qin / Qout are set per launch
  std::vector<DevBuf<int64_t>> d_ys; // per hop [rel][n_S]: crt mod Q_h of the centred lift of f_h's values
  bool device = false;
  int64_t n_max = 0;
};

namespace {

// work: a hop's input and its output [B][n_max], rounded, swapped hop by hop | what each hop's evalLin carves
struct PtTunnelWork { int64_t *a, *b, *ev; };
PtTunnelWork pt_tunnel_work(Work& w, const lolhip_pt_tunnel& c, int64_t B) {
  PtTunnelWork r = {w.take(even(B * c.n_max)), w.take(even(B * c.n_max)), nullptr};
  const int64_t m = w.mark();
  for (int h = 0; h < c.nhops; ++h) {
    w.rewind(m);
    r.ev = evallin_work(w, c.er[(size_t)h]->X, c.es[(size_t)h]->X, B).tmp_e;
  }
  return r;
}

// K rows of n words -> min(K, cap) rows of out
int64_t copy_rows(const std::vector<i64>& src, int64_t K, int64_t* out, int64_t cap) {
  if (K > 0 && out && cap > 0) {
    const int64_t n = (int64_t)src.size() / K;
    std::memcpy(out, src.data(), sizeof(int64_t) * (size_t)(std::min(K, cap) * n));
  }
  return K;
}

Relift make_relift(u64 pe) {
  Relift r{};
  r.pe = make_modctx(pe);
  r.pebits = (pe & (pe - 1)) == 0 ? __builtin_ctzll(pe) : 0;
  return r;
}

// twice rel C_S G_S D_R floor(pe/2)^2 (the hop's modulus must exceed it), or LOLHIP_ERR_MODULUS from 2^61 on
int64_t hop_bound(const std::vector<PP>& r, const std::vector<PP>& s, int64_t rel, bool first, u64 pe) {
  const u128 cap = (u128)1 << 61;
  u128 v = 2 * (u128)rel;
  auto mul = [&](u128 f) { v = (v >= cap || f >= cap || v * f >= cap) ? cap : v * f; };
  mul(growth(s));
  for (const PP& pe_s : s) if (pe_s.p != 2) mul((u128)(pe_s.p - 1));
  if (!first) for (const PP& pe_r : r) if (pe_r.p != 2) mul(2);
  mul(pe / 2);
  mul(pe / 2);
  return v >= cap ? (int64_t)LOLHIP_ERR_MODULUS : (int64_t)v;
}

}  // namespace

extern "C" {

int64_t lolhip_crtset_dec(const lolhip_pp* pps_m, int npps_m, const lolhip_pp* pps_m2, int npps_m2, int64_t p,
                          int64_t* out, int64_t cap) {
  std::vector<PP> a, b;
  if (!to_pps(pps_m, npps_m, a) || !to_pps(pps_m2, npps_m2, b) || cap < 0) return LOLHIP_ERR_INVALID;
  if (!out || cap == 0) return crtset_count(a, b, p);
  std::vector<i64> x;
  return copy_rows(x, crtset_dec(a, b, p, x), out, cap);
}

int64_t lolhip_crtset_modulus(const lolhip_pp* pps_m2, int npps_m2, int64_t p, int e) {
  std::vector<PP> b;
  if (!to_pps(pps_m2, npps_m2, b)) return LOLHIP_ERR_INVALID;
  return crtset_modulus(b, p, e);
}

int64_t lolhip_crtset_host(const lolhip_pp* pps_m, int npps_m, const lolhip_pp* pps_m2, int npps_m2, int64_t p, int e,
                           int64_t* out, int64_t cap) {
  std::vector<PP> a, b;
  if (!to_pps(pps_m, npps_m, a) || !to_pps(pps_m2, npps_m2, b) || cap < 0 || (cap > 0 && !out)) return LOLHIP_ERR_INVALID;
  std::vector<i64> x;
  return copy_rows(x, crtset_host(a, b, p, e, x), out, cap);
}

int64_t lolhip_crtset(const lolhip_plan* pQ, const lolhip_pp* pps_m, int npps_m, const lolhip_pp* pps_m2, int npps_m2,
                      int64_t p, int e, void* stream, int64_t* out_dev, int64_t cap) {
  std::vector<PP> a, b;
  if (!pQ || e < 1 || !to_pps(pps_m, npps_m, a) || !to_pps(pps_m2, npps_m2, b) || cap < 0 || (cap > 0 && !out_dev))
    return LOLHIP_ERR_INVALID;
  std::vector<MergedPP> mp;
  if (!merge_pps(a, b, mp)) return LOLHIP_ERR_INVALID;
  const std::vector<PP> bar = strip_prime(a, p), bar2 = strip_prime(b, p);
  const int64_t K = crtset_count(bar, bar2, p);
  if (K < 0) return K;
  const u64 pe = pow_below62((u64)p, e);
  if (!pe) return LOLHIP_ERR_MODULUS;
  const Plan& P = pQ->P;
  if (P.T != 1 || !same_pps(P.pps, bar2)) return LOLHIP_ERR_INVALID;
  const u64 Q = P.qs[0];
  if (Q >= ((u64)1 << 61) || !crtset_bound_ok(bar2, (u64)p, pe, Q)) return LOLHIP_ERR_MODULUS;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  int rc = need_device(pQ); if (rc) return rc;
  const int64_t rows = std::min(K, cap);
  if (rows == 0) return K;
  ExtTables X;
  if (!build_ext_tables(bar2, b, X)) return LOLHIP_ERR_INVALID;
  std::vector<i64> dec;
  const int64_t K2 = crtset_dec(bar, bar2, p, dec);
  if (K2 != K) return K2 < 0 ? K2 : (int64_t)LOLHIP_ERR_INVALID;
  const int64_t nb = P.n, n2 = X.phi2, words = K * nb;
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int64_t> bx, by;
  DevBuf<int32_t> bi;
  if (bx.alloc(std::max<size_t>((size_t)words, 1)) || by.alloc(std::max<size_t>((size_t)words, 1)) ||
      bi.alloc(std::max<size_t>((size_t)n2, 2)))         // at least 8 bytes each
    return LOLHIP_ERR_HIP;
  int64_t *x = bx, *y = by;
  Relift rl = make_relift(pe);
  rl.Qin = rl.Qout = Q;
  auto hip = [](hipError_t err) { return err == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP; };
  rc = hip(hipMemcpyAsync(x, dec.data(), sizeof(int64_t) * (size_t)words, hipMemcpyHostToDevice, s));
  if (!rc) rc = hip(hipMemcpyAsync(bi, X.embed_pow.data(), sizeof(int32_t) * (size_t)n2, hipMemcpyHostToDevice, s));
  // the decoding-basis residues in [0, p) -> powerful basis (prefix sums below Q/2) -> centred lift of the class mod p^e
  if (!rc) rc = run_prog_or_copy(P, P.prog_l, s, x, K);
  if (!rc) rc = hip(launch_relift(s, x, nullptr, x, words, rl));
  for (int step = 1; step < e && nb > 1 && !rc; ++step) {    // index 1: the set is {1}
    rc = hip(hipMemcpyAsync(y, x, sizeof(int64_t) * (size_t)words, hipMemcpyDeviceToDevice, s));
    for (int64_t t = 1; t < p && !rc; ++t) {
      rc = lolhip_polymul_batch(pQ, s, y, y, x, K);
      if (!rc) rc = hip(launch_relift(s, y, nullptr, y, words, rl));
    }
    std::swap(x, y);
  }
  if (!rc) rc = hip(launch_relift(s, x, y, nullptr, words, rl));
  if (!rc) rc = hip(launch_embed_rows(s, y, out_dev, bi, rows, nb, n2));
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = LOLHIP_ERR_HIP;   // also on error: the buffers are freed next
  return rc ? rc : K;
}

int64_t lolhip_pt_tunnel_modulus(const lolhip_pp* pps_r, int npps_r, const lolhip_pp* pps_s, int npps_s, int64_t rel,
                                 int first_hop, int64_t p, int e) {
  std::vector<PP> r, s;
  if (!to_pps(pps_r, npps_r, r) || !to_pps(pps_s, npps_s, s) || rel < 1 || e < 1) return LOLHIP_ERR_INVALID;
  if (p < 2) return LOLHIP_ERR_MODULUS;
  const u64 pe = pow_below62((u64)p, e);
  if (!pe) return LOLHIP_ERR_MODULUS;
  return hop_bound(r, s, rel, first_hop != 0, pe);
}

void lolhip_pt_tunnel_destroy(lolhip_pt_tunnel* c) { delete c; }

int lolhip_pt_tunnel_create(int nhops, const lolhip_ext* const* x_er, const lolhip_ext* const* x_es,
                            const int64_t* const* funcs_pow, int64_t p, int e, lolhip_pt_tunnel** out) {
  if (!out || !x_er || !x_es || !funcs_pow || nhops < 1 || nhops > 16 || e < 1) return LOLHIP_ERR_INVALID;
  *out = nullptr;
  for (int h = 0; h < nhops; ++h) if (!x_er[h] || !x_es[h] || !funcs_pow[h]) return LOLHIP_ERR_INVALID;
  if (p < 2) return LOLHIP_ERR_MODULUS;
  const u64 pe = pow_below62((u64)p, e);
  if (!pe) return LOLHIP_ERR_MODULUS;
  bool device = true;
  int64_t n_max = x_er[0]->X.host.phi2;
  for (int h = 0; h < nhops; ++h) {
    const ExtPlan &ER = x_er[h]->X, &ES = x_es[h]->X;
    if (ER.lo->T != 1 || ES.lo->T != 1 || !same_index(*ER.lo, *ES.lo) || ER.lo->qs != ES.lo->qs) return LOLHIP_ERR_INVALID;
    if (h + 1 < nhops && !same_index(*ES.hi, *x_er[h + 1]->X.hi)) return LOLHIP_ERR_INVALID;
    if (!ES.hi->has_crt) return LOLHIP_ERR_NO_CRT;
    const int64_t bound = hop_bound(ER.hi->pps, ES.hi->pps, ER.host.phi2 / ER.host.phi, h == 0, pe);
    if (bound < 0) return (int)bound;
    const u64 Q = ES.hi->qs[0];
    if (Q <= (u64)bound || Q < pe || Q >= ((u64)1 << 61)) return LOLHIP_ERR_MODULUS;
    device = device && ER.d_coeffs && ES.d_embed_dec && ES.hi->device && ER.hi->device;
    n_max = std::max(n_max, (int64_t)ES.host.phi2);
  }
  std::unique_ptr<lolhip_pt_tunnel> c(new lolhip_pt_tunnel);
  c->nhops = nhops;
  c->er.assign(x_er, x_er + nhops);
  c->es.assign(x_es, x_es + nhops);
  c->rl = make_relift(pe);
  c->n_max = n_max;
  c->device = device;
  c->d_ys.resize((size_t)nhops);
  if (!device) { *out = c.release(); return LOLHIP_OK; }            // host-only: validation and work lengths
  int rc = need_device(*x_es[0]->X.hi); if (rc) return rc;
  std::vector<std::vector<int64_t>> host((size_t)nhops);           // alive until the stream has drained
  ScopedStream s;                                                  // after c and host: drained before either goes
  if (!s.ok()) return LOLHIP_ERR_HIP;
  for (int h = 0; h < nhops && !rc; ++h) {
    const ExtPlan &ER = x_er[h]->X, &ES = x_es[h]->X;
    const Plan& S = *ES.hi;
    const int64_t rel = ER.host.phi2 / ER.host.phi, words = rel * S.n;
    const u64 Q = S.qs[0];
    std::vector<int64_t>& y = host[(size_t)h];
    y.resize((size_t)words);
    for (int64_t i = 0; i < words; ++i) {
      const u64 r = canon(funcs_pow[h][i], pe);
      y[(size_t)i] = 2 * r >= pe ? (int64_t)(r + Q - pe) : (int64_t)r;
    }
    DevBuf<int64_t>& d = c->d_ys[(size_t)h];
    if (d.alloc((size_t)words) ||
        hipMemcpyAsync(d, y.data(), sizeof(int64_t) * (size_t)words, hipMemcpyHostToDevice, s) != hipSuccess)
      rc = LOLHIP_ERR_HIP;
    if (!rc) rc = do_crt(S, s, d, rel, false);
  }
  const int rs = s.sync();
  if (rc || rs) return rc ? rc : rs;
  *out = c.release();
  return LOLHIP_OK;
}

int64_t lolhip_pt_tunnel_work_len(const lolhip_pt_tunnel* c, int64_t B) {
  if (!c || B < 0) return LOLHIP_ERR_INVALID;
  return measure(pt_tunnel_work, *c, B);
}

int lolhip_pt_tunnel_batch(const lolhip_pt_tunnel* c, void* stream, const int64_t* x_dec, int64_t* out_pow, int64_t* work,
                           int64_t B) {
  if (!c || B < 0) return LOLHIP_ERR_INVALID;
  if (!c->device) return LOLHIP_ERR_NO_DEVICE;
  int rc = need_device(*c->es[0]->X.hi); if (rc) return rc;
  if (B > 0 && (!x_dec || !out_pow || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  Work w(work);
  auto [a, b, ev] = pt_tunnel_work(w, *c, B);                       // a: the hop's input, decoding basis of R_h mod Q_h
  Relift rl = c->rl;
  rl.Qin = 0;
  rl.Qout = c->es[0]->X.hi->qs[0];
  if (launch_relift(s, x_dec, nullptr, a, B * c->er[0]->X.host.phi2, rl) != hipSuccess) return LOLHIP_ERR_HIP;
  for (int h = 0; h < c->nhops; ++h) {
    const Plan& S = *c->es[(size_t)h]->X.hi;
    rc = lolhip_evallin_batch(c->er[(size_t)h], c->es[(size_t)h], stream, a, c->d_ys[(size_t)h], b, ev, B);
    if (!rc) rc = do_crt(S, s, b, B, true);
    if (rc) return rc;
    rl.Qin = S.qs[0];
    if (h + 1 == c->nhops) return hip_status(launch_relift(s, b, out_pow, nullptr, B * S.n, rl));
    const Plan& R = *c->er[(size_t)(h + 1)]->X.hi;
    rl.Qout = R.qs[0];
    if (launch_relift(s, b, nullptr, b, B * S.n, rl) != hipSuccess) return LOLHIP_ERR_HIP;
    rc = run_prog_or_copy(R, R.prog_linv, s, b, B); if (rc) return rc;
    std::swap(a, b);
  }
  return LOLHIP_OK;
}

}  // extern "C"
