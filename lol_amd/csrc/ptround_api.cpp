// lol_amd/csrc/ptround_api.cpp — the C ABI of HomomPRF's homomorphic rounding 2^e -> 2 (include/lolhip.h; lol-apps
// HomomPRF.hs:215-270 over SymmSHE.hs:236-258, 361-390, 444-452): host checks, the metadata (enc, k, l) of every step,
// and the launch plan over k_ct_affine_mul (ptround.hip), lolhip_modswitch_batch, lolhip_keyswitch_batch, the passes of
// public.hip for the public constants and the existing transforms.
#include <hip/hip_runtime_api.h>

#include <memory>
#include <vector>

#include "ptround.h"
#include "she_host.h"

using namespace lolhip;

namespace {

// b's moduli are a's without the first one
bool drops_first(const Plan& a, const Plan& b) {
  if (b.T + 1 != a.T) return false;
  for (int t = 0; t < b.T; ++t)
    if (a.qs[(size_t)t + 1] != b.qs[(size_t)t]) return false;
  return true;
}

constexpr int PTROUND_MAX_E = 16;                            // p <= 2^16: at most 2^13 pairs in one launch

}  // namespace

struct lolhip_ptround {
  int e = 0;
  int64_t p = 0, base = 0;
  std::vector<const lolhip_plan*> lvl, up;
  std::vector<const int64_t*> hints;
  std::vector<int> L;                                          // digits of the gadget over U_i
  const lolhip_plan* pp_m = nullptr;
  const lolhip_ext* xq[2] = {nullptr, nullptr};
  const Plan* lo[2] = {nullptr, nullptr};                      // index m over Z_0 / Z_1
  i64 n_m = 0;
  DevBuf<int64_t> d_src;                                       // [1 + p/4][n_m]: 1, then y (1 - y) for odd y, then for even y
};

namespace {

// work, every region rounded: a level's products | the ciphertexts it leaves the next level, ping-pong | one product over
// U_i | its key switch's output | that key switch's digits | what either modSwitch of a level carves | the public constants
// over Z_i | lifted at index m | mod p (public_lift) | the zero polynomial they are added to
struct RoundWork { int64_t *prod, *cts[2], *up, *ks, *dig, *sub, *cemb, *clift, *cpw, *zero; };
RoundWork round_work(Work& w, const lolhip_ptround& c, int64_t B) {
  RoundWork r = RoundWork();
  if (c.e < 2 || B == 0) return r;
  const Plan& P0 = c.lvl[0]->P;
  const i64 N = B * P0.n, T0 = P0.T, Tu = T0 + 1, np1 = c.e >= 3 ? c.p / 8 : 0, nc = c.p / 4 + 1;
  r.prod = w.take(even(std::max(3 * N * T0, 3 * np1 * N * (T0 - 1))));
  for (int64_t*& ct : r.cts) ct = w.take(even(std::max(2 * N * T0, 2 * np1 * N * (T0 - 2))));
  r.up = w.take(even(3 * N * Tu));
  r.ks = w.take(even(2 * N * Tu));
  i64 Lmax = 0;
  for (int L : c.L) Lmax = std::max<i64>(Lmax, L);
  r.dig = w.take(even(measure(ks_digits, Lmax, B, P0.n, Tu)));
  r.sub = w.take(even(measure([&](Work& m) {
    for (size_t i = 0; i < c.up.size(); ++i) {
      modswitch_work(m, c.lvl[i]->P, 3, B);
      m.rewind(0);
      modswitch_work(m, c.up[i]->P, 2, B);
      m.rewind(0);
    }
  })));
  r.cemb = w.take(even(nc * P0.n * T0));
  r.clift = w.take(even(nc * c.n_m * T0));
  r.cpw = w.take(even(nc * c.n_m));
  r.zero = w.take(even(P0.n * T0));
  return r;
}

// emb [items][n'][T] = embed (reduce (decode' (linv g_m^k v))) in the CRT basis of P, v = src [items][n_m] in R_m mod p:
// the passes of lolhip_add_public_batch onto a zero polynomial
int public_consts(const Plan& P, const Plan& lo, const lolhip_ext* x_q, const Plan& PP, hipStream_t s, const int64_t* src,
                  i64 items, int64_t k, u64 linv, u64 p, int64_t* pw, int64_t* lifted, const int64_t* zero, int64_t* emb) {
  const int rc = public_lift(P, lo, &PP, s, src, lo.n, items, k, linv, p, true, pw, lifted); if (rc) return rc;
  PubScales one;
  set_scale(one, P, nullptr, nullptr);
  return hip_status(launch_pub_apply(s, PUB_ADD, lifted, lo.n * P.T, x_q ? x_q->X.d_embed_crt.get() : nullptr, zero, true, emb, 1,
                                     items, P.n, one, P.d_mod));
}

// the statuses of the pieces' dry runs (B = 0): *st keeps the first that is not LOLHIP_ERR_NO_DEVICE, else that one, so a
// host-only ladder reports what a device one would
void note(int rc, int* st) {
  if (rc == LOLHIP_OK) return;
  if (*st == LOLHIP_OK || (*st == LOLHIP_ERR_NO_DEVICE && rc != LOLHIP_ERR_NO_DEVICE)) *st = rc;
}

}  // namespace

extern "C" {

int lolhip_ct_affine_mul_batch(const lolhip_plan* pq, void* stream, const int64_t* a, const int64_t* alpha,
                               const int64_t* va, const int64_t* b, const int64_t* beta, const int64_t* vb, int npairs,
                               int64_t* out, int64_t B) {
  if (!pq) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (npairs < 1 || npairs > 65535 || B < 0 || P.T > PIPE_MAX_T || !alpha || !beta) return LOLHIP_ERR_INVALID;
  if (B > 0 && (!a || !b || !out)) return LOLHIP_ERR_INVALID;
  if (B > 0 && npairs > 1 && (out == a || out == b)) return LOLHIP_ERR_INVALID;   // pair 0's output would overwrite the shared input
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  int rc = need_device(pq); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  u64 al[PIPE_MAX_T], be[PIPE_MAX_T];
  for (int t = 0; t < P.T; ++t) {
    al[t] = canon(alpha[t], P.qs[(size_t)t]);
    be[t] = canon(beta[t], P.qs[(size_t)t]);
  }
  PubScales sc;
  set_scale(sc, P, al, be);
  return hip_status(launch_ct_affine_mul((hipStream_t)stream, a, 0, va, b, 0, vb, npairs, out, B, P.n, sc, P.d_gcrt,
                                         P.d_mod));
}

int lolhip_ptround_create(int e, int64_t p, const lolhip_plan* const* p_lvl, const lolhip_plan* const* p_up,
                          const int64_t* const* hints, int64_t base, const lolhip_plan* pp_m, const lolhip_ext* x_q0,
                          const lolhip_ext* x_q1, lolhip_ptround** out) {
  if (!out) return LOLHIP_ERR_INVALID;
  *out = nullptr;
  if (e < 1 || e > PTROUND_MAX_E || !p_lvl || (e > 1 && (!p_up || !hints || !pp_m))) return LOLHIP_ERR_INVALID;
  std::unique_ptr<lolhip_ptround> c(new lolhip_ptround());
  c->e = e; c->p = p; c->base = base; c->pp_m = pp_m;
  for (int i = 0; i < e; ++i) {
    if (!p_lvl[i]) return LOLHIP_ERR_INVALID;
    const Plan& Z = p_lvl[i]->P;
    if (Z.T < 1 || Z.T > PIPE_MAX_T || !same_index(Z, p_lvl[0]->P)) return LOLHIP_ERR_INVALID;
    if (i > 0 && !drops_first(p_lvl[i - 1]->P, Z)) return LOLHIP_ERR_INVALID;
    c->lvl.push_back(p_lvl[i]);
  }
  for (int i = 0; i + 1 < e; ++i) {
    if (!p_up[i] || !hints[i]) return LOLHIP_ERR_INVALID;
    const Plan& U = p_up[i]->P;
    if (U.T > PIPE_MAX_T || !same_index(U, p_lvl[0]->P) || !drops_first(U, p_lvl[i]->P)) return LOLHIP_ERR_INVALID;
    DecompParams dp;
    const int rc = make_decomp(U, base, dp); if (rc) return rc;
    c->up.push_back(p_up[i]); c->hints.push_back(hints[i]); c->L.push_back(dp.L);
  }
  const Plan& P0 = p_lvl[0]->P;
  c->lo[0] = lo_plan(P0, x_q0);
  if (!c->lo[0]) return LOLHIP_ERR_INVALID;
  c->xq[0] = x_q0;
  c->n_m = c->lo[0]->n;
  if (e > 1) {
    c->lo[1] = lo_plan(p_lvl[1]->P, x_q1);
    if (!c->lo[1] || !!x_q0 != !!x_q1 || !same_index(*c->lo[0], *c->lo[1])) return LOLHIP_ERR_INVALID;
    c->xq[1] = x_q1;
    const Plan& PP = pp_m->P;
    if (PP.T != 1 || (int64_t)PP.qs[0] != p || !same_index(PP, *c->lo[0])) return LOLHIP_ERR_INVALID;
  }
  if (p != ((int64_t)1 << e)) return LOLHIP_ERR_MODULUS;
  for (int i = 0; i < e; ++i) {
    const Plan& A = i + 1 < e ? p_up[i]->P : p_lvl[i]->P;     // U_i holds Z_i's moduli
    for (u64 q : A.qs) if ((q & 1) == 0) return LOLHIP_ERR_MODULUS;
  }
  for (int i = 0; i < e; ++i) {
    if (!p_lvl[i]->P.has_crt || (i + 1 < e && !p_up[i]->P.has_crt)) return LOLHIP_ERR_NO_CRT;
    if (i < 2 && e > 1 && !c->lo[i]->has_crt) return LOLHIP_ERR_NO_CRT;
  }
  if (e > 1 && P0.device) {
    // the constants as elements of R_m: the scalar in the first powerful-basis coefficient
    const i64 half = p / 8, nc = p / 4 + 1;
    std::vector<int64_t> src((size_t)(nc * c->n_m), 0);
    src[0] = 1;
    for (i64 y = 1; y <= p / 4; ++y) {
      const i64 slot = (y & 1) ? 1 + (y - 1) / 2 : 1 + half + (y - 2) / 2;       // odd y first (the a side of the pairs)
      src[(size_t)(slot * c->n_m)] = y * (1 - y);
    }
    if (c->d_src.upload(src)) return LOLHIP_ERR_HIP;
  }
  *out = c.release();
  return LOLHIP_OK;
}

void lolhip_ptround_destroy(lolhip_ptround* c) { delete c; }

int64_t lolhip_ptround_work_len(const lolhip_ptround* c, int64_t B) {
  if (!c || B < 0) return LOLHIP_ERR_INVALID;
  return measure(round_work, *c, B);
}

int lolhip_ptround_batch(const lolhip_ptround* c, void* stream, const int64_t* cs, int cs_crt, int enc, int64_t k,
                         int64_t l, int64_t* out, int out_crt, int64_t* k_out, int64_t* l_out, int64_t* work, int64_t B) {
  if (!c || !k_out || !l_out || B < 0 || (enc != 0 && enc != 1) || k < 0) return LOLHIP_ERR_INVALID;
  const int e = c->e;
  if (B > 0 && (!cs || !out || (e > 1 && !work))) return LOLHIP_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const lolhip_plan* h0 = c->lvl[0];
  const Plan& P0 = h0->P;
  int rc;
  if (e == 1) {                                                 // ptRound RHNil x = x
    rc = need_device(h0); if (rc) return rc;
    if (B > 0) {
      const size_t bytes = sizeof(int64_t) * (size_t)(2 * B * P0.n * P0.T);
      if (out != cs && hipMemcpyAsync(out, cs, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return LOLHIP_ERR_HIP;
      if (!cs_crt != !out_crt) { rc = do_crt(P0, s, out, 2 * B, cs_crt != 0); if (rc) return rc; }
    }
    *k_out = k; *l_out = l;
    return LOLHIP_OK;
  }
  if (k > (((int64_t)1 << 40) >> e)) return LOLHIP_ERR_INVALID;  // k_out and the mulGPow count stay small

  // ---- every status and the metadata of every step, on the host ----------------------------------------------------
  const int nlev = e - 1;                                       // levels 0 .. e-2, one hint each
  const u64 p0 = (u64)c->p;
  u64 zq[PIPE_MAX_T], zp = 1;
  // level 0: x' = addPublic 1 x (toLSD), prod = x * x'
  u64 beta0[PIPE_MAX_T], ones[PIPE_MAX_T];                     // the factor 1 (a plan's moduli are at least 2)
  for (int t = 0; t < PIPE_MAX_T; ++t) beta0[t] = ones[t] = 1;
  if (enc == 1) { rc = encode_scales(P0, (int64_t)p0, false, beta0, &zp); if (rc) return rc; }
  const u64 lL0 = encode_l(l, zp, p0);                          // l of x' (LSD)
  const u64 linv0 = invmod(lL0, p0);
  if (linv0 == 0) return LOLHIP_ERR_MODULUS;
  int64_t l_in[PTROUND_MAX_E], l_up[PTROUND_MAX_E], l_dn[PTROUND_MAX_E], kk[PTROUND_MAX_E + 1];   // on the stack: no allocation
  u64 alpha[PTROUND_MAX_E * PIPE_MAX_T] = {0};
  kk[0] = k;
  l_in[0] = (int64_t)mulmod(lL0, canon(l, p0), p0);             // (*): l1 l2, the product keeps the encoding of x
  u64 linv1 = 0, scale_a[PIPE_MAX_T], scale_b[PIPE_MAX_T];
  int st = LOLHIP_OK;
  for (int i = 0; i < nlev; ++i) {
    const int64_t pi = c->p >> i;
    const Plan& Z = c->lvl[(size_t)i]->P;
    if (i >= 1) {
      // (*) of two MSD ciphertexts: toLSD on the first operand
      rc = encode_scales(Z, pi, false, &alpha[(size_t)i * PIPE_MAX_T], &zp); if (rc) return rc;
      const u64 la = encode_l(l_dn[(size_t)i - 1], zp, (u64)pi);
      l_in[(size_t)i] = (int64_t)mulmod(la, (u64)l_dn[(size_t)i - 1], (u64)pi);
    }
    kk[(size_t)i + 1] = 2 * kk[(size_t)i] + 1;
    // modSwitch up is toMSD as well (level 0 of an LSD input); down and the key switch leave l alone
    zp = 1;
    if (i == 0 && enc == 0) { rc = encode_scales(Z, pi, true, zq, &zp); if (rc) return rc; }
    l_up[(size_t)i] = l_dn[(size_t)i] = (int64_t)encode_l(l_in[(size_t)i], zp, (u64)pi);
    int64_t dry = 0;                                            // the pieces' own statuses, by dry runs (B = 0)
    note(lolhip_modswitch_batch(c->lvl[(size_t)i], c->up[(size_t)i], nullptr, nullptr, 3, 1, i == 0 ? enc : 1, l_in[(size_t)i], pi,
                                nullptr, 0, &dry, nullptr, 0), &st);
    note(lolhip_modswitch_batch(c->up[(size_t)i], c->lvl[(size_t)i + 1], nullptr, nullptr, 2, 1, 1, l_up[(size_t)i], pi, nullptr,
                                i + 1 == nlev ? out_crt : 1, &dry, nullptr, 0), &st);
    if (st != LOLHIP_OK && st != LOLHIP_ERR_NO_DEVICE) return st;
    if (i == 0) {
      // xs_y = modSwitchPT (addPublic (y (1 - y)) xprod): toLSD, the constant over l^-1, toMSD, l into p / 2
      const Plan& Z1 = c->lvl[1]->P;
      u64 zpl = 1, zpm = 1;
      rc = encode_scales(Z1, (int64_t)p0, false, zq, &zpl); if (rc) return rc;
      const u64 lL1 = encode_l(l_dn[0], zpl, p0);
      linv1 = invmod(lL1, p0);
      if (linv1 == 0) return LOLHIP_ERR_MODULUS;
      rc = encode_scales(Z1, (int64_t)p0, true, scale_b, &zpm); if (rc) return rc;     // p^-1 mod q_t on the constants
      const u64 lm = encode_l((int64_t)lL1, zpm, p0);
      l_dn[0] = (int64_t)(lm % (p0 / 2));                       // reduce (lift l): p / 2 divides p
    } else {
      l_dn[(size_t)i] = (int64_t)((u64)l_dn[(size_t)i] % ((u64)pi / 2));             // modSwitchPT
    }
  }
  if (nlev >= 2) {                                              // the a side of level 1 carries toLSD's p_1 as well
    const Plan& Z1 = c->lvl[1]->P;
    for (int t = 0; t < Z1.T; ++t) scale_a[t] = mulmod(scale_b[t], alpha[(size_t)PIPE_MAX_T + t], Z1.qs[(size_t)t]);
  }
  for (int i = 0; i < nlev; ++i) note(lolhip_keyswitch_batch(c->up[(size_t)i], nullptr, nullptr, c->base, nullptr, 2, nullptr, nullptr, nullptr, 0), &st);
  note(need_device(h0), &st);
  note(need_device(c->pp_m), &st);
  for (int i = 0; i < 2; ++i) {
    if (c->xq[i] && (!c->xq[i]->X.d_embed_crt || !c->lo[i]->device)) note(LOLHIP_ERR_NO_DEVICE, &st);
  }
  if (st == LOLHIP_OK && !c->d_src) st = LOLHIP_ERR_NO_DEVICE;
  if (st != LOLHIP_OK) return st;
  const int64_t k_fin = kk[(size_t)nlev], l_fin = l_dn[(size_t)nlev - 1];
  if (B == 0) { *k_out = k_fin; *l_out = l_fin; return LOLHIP_OK; }

  // ---- launches ---------------------------------------------------------------------------------------------------------
  Work w(work);
  const auto [prod, cts, up, ks, dig, sub, cemb, clift, cpw, zero] = round_work(w, *c, B);
  const i64 N = B * P0.n;
  const Plan& PP = c->pp_m->P;
  if (hipMemsetAsync(zero, 0, sizeof(int64_t) * (size_t)(P0.n * P0.T), s) != hipSuccess) return LOLHIP_ERR_HIP;

  // level 0: x (beta x + v), v the constant 1
  const int64_t* x = cs;
  if (!cs_crt) {
    if (hipMemcpyAsync(cts[1], cs, sizeof(int64_t) * (size_t)(2 * N * P0.T), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return LOLHIP_ERR_HIP;
    rc = do_crt(P0, s, cts[1], 2 * B, false); if (rc) return rc;
    x = cts[1];
  }
  rc = public_consts(P0, *c->lo[0], c->xq[0], PP, s, c->d_src, 1, k, linv0, p0, cpw, clift, zero, cemb); if (rc) return rc;
  PubScales sc;
  set_scale(sc, P0, nullptr, beta0);
  if (launch_ct_affine_mul(s, x, 0, nullptr, x, 0, cemb, 1, prod, B, P0.n, sc, P0.d_gcrt, P0.d_mod) != hipSuccess)
    return LOLHIP_ERR_HIP;

  i64 npairs = 1;
  int cur = 0;                                                  // cts[cur]: this level's outputs
  for (int i = 0; i < nlev; ++i) {
    const int64_t pi = c->p >> i;
    const lolhip_plan *hz = c->lvl[(size_t)i], *hu = c->up[(size_t)i], *hn = c->lvl[(size_t)i + 1];
    const Plan &Z = hz->P, &U = hu->P, &Zn = hn->P;
    if (i == 1) {
      // the fan-out and the first pairing from xprod alone: (p_1 (xprod + v_{2j+1})) (xprod + v_{2j+2}), the constants
      // through toMSD's p^-1 (and toLSD's p_1 on the a side)
      npairs = c->p / 8;
      const i64 per = Z.n * Z.T;
      rc = public_consts(Z, *c->lo[1], c->xq[1], PP, s, c->d_src + c->n_m, 2 * npairs, kk[1], linv1, p0, cpw, clift, zero, cemb);
      if (rc) return rc;
      PubScales sa, sb;
      set_scale(sa, Z, scale_a, nullptr);
      set_scale(sb, Z, scale_b, nullptr);
      if (launch_ct_lincomb(s, cemb, 1, nullptr, 0, cemb, npairs * per, sa) != hipSuccess) return LOLHIP_ERR_HIP;
      if (launch_ct_lincomb(s, cemb + npairs * per, 1, nullptr, 0, cemb + npairs * per, npairs * per, sb) != hipSuccess)
        return LOLHIP_ERR_HIP;
      set_scale(sc, Z, &alpha[(size_t)PIPE_MAX_T], ones);
      if (launch_ct_affine_mul(s, cts[cur], 0, cemb, cts[cur], 0, cemb + npairs * per, (int)npairs, prod, B, Z.n, sc, Z.d_gcrt,
                               Z.d_mod) != hipSuccess)
        return LOLHIP_ERR_HIP;
      cur ^= 1;
    } else if (i >= 2) {
      npairs /= 2;
      const i64 ctw = 2 * N * Z.T;
      set_scale(sc, Z, &alpha[(size_t)i * PIPE_MAX_T], ones);
      if (launch_ct_affine_mul(s, cts[cur], 2 * ctw, nullptr, cts[cur] + ctw, 2 * ctw, nullptr, (int)npairs, prod, B, Z.n, sc,
                               Z.d_gcrt, Z.d_mod) != hipSuccess)
        return LOLHIP_ERR_HIP;
      cur ^= 1;
    }
    const bool last = i + 1 == nlev;
    for (i64 j = 0; j < npairs; ++j) {
      int64_t lo_ = 0;
      rc = lolhip_modswitch_batch(hz, hu, stream, prod + j * 3 * N * Z.T, 3, 1, i == 0 ? enc : 1, l_in[(size_t)i], pi, up, 0, &lo_,
                                  sub, B);
      if (rc) return rc;
      rc = do_crt(U, s, up, 2 * B, false); if (rc) return rc;
      rc = lolhip_keyswitch_batch(hu, stream, up + 2 * N * U.T, c->base, c->hints[(size_t)i], 2, up, ks, dig, B); if (rc) return rc;
      int64_t* dst = last ? out : cts[cur] + j * 2 * N * Zn.T;
      rc = lolhip_modswitch_batch(hu, hn, stream, ks, 2, 1, 1, l_up[(size_t)i], pi, dst, last ? out_crt : 1, &lo_, sub, B);
      if (rc) return rc;
    }
  }
  *k_out = k_fin; *l_out = l_fin;                                // last: not written where a launch fails
  return LOLHIP_OK;
}

}  // extern "C"
