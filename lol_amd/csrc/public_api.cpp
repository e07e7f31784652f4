// lol_amd/csrc/public_api.cpp — the C ABI of the SymmSHE public operations and ciphertext addition (include/lolhip.h;
// lol-apps SymmSHE.hs:214-230, 381-436): host checks, the encoding factors and the launch plan over the kernels of
// public.hip and the existing transforms.
#include <hip/hip_runtime_api.h>

#include "public.h"
#include "she_host.h"

using namespace lolhip;

namespace {

// the checks both public entries share, in the order of their statuses.  *lo: the plan of index m
int public_checks(const lolhip_plan* pq, const lolhip_ext* x_q, int64_t stride, int ncs, int cs_shared,
                  const int64_t* cs, const int64_t* out, const int64_t* work, const int64_t* pub, int64_t B,
                  const Plan** lo) {
  if (!pq) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (ncs < 1 || B < 0 || P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  *lo = lo_plan(P, x_q);
  if (!*lo) return LOLHIP_ERR_INVALID;
  if (stride < 0 || (stride > 0 && stride < (*lo)->n)) return LOLHIP_ERR_INVALID;
  if (B > 0 && (!pub || !cs || !out || !work)) return LOLHIP_ERR_INVALID;
  if (cs_shared && B > 1 && out == cs) return LOLHIP_ERR_INVALID;     // item 0's output would overwrite the shared input
  return LOLHIP_OK;
}

// device checks: the plans and the ext's tables live on the calling thread's device
int public_device(const lolhip_plan* pq, const lolhip_ext* x_q) {
  int rc = need_device(pq); if (rc) return rc;
  if (x_q && (!x_q->X.d_embed_pow || !x_q->X.d_embed_crt || !x_q->X.lo->device)) return LOLHIP_ERR_NO_DEVICE;
  return LOLHIP_OK;
}

// work: the lifted public values [items][n_m][T] | their residues mod p [items][n_m] (addPublic with k > 0)
struct PubWork { int64_t *lifted, *pw; };
PubWork pub_work(Work& w, const Plan& P, const Plan& lo, int64_t items) {
  return {w.take(items * lo.n * P.T), w.take(items * lo.n)};
}

}  // namespace

// k = 0: k_pub_lift (b -> the T moduli at index m, linv folded in);  k > 0: k_pub_lift (b mod p) -> mulgpow k times on pp
// -> k_pub_lift (-> the T moduli, linv folded in);  then crt at index m
int lolhip::public_lift(const Plan& P, const Plan& lo, const Plan* pp, hipStream_t s, const int64_t* b, int64_t stride,
                        int64_t items, int64_t k, u64 linv, u64 p, bool crt, int64_t* pw, int64_t* lifted) {
  const ModCtx mp = make_modctx(p);
  const i64 n_m = lo.n;
  if (k > 0) {
    if (launch_pub_lift(s, b, stride, items, n_m, pw, 1, pp->d_mod, mp, 1) != hipSuccess) return LOLHIP_ERR_HIP;
    for (int64_t i = 0; i < k; ++i) {
      const int rc = run_prog_or_copy(*pp, pp->prog_gpow, s, pw, items); if (rc) return rc;
    }
    if (launch_pub_lift(s, pw, n_m, items, n_m, lifted, P.T, lo.d_mod, mp, linv) != hipSuccess) return LOLHIP_ERR_HIP;
  } else if (launch_pub_lift(s, b, stride, items, n_m, lifted, P.T, lo.d_mod, mp, linv) != hipSuccess) {
    return LOLHIP_ERR_HIP;
  }
  return crt ? do_crt(lo, s, lifted, items, false) : LOLHIP_OK;
}

extern "C" {

int lolhip_encode_scales(const lolhip_plan* pq, int64_t p, int to_msd, int64_t* zq_scale, int64_t* zp_scale) {
  if (!pq || !zq_scale || !zp_scale || (to_msd != 0 && to_msd != 1) || pq->P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  u64 zq[PIPE_MAX_T], zp = 0;
  const int rc = encode_scales(pq->P, p, to_msd != 0, zq, &zp);
  if (rc) return rc;
  for (int t = 0; t < pq->P.T; ++t) zq_scale[t] = (int64_t)zq[t];
  *zp_scale = (int64_t)zp;
  return LOLHIP_OK;
}

int lolhip_ct_lincomb_batch(const lolhip_plan* pq, void* stream, const int64_t* a, int na, const int64_t* alpha,
                            const int64_t* b, int nb, const int64_t* beta, int64_t* out, int64_t B) {
  if (!pq) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (na < 1 || nb < 0 || B < 0 || P.T > PIPE_MAX_T || !alpha || (nb > 0 && (!b || !beta)) || (nb == 0 && b))
    return LOLHIP_ERR_INVALID;
  if (B > 0 && (!a || !out)) return LOLHIP_ERR_INVALID;
  int rc = need_device(pq); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  u64 al[PIPE_MAX_T], be[PIPE_MAX_T];
  for (int t = 0; t < P.T; ++t) {
    al[t] = canon(alpha[t], P.qs[(size_t)t]);
    be[t] = nb > 0 ? canon(beta[t], P.qs[(size_t)t]) : 0;
  }
  PubScales sc;
  set_scale(sc, P, al, be);
  return hip_status(launch_ct_lincomb((hipStream_t)stream, a, na, nb > 0 ? b : nullptr, nb, out, B * P.n * P.T, sc));
}

int64_t lolhip_public_work_len(const lolhip_plan* pq, const lolhip_ext* x_q, int64_t B) {
  if (!pq || B < 0) return LOLHIP_ERR_INVALID;
  const Plan* lo = lo_plan(pq->P, x_q);
  if (!lo) return LOLHIP_ERR_INVALID;
  return measure(pub_work, pq->P, *lo, B);
}

// addPublic (SymmSHE.hs:381-390): toLSD, then c_0 + embed (reduce (decode' (l^-1 g^k b))).  Launch plan: public_lift
// (into the CRT basis for CRT-basis ciphertexts) -> k_pub_apply (the MSD -> LSD factor p mod q_t on every component, the
// embed gather: baseIndicesCRT or embedPow)
int lolhip_add_public_batch(const lolhip_plan* pq, const lolhip_ext* x_q, const lolhip_plan* pp_m, void* stream,
                            const int64_t* b_pow, int64_t b_stride, const int64_t* cs, int ncs, int cs_shared,
                            int cs_crt, int enc, int64_t k, int64_t l, int64_t p, int64_t* out, int64_t* l_out,
                            int64_t* work, int64_t B) {
  const Plan* lo = nullptr;
  int rc = public_checks(pq, x_q, b_stride, ncs, cs_shared, cs, out, work, b_pow, B, &lo); if (rc) return rc;
  const Plan& P = pq->P;
  if ((enc != 0 && enc != 1) || k < 0 || !l_out) return LOLHIP_ERR_INVALID;
  if (k > 0 && (!pp_m || pp_m->P.T != 1 || pp_m->P.m != lo->m || (int64_t)pp_m->P.qs[0] != p)) return LOLHIP_ERR_INVALID;
  if (cs_crt && (!P.has_crt || !lo->has_crt)) return LOLHIP_ERR_NO_CRT;
  if (!p_ok(p)) return LOLHIP_ERR_MODULUS;
  const u64 up = (u64)p;
  u64 zq[PIPE_MAX_T], zp = 1;
  if (enc == 1) { rc = encode_scales(P, p, false, zq, &zp); if (rc) return rc; }      // msdToLSD
  const u64 l2 = encode_l(l, zp, up);                                              // l after toLSD
  const u64 linv = invmod(l2, up);
  if (linv == 0) return LOLHIP_ERR_MODULUS;
  rc = public_device(pq, x_q); if (rc) return rc;
  if (k > 0) { rc = need_device(pp_m); if (rc) return rc; }
  *l_out = (int64_t)l2;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const i64 n_m = lo->n, items = b_stride == 0 ? 1 : B;
  Work w(work);
  const auto [lifted, pw] = pub_work(w, P, *lo, items);
  rc = public_lift(P, *lo, k > 0 ? &pp_m->P : nullptr, s, b_pow, b_stride, items, k, linv, up, cs_crt != 0, pw, lifted);
  if (rc) return rc;
  const int32_t* idx = x_q ? (cs_crt ? x_q->X.d_embed_crt : x_q->X.d_embed_pow).get() : nullptr;
  PubScales sc;
  set_scale(sc, P, enc == 1 ? zq : nullptr, nullptr);
  return hip_status(launch_pub_apply(s, PUB_ADD, lifted, b_stride == 0 ? 0 : n_m * P.T, idx, cs, cs_shared != 0, out,
                                     ncs, B, P.n, sc, P.d_mod));
}

// mulPublic (SymmSHE.hs:405-411): every c_i times embed (reduce (decode' a)), CRT basis.  Launch plan: public_lift (k = 0,
// no factor) -> k_pub_apply (the baseIndicesCRT gather folded into the product)
int lolhip_mul_public_batch(const lolhip_plan* pq, const lolhip_ext* x_q, void* stream, const int64_t* a_pow,
                            int64_t a_stride, int64_t p, const int64_t* cs, int ncs, int cs_shared, int64_t* out,
                            int64_t* work, int64_t B) {
  const Plan* lo = nullptr;
  int rc = public_checks(pq, x_q, a_stride, ncs, cs_shared, cs, out, work, a_pow, B, &lo); if (rc) return rc;
  const Plan& P = pq->P;
  if (!P.has_crt || !lo->has_crt) return LOLHIP_ERR_NO_CRT;
  if (!p_ok(p)) return LOLHIP_ERR_MODULUS;
  rc = public_device(pq, x_q); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const i64 n_m = lo->n, items = a_stride == 0 ? 1 : B;
  rc = public_lift(P, *lo, nullptr, s, a_pow, a_stride, items, 0, 1, (u64)p, true, nullptr, work); if (rc) return rc;
  PubScales sc;
  set_scale(sc, P, nullptr, nullptr);
  return hip_status(launch_pub_apply(s, PUB_MUL, work, a_stride == 0 ? 0 : n_m * P.T,
                                     x_q ? x_q->X.d_embed_crt.get() : nullptr, cs, cs_shared != 0, out, ncs, B, P.n, sc,
                                     P.d_mod));
}

}  // extern "C"
