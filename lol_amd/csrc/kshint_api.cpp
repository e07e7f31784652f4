// lol_amd/csrc/kshint_api.cpp — the C ABI of SymmSHE's key-switch and tunnel hints (include/lolhip.h; lol-apps
// SymmSHE.hs:262-296 lweSample / ksHint, :531-545 tunnelHint): host checks and the launch plan over the samplers of
// encrypt.hip, the existing transforms, evalLin and the combine kernel of kshint.hip.
#include <hip/hip_runtime_api.h>

#include "sampler_internal.h"

using namespace lolhip;

namespace {

// every status of a ksHint call over plan p (B rows of L samples each), decided on the host; d: the decomposition
// parameters of the key switch (launch_kshint_combine reads T, L, base and the digit counts)
int hint_status(const Plan& P, double svar, int64_t base, int64_t B, DecompParams& d) {
  if (!svar_ok(svar) || B < 0) return LOLHIP_ERR_INVALID;
  int rc = make_decomp(P, base, d); if (rc) return rc;
  rc = sampler_ok(P); if (rc) return rc;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  return LOLHIP_OK;
}

// ksHint's work: e^ [B][L][n][T] | the double slab [B][L][n] of the Gaussian map (an index that is not a 2-power)
struct HintWork { int64_t* e; double* dbl; };
HintWork hint_work(Work& w, const Plan& P, int64_t L, int64_t B) {
  return {w.take(B * L * P.n * P.T), two_power(P) ? nullptr : w.take_f64(B * L * P.n)};
}

// rounded Gaussians (domain 3) -> residues -> l -> one crt of B*L polynomials -> k_kshint_combine (domain 4)
int kshint_launch(const Plan& P, hipStream_t s, const int64_t* s_crt, const int64_t* vals_crt, double svar,
                  const DecompParams& d, const uint8_t key[32], uint64_t ctr, int64_t* hints, HintWork hw, int64_t B) {
  const int64_t BL = B * d.L;
  const ChaChaKey k = make_key(key);
  const auto [e, dbl] = hw;
  int rc = sample_error(P, s, dbl, nullptr, 1, e, ENC_WRITE, k, ctr, CHACHA_DOM_HINT_GAUSS, deviation(P, svar), BL);
  if (rc) return rc;
  rc = run_prog_or_copy(P, P.prog_l, s, e, BL); if (rc) return rc;
  rc = do_crt(P, s, e, BL, false); if (rc) return rc;
  return hip_status(launch_kshint_combine(s, e, vals_crt, s_crt, hints, B, P.n, d, P.d_mod, k, ctr));
}

// tunnelHint's work: comps [rel][n_S][T] | then either (p_i s_in [rel][n_R][T] | evalLin's regions at B = rel) or, once
// evalLin is done, ksHint's regions of rel rows over the S' plan
struct TunnelHintWork { int64_t *comps, *sp; EvalLinWork ev; HintWork ks; };
TunnelHintWork tunnel_hint_work(Work& w, const ExtPlan& ER, const ExtPlan& ES, int64_t L) {
  const int64_t rel = ER.host.phi2 / ER.host.phi, T = ER.lo->T;
  TunnelHintWork r;
  r.comps = w.take(rel * ES.host.phi2 * T);
  const int64_t m = w.mark();
  r.sp = w.take(rel * ER.host.phi2 * T);
  r.ev = evallin_work(w, ER, ES, rel);
  w.rewind(m);
  r.ks = hint_work(w, *ES.hi, L, rel);
  return r;
}

}  // namespace

extern "C" {

int64_t lolhip_kshint_work_len(const lolhip_plan* pq, int64_t base, int64_t B) {
  if (!pq || B < 0) return LOLHIP_ERR_INVALID;
  DecompParams d;
  const int rc = make_decomp(pq->P, base, d); if (rc) return rc;
  return measure(hint_work, pq->P, d.L, B);
}

int lolhip_kshint_batch(const lolhip_plan* pq, void* stream, const int64_t* s_crt, const int64_t* vals_crt, double svar,
                        int64_t base, const uint8_t key[32], uint64_t ctr, int64_t* hints_out, int64_t* work, int64_t B) {
  int rc = index_status(pq); if (rc) return rc;
  rc = need_device(pq); if (rc) return rc;
  DecompParams d;
  rc = hint_status(pq->P, svar, base, B, d); if (rc) return rc;
  if (B > 0 && (!s_crt || !vals_crt || !key || !hints_out || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  Work w(work);
  return kshint_launch(pq->P, (hipStream_t)stream, s_crt, vals_crt, svar, d, key, ctr, hints_out, hint_work(w, pq->P, d.L, B), B);
}

int64_t lolhip_tunnel_hint_work_len(const lolhip_ext* x_er, const lolhip_ext* x_es, int64_t base) {
  if (!x_er || !x_es) return LOLHIP_ERR_INVALID;
  DecompParams d;
  const int rc = make_decomp(*x_es->X.hi, base, d); if (rc) return rc;
  return measure(tunnel_hint_work, x_er->X, x_es->X, d.L);
}

// tunnelHint f skout skin (SymmSHE.hs:531-545): comps_i = evalLin f' (s_in p_i) over the relative powerful basis p_i of
// R'/E', then hints_i = ksHint skout comps_i:
//   unit vectors p_i -> crt (R') -> * s_in^ -> crtInv -> lInv -> evalLin (B = rel) -> ksHint (B = rel, S' plan)
int lolhip_tunnel_hint_batch(const lolhip_ext* x_er, const lolhip_ext* x_es, void* stream, const int64_t* ys_crt,
                             const int64_t* s_in_crt, const int64_t* s_out_crt, double svar, int64_t base,
                             const uint8_t key[32], uint64_t ctr, int64_t* hints_out, int64_t* work) {
  if (!x_er || !x_es) return LOLHIP_ERR_INVALID;
  const ExtPlan &ER = x_er->X, &ES = x_es->X;
  if (!ER.d_coeffs || !ES.d_embed_dec) return LOLHIP_ERR_NO_DEVICE;
  if (ER.host.phi != ES.host.phi || ER.lo->T != ES.lo->T || ER.lo->qs != ES.lo->qs || ER.lo->pps.size() != ES.lo->pps.size())
    return LOLHIP_ERR_INVALID;                                     // the two extensions must share E' and the moduli
  const Plan &PR = *ER.hi, &PS = *ES.hi;
  DecompParams d;
  int rc = hint_status(PS, svar, base, 0, d); if (rc) return rc;
  if (!PR.has_crt) return LOLHIP_ERR_NO_CRT;
  if (!ys_crt || !s_in_crt || !s_out_crt || !key || !hints_out || !work) return LOLHIP_ERR_INVALID;

  hipStream_t s = (hipStream_t)stream;
  const int64_t rel = ER.host.phi2 / ER.host.phi, T = PS.T, nR = PR.n;
  Work w(work);
  const auto [comps, sp, ev, ks] = tunnel_hint_work(w, ER, ES, d.L);
  if (launch_unit_rows(s, sp, ER.d_coeffs, rel, nR, (int)T, ER.host.phi) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(PR, s, sp, rel, false); if (rc) return rc;
  if (launch_sk_eval(s, sp, 1, true, s_in_crt, sp, rel, nR, (int)T, PR.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(PR, s, sp, rel, true); if (rc) return rc;
  rc = run_prog_or_copy(PR, PR.prog_linv, s, sp, rel); if (rc) return rc;
  rc = lolhip_evallin_batch(x_er, x_es, stream, sp, ys_crt, comps, ev.tmp_e, rel); if (rc) return rc;
  return kshint_launch(PS, s, s_out_crt, comps, svar, d, key, ctr, hints_out, ks, rel);
}

}  // extern "C"
