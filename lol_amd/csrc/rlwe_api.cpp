// lol_amd/csrc/rlwe_api.cpp — the C ABI of gSqNormDec and of RLWE / RLWR sampling and instance verification
// (include/lolhip.h; lol RLWE/{Continuous,Discrete,RLWR}.hs, rlwe-challenges Generate.hs / Verify.hs): host checks and
// the launch plans over the kernels of rlwe.hip, the samplers of encrypt.hip, the lift of decrypt.hip and the existing
// transforms.
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "rlwe.h"
#include "sampler_internal.h"

using namespace lolhip;

namespace {

enum { KIND_DISC = 0, KIND_CONT = 1, KIND_RLWR = 2 };

int odd_primes(const Plan& P) {
  int k = 0;
  for (const PP& pe : P.pps) k += pe.p != 2;
  return k;
}

bool norm_ok(const Plan& P) { return P.n <= NORM_MAX_N && odd_primes(P) <= NORM_MAX_PRIMES; }

// the rounding modulus of RLWR against the plan's single q
bool rlwr_p_ok(const Plan& P, int64_t p) { return p >= 2 && (u64)p < P.qs[0]; }

// a s (b null) or b - a s as decoding-basis residues in place in v
int as_dec(const Plan& P, hipStream_t s, const int64_t* a, const int64_t* b, const int64_t* s_crt, int64_t* v, int64_t B) {
  if (launch_rlwe_as(s, a, b, s_crt, v, B, P.n, P.T, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  const int rc = do_crt(P, s, v, B, true);
  return rc ? rc : run_prog_or_copy(P, P.prog_linv, s, v, B, nullptr);
}

// the host checks of the two RLWR entries
int rlwr_setup(const lolhip_plan* pq, int64_t p, int64_t B) {
  if (!pq) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (B < 0 || P.T != 1 || !rlwr_p_ok(P, p)) return LOLHIP_ERR_INVALID;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  return need_device(pq);
}

// stabilize (Continuous.hs:81-83, Discrete.hs:73-75): x' = (1/2 + log(2 pi x)/2 - c)/pi from 1/(2 pi) until x' - x < 1e-4
// work: v, then e.  Disc: v the residues of b - a s [B][n][T] (error; sample keeps the double slab of the Gaussian map
// [B][n] there) and e the lifted error [B][n];  Cont: v = a s [B][n] and e the Gaussians / the error [B][n];  RLWR: v = a s
struct RlweWork { int64_t *v, *e; };
RlweWork rlwe_work(Work& w, const Plan& P, int kind, int64_t B) {
  return {w.take(B * P.n * (kind == KIND_DISC ? P.T : 1)), kind == KIND_RLWR ? nullptr : w.take(B * P.n)};
}

bool stabilize(double c, double* out) {
  const double pi = 3.141592653589793;
  double x = 1 / (2 * pi);
  for (int it = 0; it < 100000; ++it) {
    const double x1 = (1.0 / 2 + std::log(2 * pi * x) / 2 - c) / pi;
    if (x1 - x < 0.0001) { *out = x1; return std::isfinite(x1); }
    x = x1;
  }
  return false;
}

}  // namespace

extern "C" {

// ---- gSqNormDec ---------------------------------------------------------------------------------------------------
static int gsqnorm_setup(const lolhip_plan* p, const void* e, const void* out, int64_t B) {
  if (!p || B < 0 || !norm_ok(p->P)) return LOLHIP_ERR_INVALID;
  const int rc = need_device(p); if (rc) return rc;
  return B > 0 && (!e || !out) ? LOLHIP_ERR_INVALID : LOLHIP_OK;
}

int lolhip_gsqnorm_batch(const lolhip_plan* p, void* stream, const int64_t* e_dec, int64_t* out, int64_t B) {
  const int rc = gsqnorm_setup(p, e_dec, out, B); if (rc) return rc;
  return hip_status(launch_gsqnorm_i64((hipStream_t)stream, e_dec, out, B, p->P.n, norm_dims(p->P)));
}

int lolhip_gsqnorm_f64_batch(const lolhip_plan* p, void* stream, const double* e_dec, double* out, int64_t B) {
  const int rc = gsqnorm_setup(p, e_dec, out, B); if (rc) return rc;
  return hip_status(launch_gsqnorm_f64((hipStream_t)stream, e_dec, out, B, p->P.n, norm_dims(p->P)));
}

// ---- samplers (Generate.hs:192-218) -------------------------------------------------------------------------------
int64_t lolhip_rlwe_work_len(const lolhip_plan* pq, int kind, int64_t B) {
  if (!pq || B < 0 || kind < KIND_DISC || kind > KIND_RLWR) return LOLHIP_ERR_INVALID;
  return measure(rlwe_work, pq->P, kind, B);
}

int lolhip_rlwe_secret(const lolhip_plan* pq, void* stream, const uint8_t key[32], uint64_t ctr, int64_t* s_crt) {
  if (!pq || pq->P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  const int rc = need_device(pq); if (rc) return rc;
  if (!key || !s_crt) return LOLHIP_ERR_INVALID;
  return hip_status(launch_rlwe_uniform((hipStream_t)stream, RLWE_U_ONLY, s_crt, nullptr, nullptr, 1, P.n, P.T, P.d_mod,
                                        make_key(key), ctr, CHACHA_DOM_RLWE_SECRET));
}

// Launch plans:
//   Disc   rounded Gaussians of domain 6 as residues in b (the sampler of errorRounded) -> l -> crt -> b += a s with a
//          drawn in the same pass
//   Cont   a and a s in one pass -> crtInv -> lInv (x) | Gaussians of domain 6 (-> the decoding-basis map) | b = x + g
//   RLWR   a and a s in one pass -> crtInv -> lInv -> the rounding pass
int lolhip_rlwe_sample_batch(const lolhip_plan* pq, void* stream, int kind, int64_t p, const int64_t* s_crt, double svar,
                             const uint8_t key[32], uint64_t ctr, int64_t* a_crt, void* b_out, int64_t* work, int64_t B) {
  if (!pq || kind < KIND_DISC || kind > KIND_RLWR) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (B < 0 || P.T > PIPE_MAX_T || (kind != KIND_DISC && P.T != 1)) return LOLHIP_ERR_INVALID;
  if (kind == KIND_RLWR) {
    if (!rlwr_p_ok(P, p)) return LOLHIP_ERR_INVALID;
  } else {
    if (!svar_ok(svar)) return LOLHIP_ERR_INVALID;
    const int rc = sampler_ok(P); if (rc) return rc;
  }
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  int rc = need_device(pq); if (rc) return rc;
  if (B > 0 && (!s_crt || !key || !a_crt || !b_out || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const ChaChaKey k = make_key(key);
  const int64_t n = P.n;
  Work w(work);
  const auto [x, e] = rlwe_work(w, P, kind, B);
  if (kind == KIND_DISC) {
    int64_t* b = static_cast<int64_t*>(b_out);
    rc = sample_error(P, s, reinterpret_cast<double*>(x), nullptr, 1, b, ENC_WRITE, k, ctr, CHACHA_DOM_RLWE_GAUSS,
                      deviation(P, svar), B);
    if (rc) return rc;
    rc = run_prog_or_copy(P, P.prog_l, s, b, B); if (rc) return rc;
    rc = do_crt(P, s, b, B, false); if (rc) return rc;
    return hip_status(launch_rlwe_uniform(s, RLWE_U_ADD, a_crt, s_crt, b, B, n, P.T, P.d_mod, k, ctr,
                                          CHACHA_DOM_RLWE_UNIFORM));
  }
  if (launch_rlwe_uniform(s, RLWE_U_PROD, a_crt, s_crt, x, B, n, 1, P.d_mod, k, ctr, CHACHA_DOM_RLWE_UNIFORM) != hipSuccess)
    return LOLHIP_ERR_HIP;
  rc = do_crt(P, s, x, B, true); if (rc) return rc;
  rc = run_prog_or_copy(P, P.prog_linv, s, x, B, nullptr); if (rc) return rc;
  if (kind == KIND_RLWR)
    return hip_status(launch_rlwr_round(s, x, static_cast<int64_t*>(b_out), B * n, P.qs[0], (u64)p));
  double* g = reinterpret_cast<double*>(e);
  if (launch_enc_gauss(s, g, B, n, k, ctr, CHACHA_DOM_RLWE_GAUSS, deviation(P, svar)) != hipSuccess) return LOLHIP_ERR_HIP;
  if (!two_power(P) &&
      launch_gauss(s, g, B, n, P.prog_gauss.d_stages, P.gauss_word, P.d_rconsts) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return hip_status(launch_rlwe_cont_sample(s, x, g, static_cast<double*>(b_out), B * n, (double)P.qs[0]));
}

// ---- error terms and norms (Verify.hs:346-366) ----------------------------------------------------------------------
// Launch plans (the lifted values go to e_out, or to work when only the norm is asked for):
//   Disc   b - a s in one pass -> crtInv -> lInv -> the centred lift -> gSqNorm
//   Cont   a s -> crtInv -> lInv -> e = lift (b - x) in RRq -> gSqNorm
int lolhip_rlwe_error_batch(const lolhip_plan* pq, void* stream, int kind, const int64_t* a_crt, const void* b,
                            const int64_t* s_crt, void* e_out, void* norm_out, int64_t* work, int64_t B) {
  if (!pq || (kind != KIND_DISC && kind != KIND_CONT)) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (B < 0 || P.T > PIPE_MAX_T || (kind == KIND_CONT && P.T != 1)) return LOLHIP_ERR_INVALID;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (kind == KIND_DISC && !P.lift_ok) return LOLHIP_ERR_MODULUS;
  int rc = need_device(pq); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!a_crt || !b || !s_crt || !work || (!e_out && !norm_out) || (norm_out && !norm_ok(P))) return LOLHIP_ERR_INVALID;

  hipStream_t s = (hipStream_t)stream;
  const int64_t n = P.n;
  Work w(work);
  const auto [v, ew] = rlwe_work(w, P, kind, B);
  if (kind == KIND_DISC) {
    rc = as_dec(P, s, a_crt, static_cast<const int64_t*>(b), s_crt, v, B); if (rc) return rc;
    int64_t* e = e_out ? static_cast<int64_t*>(e_out) : ew;
    LiftParams lp = LiftParams();
    lp.T = P.T;
    if (launch_lift(s, v, nullptr, e, B * n, lp, false, P.d_lift, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
    if (!norm_out) return LOLHIP_OK;
    return hip_status(launch_gsqnorm_i64(s, e, static_cast<int64_t*>(norm_out), B, n, norm_dims(P)));
  }
  rc = as_dec(P, s, a_crt, nullptr, s_crt, v, B); if (rc) return rc;
  double* e = e_out ? static_cast<double*>(e_out) : reinterpret_cast<double*>(ew);
  if (launch_rlwe_cont_error(s, v, static_cast<const double*>(b), e, B * n, (double)P.qs[0]) != hipSuccess)
    return LOLHIP_ERR_HIP;
  if (!norm_out) return LOLHIP_OK;
  return hip_status(launch_gsqnorm_f64(s, e, static_cast<double*>(norm_out), B, n, norm_dims(P)));
}

// ---- RLWR rounding and check (RLWR.hs:34-44) ------------------------------------------------------------------------
int lolhip_rlwr_rounded_prod_batch(const lolhip_plan* pq, int64_t p, void* stream, const int64_t* a_crt,
                                   const int64_t* s_crt, int64_t* b_out, int64_t* work, int64_t B) {
  int rc = rlwr_setup(pq, p, B); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!a_crt || !s_crt || !b_out || !work) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  hipStream_t s = (hipStream_t)stream;
  rc = as_dec(P, s, a_crt, nullptr, s_crt, work, B); if (rc) return rc;
  return hip_status(launch_rlwr_round(s, work, b_out, B * P.n, P.qs[0], (u64)p));
}

int lolhip_rlwr_check_batch(const lolhip_plan* pq, int64_t p, void* stream, const int64_t* a_crt, const int64_t* b,
                            const int64_t* s_crt, int32_t* mismatch, int64_t* work, int64_t B) {
  int rc = rlwr_setup(pq, p, B); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!a_crt || !b || !s_crt || !mismatch || !work) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  hipStream_t s = (hipStream_t)stream;
  rc = as_dec(P, s, a_crt, nullptr, s_crt, work, B); if (rc) return rc;
  return hip_status(launch_rlwr_check(s, work, b, mismatch, B, P.n, P.qs[0], (u64)p));
}

// ---- error bounds (Continuous.hs:74-84, Discrete.hs:65-76), host only -------------------------------------------------
int lolhip_rlwe_error_bound(const lolhip_pp* pps, int npps, double svar, double eps, int kind, double* out) {
  if (npps < 0 || (npps > 0 && !pps) || !out || (kind != KIND_DISC && kind != KIND_CONT)) return LOLHIP_ERR_INVALID;
  if (!std::isfinite(svar) || !std::isfinite(eps) || svar <= 0 || eps <= 0 || eps >= 1) return LOLHIP_ERR_INVALID;
  std::vector<PP> v;
  int odd = 0;
  for (int i = 0; i < npps; ++i) {
    if (pps[i].prime < 2 || pps[i].exponent < 1 || !is_prime((u64)pps[i].prime)) return LOLHIP_ERR_INVALID;
    for (const PP& pe : v) if (pe.p == pps[i].prime) return LOLHIP_ERR_INVALID;
    v.push_back(PP{pps[i].prime, pps[i].exponent});
    odd += pps[i].prime != 2;
  }
  const double n = (double)totient_pps(v), mhat = (double)value_hat(value_pps(v));
  double st;
  if (!stabilize(std::log(eps) / n, &st)) return LOLHIP_ERR_INVALID;
  const double cont = mhat * n * svar * st;
  if (kind == KIND_CONT) { *out = cont; return LOLHIP_OK; }
  if (!stabilize(std::log(eps), &st)) return LOLHIP_ERR_INVALID;
  *out = std::ceil((double)((int64_t)1 << odd) * n * st + cont);
  return LOLHIP_OK;
}

}  // extern "C"
