// lol_amd/csrc/encrypt_api.cpp — the C ABI of SymmSHE encrypt / genSK (include/lolhip.h; lol-apps SymmSHE.hs:120-146):
// host checks, the deviation of the samplers and the launch plan over the kernels of encrypt.hip and the existing
// transforms.
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "capi_internal.h"
#include "kernels.h"
#include "rng_dev.h"

using namespace lolhip;

namespace {

constexpr int64_t POW2_MAX_N = 16384;        // 2-powers: no map, one fused pass (k_enc_error from the stream)

// every prime of the index is 2 (m' = 2^k, or 1): L and the Gaussian map are identities
bool two_power(const Plan& P) {
  for (const PP& pe : P.pps) if (pe.p != 2) return false;
  return true;
}

// LOLHIP_OK when the sampler takes this index: a 2-power up to n' = 16384, else the limits of the Gaussian map
int sampler_ok(const Plan& P) {
  if (two_power(P)) return P.n <= POW2_MAX_N ? LOLHIP_OK : LOLHIP_ERR_INVALID;
  return P.float_ok ? LOLHIP_OK : LOLHIP_ERR_INVALID;
}

// sigma = sqrt(v (m'/rad m') / 2 pi): the deviation of tGaussianDec v (scaled variance = 2 pi x variance,
// GaussRandom.hs:27-44; CPP.hs:376-389)
double deviation(const Plan& P, double v) {
  double mrad = 1.0;
  for (const PP& pe : P.pps)
    for (int i = 1; i < pe.e; ++i) mrad *= pe.p;
  return std::sqrt(v * mrad / 6.283185307179586);
}

ChaChaKey make_key(const uint8_t key[32]) {
  ChaChaKey k;
  for (int i = 0; i < 8; ++i)
    k.k[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 |
             (uint32_t)key[4 * i + 3] << 24;
  return k;
}

bool svar_ok(double svar) { return std::isfinite(svar) && svar > 0; }

// the double slab of the map and the sampled coefficients into [B][n] int64 / residues: one pass from the stream for a
// 2-power, else Gaussians -> k_gauss (the decoding-basis map of tGaussianDec) -> the rounding pass
int sample_error(const Plan& P, hipStream_t s, double* d, const int64_t* rep, int64_t p, int64_t* out, int mode,
                 const ChaChaKey& key, uint64_t ctr, int domain, double sigma, int64_t B) {
  if (two_power(P))
    return launch_enc_error(s, nullptr, rep, p, out, B, P.n, P.T, P.d_mod, mode, key, ctr, domain, sigma) == hipSuccess
               ? LOLHIP_OK : LOLHIP_ERR_HIP;
  if (launch_enc_gauss(s, d, B, P.n, key, ctr, domain, sigma) != hipSuccess) return LOLHIP_ERR_HIP;
  if (launch_gauss(s, d, B, P.n, P.prog_gauss.d_stages, P.prog_gauss.nstages, P.d_rconsts) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return launch_enc_error(s, d, rep, p, out, B, P.n, P.T, P.d_mod, mode, key, ctr, domain, sigma) == hipSuccess
             ? LOLHIP_OK : LOLHIP_ERR_HIP;
}

}  // namespace

extern "C" {

void lolhip_chacha20_block(const uint8_t key[32], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
  chacha20_block(make_key(key), counter, nonce[0], nonce[1], nonce[2], out);
}

int64_t lolhip_encrypt_work_len(const lolhip_plan* pq, int64_t B) {
  if (!pq || B < 0) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  return two_power(P) ? B * P.n : B * P.n * (2 + P.T);
}

// Launch plan (work: rep [B][n'] | double slab [B][n'] | e residues [B][n'][T], the last two for an index that is
// not a 2-power).  rep = lInv (embedPow pt) over pp, read straight from pt_pow when both are identities.
//   CRT out:       error -> c0 slot (residues) -> l -> crt -> k_enc_combine (c^1, c^0 = e^ - c^1 s^)
//   powerful out:  k_enc_uniform (c^1, -c^1 s^) -> one crtInv of 2B -> c0 += l (reduce e): in the fused pass for a
//                  2-power, else the rounding pass into work, l, one add pass
int lolhip_encrypt_batch(const lolhip_plan* pq, const lolhip_plan* pp, const lolhip_ext* x_p, void* stream,
                         const int64_t* pt_pow, const int64_t* s_crt, double svar, const uint8_t key[32], uint64_t ctr,
                         int out_crt, int64_t* cs_out, int64_t* work, int64_t B) {
  int rc = capi_need_device(pq); if (rc) return rc;
  if (!pp) return LOLHIP_ERR_INVALID;
  rc = capi_need_device(pp); if (rc) return rc;
  const Plan &P = pq->P, &PP = pp->P;
  if (!svar_ok(svar) || B < 0 || PP.T != 1 || PP.m != P.m || P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (x_p) {
    const ExtPlan& X = x_p->X;
    if (X.hi->m != PP.m || X.hi->qs != PP.qs) return LOLHIP_ERR_INVALID;
    if (!X.d_embed_pow) return LOLHIP_ERR_NO_DEVICE;
  }
  rc = sampler_ok(P); if (rc) return rc;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  const int64_t p = (int64_t)PP.qs[0];
  if (p < 2) return LOLHIP_ERR_MODULUS;
  if (B > 0 && (!pt_pow || !s_crt || !key || !cs_out || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const ChaChaKey k = make_key(key);
  const double sigma = deviation(P, svar * ((double)p * (double)p));
  const bool pow2 = two_power(P);
  const int64_t n = P.n, slab = B * n * P.T;
  int64_t* rep = work;
  double* d = pow2 ? nullptr : reinterpret_cast<double*>(work + B * n);
  int64_t* e = pow2 ? nullptr : work + 2 * B * n;
  int64_t *c0 = cs_out, *c1 = cs_out + slab;

  // rep: the decoding-basis coefficients of embed pt over p
  const int64_t* rep_src = rep;
  if (x_p) {
    rc = lolhip_embed_pow_batch(x_p, stream, rep, pt_pow, B); if (rc) return rc;
    if (!PP.prog_linv.stages.empty()) { rc = capi_run_prog(PP, PP.prog_linv, s, rep, B, nullptr); if (rc) return rc; }
  } else if (!PP.prog_linv.stages.empty()) {
    rc = capi_run_prog(PP, PP.prog_linv, s, rep, B, pt_pow); if (rc) return rc;
  } else {
    rep_src = pt_pow;
  }

  if (out_crt) {
    rc = sample_error(P, s, d, rep_src, p, c0, ENC_WRITE, k, ctr, CHACHA_DOM_ENC_GAUSS, sigma, B); if (rc) return rc;
    if (!P.prog_l.stages.empty()) { rc = capi_run_prog(P, P.prog_l, s, c0, B, nullptr); if (rc) return rc; }
    rc = capi_do_crt(P, s, c0, B, false); if (rc) return rc;
    return launch_enc_c1(s, true, c0, c1, s_crt, B, n, P.T, P.d_mod, k, ctr) == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP;
  }
  if (launch_enc_c1(s, false, c0, c1, s_crt, B, n, P.T, P.d_mod, k, ctr) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = capi_do_crt(P, s, cs_out, 2 * B, true); if (rc) return rc;
  if (pow2) return sample_error(P, s, d, rep_src, p, c0, ENC_ADD, k, ctr, CHACHA_DOM_ENC_GAUSS, sigma, B);
  rc = sample_error(P, s, d, rep_src, p, e, ENC_WRITE, k, ctr, CHACHA_DOM_ENC_GAUSS, sigma, B); if (rc) return rc;
  rc = capi_run_prog(P, P.prog_l, s, e, B, nullptr); if (rc) return rc;
  return launch_addmod(s, c0, e, B, n, P.T, P.d_mod) == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP;
}

// errorRounded svar = round (tGaussianDec svar), coefficient-wise (UCyc.hs:422-429): the sampler with p = 1, rep = 0,
// written as int64; for an index that is not a 2-power the double slab is z_dec itself (the rounding runs in place)
int lolhip_error_rounded_batch(const lolhip_plan* p, void* stream, double svar, const uint8_t key[32], uint64_t ctr,
                               int64_t* z_dec, int64_t* work, int64_t B) {
  (void)work;
  int rc = capi_need_device(p); if (rc) return rc;
  const Plan& P = p->P;
  if (!svar_ok(svar) || B < 0) return LOLHIP_ERR_INVALID;
  rc = sampler_ok(P); if (rc) return rc;
  if (B > 0 && (!key || !z_dec)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  return sample_error(P, (hipStream_t)stream, reinterpret_cast<double*>(z_dec), nullptr, 1, z_dec, ENC_INT, make_key(key),
                      ctr, CHACHA_DOM_ERR_ROUNDED, deviation(P, svar), B);
}

}  // extern "C"
