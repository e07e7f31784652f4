// lol_amd/csrc/encrypt_api.cpp — the C ABI of SymmSHE encrypt / genSK (include/lolhip.h; lol-apps SymmSHE.hs:120-146):
// host checks and the launch plan over the kernels of encrypt.hip and the existing transforms (the sampler's limits,
// deviation and key words are in sampler_internal.h).
#include <hip/hip_runtime_api.h>

#include "sampler_internal.h"

using namespace lolhip;

namespace {
// work: rep [B][n'] | double slab [B][n'] | e residues [B][n'][T], the last two for an index that is not a 2-power
struct EncWork { int64_t* rep; double* d; int64_t* e; };
EncWork enc_work(Work& w, const Plan& P, int64_t B) {
  EncWork r = {w.take(B * P.n), nullptr, nullptr};
  if (!two_power(P)) { r.d = w.take_f64(B * P.n); r.e = w.take(B * P.n * P.T); }
  return r;
}
}  // namespace

extern "C" {

void lolhip_chacha20_block(const uint8_t key[32], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
  chacha20_block(make_key(key), counter, nonce[0], nonce[1], nonce[2], out);
}

int64_t lolhip_encrypt_work_len(const lolhip_plan* pq, int64_t B) {
  if (!pq || B < 0) return LOLHIP_ERR_INVALID;
  return measure(enc_work, pq->P, B);
}

// Launch plan.  rep = lInv (embedPow pt) over pp, read straight from pt_pow when both are identities.
//   CRT out:       error -> c0 slot (residues) -> l -> crt -> k_enc_combine (c^1, c^0 = e^ - c^1 s^)
//   powerful out:  k_enc_uniform (c^1, -c^1 s^) -> one crtInv of 2B -> c0 += l (reduce e): in the fused pass for a
//                  2-power, else the rounding pass into work, l, one add pass
int lolhip_encrypt_batch(const lolhip_plan* pq, const lolhip_plan* pp, const lolhip_ext* x_p, void* stream,
                         const int64_t* pt_pow, const int64_t* s_crt, double svar, const uint8_t key[32], uint64_t ctr,
                         int out_crt, int64_t* cs_out, int64_t* work, int64_t B) {
  int rc = index_status(pq); if (rc) return rc;
  rc = need_device(pq); if (rc) return rc;
  if (!pp) return LOLHIP_ERR_INVALID;
  rc = need_device(pp); if (rc) return rc;
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
  Work w(work);
  const auto [rep, d, e] = enc_work(w, P, B);
  int64_t *c0 = cs_out, *c1 = cs_out + slab;

  // rep: the decoding-basis coefficients of embed pt over p
  const int64_t* rep_src = rep;
  if (x_p) {
    rc = lolhip_embed_pow_batch(x_p, stream, rep, pt_pow, B); if (rc) return rc;
    rc = run_prog_or_copy(PP, PP.prog_linv, s, rep, B); if (rc) return rc;
  } else if (!PP.prog_linv.stages.empty()) {
    rc = run_prog(PP, PP.prog_linv, s, rep, B, pt_pow); if (rc) return rc;
  } else {
    rep_src = pt_pow;
  }

  if (out_crt) {
    rc = sample_error(P, s, d, rep_src, p, c0, ENC_WRITE, k, ctr, CHACHA_DOM_ENC_GAUSS, sigma, B); if (rc) return rc;
    rc = run_prog_or_copy(P, P.prog_l, s, c0, B); if (rc) return rc;
    rc = do_crt(P, s, c0, B, false); if (rc) return rc;
    return hip_status(launch_enc_c1(s, true, c0, c1, s_crt, B, n, P.T, P.d_mod, k, ctr));
  }
  if (launch_enc_c1(s, false, c0, c1, s_crt, B, n, P.T, P.d_mod, k, ctr) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(P, s, cs_out, 2 * B, true); if (rc) return rc;
  if (pow2) return sample_error(P, s, d, rep_src, p, c0, ENC_ADD, k, ctr, CHACHA_DOM_ENC_GAUSS, sigma, B);
  rc = sample_error(P, s, d, rep_src, p, e, ENC_WRITE, k, ctr, CHACHA_DOM_ENC_GAUSS, sigma, B); if (rc) return rc;
  rc = run_prog(P, P.prog_l, s, e, B, nullptr); if (rc) return rc;
  return hip_status(launch_addmod(s, c0, e, B, n, P.T, P.d_mod));
}

// errorRounded svar = round (tGaussianDec svar), coefficient-wise (UCyc.hs:422-429): the sampler with p = 1, rep = 0,
// written as int64; for an index that is not a 2-power the double slab is z_dec itself (the rounding runs in place)
int lolhip_error_rounded_batch(const lolhip_plan* p, void* stream, double svar, const uint8_t key[32], uint64_t ctr,
                               int64_t* z_dec, int64_t* work, int64_t B) {
  (void)work;
  int rc = index_status(p); if (rc) return rc;
  rc = need_device(p); if (rc) return rc;
  const Plan& P = p->P;
  if (!svar_ok(svar) || B < 0) return LOLHIP_ERR_INVALID;
  rc = sampler_ok(P); if (rc) return rc;
  if (B > 0 && (!key || !z_dec)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  return sample_error(P, (hipStream_t)stream, reinterpret_cast<double*>(z_dec), nullptr, 1, z_dec, ENC_INT, make_key(key),
                      ctr, CHACHA_DOM_ERR_ROUNDED, deviation(P, svar), B);
}

}  // extern "C"
