// lol_amd/csrc/rlwe_ring_api.cpp — the C ABI of RLWE / RLWR instances over one modulus without a CRT basis
// (include/lolhip.h): the instances of rlwe_api.cpp with a s computed as the exact ring product of
// ringmul_api.cpp against a prepared secret.  Host checks and the launch plans over rlwe_ring.hip, ringmul.hip, the
// samplers of encrypt.hip, the element-wise passes of rlwe.hip and the existing transforms.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>

#include "kernels.h"
#include "rlwe_ring.h"
#include "sampler_internal.h"

using namespace lolhip;

namespace {

enum { KIND_DISC = 0, KIND_CONT = 1, KIND_RLWR = 2 };

// pq is the plan h was created from, as far as a handle remembers it: the index of pQ, one modulus, h's q
bool plan_of(const lolhip_ringmul* h, const lolhip_plan* pq) {
  const Plan& P = pq->P;
  return h->pQ && h->rm.T == 1 && P.T == 1 && same_index(P, h->pQ->P) && P.qs[0] == h->rm.q[0].q;
}

// the batches lolhip_ringmul_prepared_batch takes against one prepared element
bool batch_fits(const lolhip_ringmul* h, int64_t B) {
  return B >= 0 && B <= 0x7fffffff && (B <= 1 || h->pQ->P.n * h->rm.K <= 0x7fffffff);
}

bool norm_ok(const Plan& P) { return P.n <= NORM_MAX_N && norm_dims(P).k <= NORM_MAX_PRIMES; }

// statuses 1 to 3 of every entry (include/lolhip.h): the arguments, then the device
int setup(const lolhip_ringmul* h, const lolhip_plan* pq, int64_t B) {
  if (!h || !pq || !batch_fits(h, B) || !plan_of(h, pq)) return LOLHIP_ERR_INVALID;
  return LOLHIP_OK;
}
int devices(const lolhip_ringmul* h, const lolhip_plan* pq) {
  if (!h->device) return LOLHIP_ERR_NO_DEVICE;
  const int rc = need_device(pq);
  return rc ? rc : need_device(h->pQ);
}
bool rlwr_p_ok(const Plan& P, int64_t p) { return p >= 2 && (u64)p < P.qs[0]; }

// work: la, the lifted a and then the product [B][n][K] | x, residues of a s (or the addend l(e)) [B][n] | e, the double
// slab of the Gaussians / the error, or the lifted Disc error [B][n] (Disc and Cont)
struct RrWork { int64_t *la, *x, *e; };
RrWork rr_work(Work& w, const lolhip_ringmul* h, int kind, int64_t B) {
  const int64_t n = h->pQ->P.n;
  int64_t* la = w.take(even(B * n * h->rm.K));
  int64_t* x = w.take(even(B * n));
  return {la, x, kind == KIND_RLWR ? nullptr : w.take(even(B * n))};
}

// at a 2-power index the fold's tail finishes the call
bool fused_route(const Plan& P) { return two_power(P) && !sw(SW_RLWE_RING_UNFUSED); }

void info(const char* entry, int kind, bool fused, const lolhip_ringmul* h, int64_t B) {
  if (getenv("LOLHIP_RLWE_RING_INFO"))
    fprintf(stderr, "rlwe_ring: %s kind %d, route %s, K %d, n %lld, B %lld\n", entry, kind, fused ? "fused" : "unfused",
            h->rm.K, (long long)h->pQ->P.n, (long long)B);
}

// la <- crtInv (crt la . shat) on pQ: the integer product's residues
int product(const lolhip_ringmul* h, hipStream_t s, int64_t* la, const int64_t* shat, int64_t B) {
  const Plan& R = h->pQ->P;
  const int64_t period = R.n * h->rm.K;
  int rc = do_crt(R, s, la, B, false); if (rc) return rc;
  if (launch_pointwise_mul(s, la, shat, B * period, period, R.T, R.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  return do_crt(R, s, la, B, true);
}

// la <- the residues of a s for a given a
int product_of(const lolhip_ringmul* h, hipStream_t s, const int64_t* a_pow, int64_t* la, const int64_t* shat, int64_t B) {
  if (launch_ring_lift(s, a_pow, la, B, h->pQ->P.n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  return product(h, s, la, shat, B);
}

// x <- the decoding-basis residues of the folded la (the general route of Cont and RLWR)
int fold_dec(const lolhip_ringmul* h, const Plan& P, hipStream_t s, const int64_t* la, int64_t* x, int64_t B) {
  if (launch_ring_fold(s, la, x, B, P.n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  return run_prog_or_copy(P, P.prog_linv, s, x, B, nullptr);
}

int rlwr_setup(const lolhip_ringmul* h, const lolhip_plan* pq, int64_t p, int64_t B) {
  const int rc = setup(h, pq, B); if (rc) return rc;
  if (!rlwr_p_ok(pq->P, p)) return LOLHIP_ERR_INVALID;
  return devices(h, pq);
}

}  // namespace

extern "C" {

int64_t lolhip_rlwe_ring_work_len(const lolhip_ringmul* h, const lolhip_plan* pq, int kind, int64_t B) {
  if (kind < KIND_DISC || kind > KIND_RLWR) return LOLHIP_ERR_INVALID;
  const int rc = setup(h, pq, B); if (rc) return rc;
  return measure(rr_work, h, kind, B);
}

int lolhip_rlwe_ring_secret(const lolhip_ringmul* h, const lolhip_plan* pq, void* stream, const uint8_t key[32],
                            uint64_t ctr, int64_t* s_pow, int64_t* shat) {
  int rc = setup(h, pq, 1); if (rc) return rc;
  rc = devices(h, pq); if (rc) return rc;
  if (!key || !s_pow || !shat) return LOLHIP_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (launch_rr_draw_lift(s, s_pow, shat, 1, pq->P.n, h->rm, make_key(key), ctr, CHACHA_DOM_RLWE_SECRET) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return do_crt(h->pQ->P, s, shat, 1, false);
}

// Launch plans (include/lolhip.h): k_rr_draw_lift -> the product -> the way out of the kind
int lolhip_rlwe_ring_sample_batch(const lolhip_ringmul* h, const lolhip_plan* pq, void* stream, int kind, int64_t p,
                                  const int64_t* shat, double svar, const uint8_t key[32], uint64_t ctr, int64_t* a_pow,
                                  void* b_out, int64_t* work, int64_t B) {
  if (kind < KIND_DISC || kind > KIND_RLWR) return LOLHIP_ERR_INVALID;
  int rc = setup(h, pq, B); if (rc) return rc;
  const Plan& P = pq->P;
  if (kind == KIND_RLWR) {
    if (!rlwr_p_ok(P, p)) return LOLHIP_ERR_INVALID;
  } else {
    if (!svar_ok(svar)) return LOLHIP_ERR_INVALID;
    rc = sampler_ok(P); if (rc) return rc;
  }
  rc = devices(h, pq); if (rc) return rc;
  if (B > 0 && (!shat || !key || !a_pow || !b_out || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const int64_t n = P.n;
  const bool fused = fused_route(P);
  info("sample", kind, fused, h, B);
  Work w(work);
  const auto [la, x, e] = rr_work(w, h, kind, B);
  RrTail t = RrTail();
  t.key = make_key(key);
  t.ctr = ctr;
  t.p = (u64)p;
  if (kind != KIND_RLWR) t.sigma = deviation(P, svar);
  if (launch_rr_draw_lift(s, a_pow, la, B, n, h->rm, t.key, ctr, CHACHA_DOM_RLWE_UNIFORM) != hipSuccess)
    return LOLHIP_ERR_HIP;
  rc = product(h, s, la, shat, B); if (rc) return rc;
  if (fused) {
    const int tail = kind == KIND_DISC ? RR_DISC_SAMPLE : kind == KIND_CONT ? RR_CONT_SAMPLE : RR_RLWR;
    return hip_status(launch_rr_fold(s, tail, la, nullptr, b_out, B, n, h->rm, t));
  }
  if (kind == KIND_DISC) {
    // the addend l(e): the rounded Gaussians as residues mod q, then L on pq
    rc = sample_error(P, s, reinterpret_cast<double*>(e), nullptr, 1, x, ENC_WRITE, t.key, ctr, CHACHA_DOM_RLWE_GAUSS,
                      t.sigma, B);
    if (rc) return rc;
    rc = run_prog_or_copy(P, P.prog_l, s, x, B); if (rc) return rc;
    return hip_status(launch_rr_fold(s, RR_ADD, la, x, b_out, B, n, h->rm, t));
  }
  rc = fold_dec(h, P, s, la, x, B); if (rc) return rc;
  if (kind == KIND_RLWR)
    return hip_status(launch_rlwr_round(s, x, static_cast<int64_t*>(b_out), B * n, P.qs[0], (u64)p));
  double* g = reinterpret_cast<double*>(e);
  if (launch_enc_gauss(s, g, B, n, t.key, ctr, CHACHA_DOM_RLWE_GAUSS, t.sigma) != hipSuccess) return LOLHIP_ERR_HIP;
  if (!two_power(P) &&
      launch_gauss(s, g, B, n, P.prog_gauss.d_stages, P.gauss_word, P.d_rconsts) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return hip_status(launch_rlwe_cont_sample(s, x, g, static_cast<double*>(b_out), B * n, (double)P.qs[0]));
}

// Launch plans: k_ring_lift -> the product -> the way out; the lifted values go to e_out, or to work when only the norm
// is asked for; then gSqNorm
int lolhip_rlwe_ring_error_batch(const lolhip_ringmul* h, const lolhip_plan* pq, void* stream, int kind,
                                 const int64_t* a_pow, const void* b, const int64_t* shat, void* e_out, void* norm_out,
                                 int64_t* work, int64_t B) {
  if (kind != KIND_DISC && kind != KIND_CONT) return LOLHIP_ERR_INVALID;
  int rc = setup(h, pq, B); if (rc) return rc;
  const Plan& P = pq->P;
  rc = sampler_ok(P); if (rc) return rc;
  rc = devices(h, pq); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!a_pow || !b || !shat || !work || (!e_out && !norm_out) || (norm_out && !norm_ok(P))) return LOLHIP_ERR_INVALID;

  hipStream_t s = (hipStream_t)stream;
  const int64_t n = P.n;
  const bool fused = fused_route(P);
  info("error", kind, fused, h, B);
  Work w(work);
  const auto [la, x, ew] = rr_work(w, h, kind, B);
  const RrTail t = RrTail();
  rc = product_of(h, s, a_pow, la, shat, B); if (rc) return rc;
  if (kind == KIND_DISC) {
    int64_t* e = e_out ? static_cast<int64_t*>(e_out) : ew;
    if (fused) {
      if (launch_rr_fold(s, RR_DISC_ERROR, la, b, e, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
    } else {
      if (launch_rr_fold(s, RR_SUB, la, b, x, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
      rc = run_prog_or_copy(P, P.prog_linv, s, x, B, nullptr); if (rc) return rc;
      if (launch_rr_centre(s, x, e, B * n, P.qs[0]) != hipSuccess) return LOLHIP_ERR_HIP;
    }
    if (!norm_out) return LOLHIP_OK;
    return hip_status(launch_gsqnorm_i64(s, e, static_cast<int64_t*>(norm_out), B, n, norm_dims(P)));
  }
  double* e = e_out ? static_cast<double*>(e_out) : reinterpret_cast<double*>(ew);
  if (fused) {
    if (launch_rr_fold(s, RR_CONT_ERROR, la, b, e, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
  } else {
    rc = fold_dec(h, P, s, la, x, B); if (rc) return rc;
    if (launch_rlwe_cont_error(s, x, static_cast<const double*>(b), e, B * n, (double)P.qs[0]) != hipSuccess)
      return LOLHIP_ERR_HIP;
  }
  if (!norm_out) return LOLHIP_OK;
  return hip_status(launch_gsqnorm_f64(s, e, static_cast<double*>(norm_out), B, n, norm_dims(P)));
}

int lolhip_rlwr_ring_rounded_prod_batch(const lolhip_ringmul* h, const lolhip_plan* pq, int64_t p, void* stream,
                                        const int64_t* a_pow, const int64_t* shat, int64_t* b_out, int64_t* work,
                                        int64_t B) {
  int rc = rlwr_setup(h, pq, p, B); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!a_pow || !shat || !b_out || !work) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  hipStream_t s = (hipStream_t)stream;
  const bool fused = fused_route(P);
  info("rounded_prod", KIND_RLWR, fused, h, B);
  Work w(work);
  const auto [la, x, e] = rr_work(w, h, KIND_RLWR, B);
  (void)e;
  rc = product_of(h, s, a_pow, la, shat, B); if (rc) return rc;
  if (fused) {
    RrTail t = RrTail();
    t.p = (u64)p;
    return hip_status(launch_rr_fold(s, RR_RLWR, la, nullptr, b_out, B, P.n, h->rm, t));
  }
  rc = fold_dec(h, P, s, la, x, B); if (rc) return rc;
  return hip_status(launch_rlwr_round(s, x, b_out, B * P.n, P.qs[0], (u64)p));
}

// the counting pass reads x per sample: lInv (the identity at a 2-power) and k_rlwr_check at every index
int lolhip_rlwr_ring_check_batch(const lolhip_ringmul* h, const lolhip_plan* pq, int64_t p, void* stream,
                                 const int64_t* a_pow, const int64_t* b, const int64_t* shat, int32_t* mismatch,
                                 int64_t* work, int64_t B) {
  int rc = rlwr_setup(h, pq, p, B); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!a_pow || !b || !shat || !mismatch || !work) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  hipStream_t s = (hipStream_t)stream;
  info("check", KIND_RLWR, false, h, B);
  Work w(work);
  const auto [la, x, e] = rr_work(w, h, KIND_RLWR, B);
  (void)e;
  rc = product_of(h, s, a_pow, la, shat, B); if (rc) return rc;
  rc = fold_dec(h, P, s, la, x, B); if (rc) return rc;
  return hip_status(launch_rlwr_check(s, x, b, mismatch, B, P.n, P.qs[0], (u64)p));
}

}  // extern "C"
