// lol_amd/csrc/challenge_api.cpp — the C ABI of whole RLWE / RLWR challenges (include/lolhip.h; rlwe-challenges
// Generate.hs:105-218, Verify.hs:236-366): I instances of L samples generated in one call and verified in one call,
// every instance against its own secret.  lolhip_chall_*: moduli with a CRT basis (the plans of rlwe_api.cpp);
// lolhip_chall_ring_*: any single modulus (the plans of rlwe_ring_api.cpp).  Host checks and the launch plans over the
// grouped passes of challenge.hip, the kernels of rlwe.hip, rlwe_ring.hip and ringmul.hip, the samplers of
// encrypt.hip, the lift of decrypt.hip and the existing transforms.
#include <hip/hip_runtime_api.h>

#include "challenge.h"
#include "kernels.h"
#include "rlwe.h"
#include "rlwe_ring.h"
#include "sampler_internal.h"

using namespace lolhip;

namespace {

enum { KIND_DISC = 0, KIND_CONT = 1, KIND_RLWR = 2 };

bool norm_ok(const Plan& P) { return P.n <= NORM_MAX_N && norm_dims(P).k <= NORM_MAX_PRIMES; }

// work (B = I L), one layout for both calls:
//   sc   verify: the secrets in the CRT basis [I][n][T]
//   v    generate: the Gaussian map's double slab [B][n] (Disc) or a s [B][n] (Cont, RLWR);
//        verify: a in the CRT basis, then a s_i or b - a s_i and its decoding-basis residues [B][n][T]
//   bc   Disc verify: b in the CRT basis [B][n][T]
//   e    Disc, Cont: generate: the Gaussians (Cont); verify: the lifted error [B][n]
//   nm   verify: the norms [B] (int64 or double), or the mismatch counts [B] int32
struct ChallWork { int64_t *sc, *v, *bc, *e, *nm; };
ChallWork chall_work(Work& w, const Plan& P, int kind, int64_t I, int64_t L) {
  const int64_t B = I * L, nT = P.n * P.T;
  ChallWork c;
  c.sc = w.take(even(I * nT));
  c.v = w.take(even(B * nT));
  c.bc = kind == KIND_DISC ? w.take(even(B * nT)) : nullptr;
  c.e = kind == KIND_RLWR ? nullptr : w.take(even(B * P.n));
  c.nm = w.take(even(B));
  return c;
}

// statuses of both calls that need neither pointers nor the device (include/lolhip.h), in the order of lolhip_rlwe_*
bool shape_ok(const lolhip_plan* pq, int kind, int64_t I, int64_t L) {
  return pq && kind >= KIND_DISC && kind <= KIND_RLWR && I >= 0 && L >= 1 && I <= CHALL_MAX_ITEMS / L;
}

int host_checks(const lolhip_plan* pq, int kind, int64_t p, int64_t I, int64_t L) {
  if (!shape_ok(pq, kind, I, L)) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (P.T > PIPE_MAX_T || (kind != KIND_DISC && P.T != 1)) return LOLHIP_ERR_INVALID;
  if (kind == KIND_RLWR && !(p >= 2 && (u64)p < P.qs[0])) return LOLHIP_ERR_INVALID;
  return LOLHIP_OK;
}

// CRT basis -> decoding basis in place
int to_dec(const Plan& P, hipStream_t s, int64_t* y, int64_t B) {
  const int rc = do_crt(P, s, y, B, true);
  return rc ? rc : run_prog_or_copy(P, P.prog_linv, s, y, B, nullptr);
}

// decoding basis (src) -> CRT basis (y)
int to_crt(const Plan& P, hipStream_t s, const int64_t* src, int64_t* y, int64_t B) {
  const int rc = run_prog_or_copy(P, P.prog_l, s, y, B, src);
  return rc ? rc : do_crt(P, s, y, B, false);
}

// ---- the ring route: one modulus without a CRT basis, a s_i the exact ring product against prepared secrets ------------
// pq is the plan h was created from (rlwe_ring_api.cpp): the index of pQ, one modulus, h's q
bool plan_of(const lolhip_ringmul* h, const lolhip_plan* pq) {
  const Plan& P = pq->P;
  return h->pQ && h->rm.T == 1 && P.T == 1 && same_index(P, h->pQ->P) && P.qs[0] == h->rm.q[0].q;
}

bool ring_shape_ok(const lolhip_ringmul* h, const lolhip_plan* pq, int kind, int64_t I, int64_t L) {
  // a row of n K words is indexed in 32 bits (launch_chall_as), whatever the item count
  return h && shape_ok(pq, kind, I, L) && plan_of(h, pq) && pq->P.n * h->rm.K <= 0x7fffffff;
}

int ring_devices(const lolhip_ringmul* h, const lolhip_plan* pq) {
  if (!h->device) return LOLHIP_ERR_NO_DEVICE;
  const int rc = need_device(pq);
  return rc ? rc : need_device(h->pQ);
}

bool fused_route(const Plan& P) { return two_power(P) && !sw(SW_RLWE_RING_UNFUSED); }

// work (B = I L), one layout for both calls, every region an even count of words:
//   shat  the prepared secrets [I][n][K]
//   la    the lifted a, then the products [B][n][K]
//   x     residues of a s_i, or the addend l(e) [B][n]
//   e     Disc, Cont: the double slab of the Gaussians / the error, or the lifted Disc error [B][n]
//   sp    verify: the secrets in the powerful basis [I][n]
//   ap    verify: a in the powerful basis [B][n]
//   bp    Disc verify: b in the powerful basis [B][n]
//   nm    verify: the norms [B] (int64 or double), or the mismatch counts [B] int32
struct RingWork { int64_t *shat, *la, *x, *e, *sp, *ap, *bp, *nm; };
RingWork ring_work(Work& w, const lolhip_ringmul* h, int kind, int64_t I, int64_t L) {
  const int64_t n = h->pQ->P.n, B = I * L;
  RingWork c;
  c.shat = w.take(even(I * n * h->rm.K));
  c.la = w.take(even(B * n * h->rm.K));
  c.x = w.take(even(B * n));
  c.e = kind == KIND_RLWR ? nullptr : w.take(even(B * n));
  c.sp = w.take(even(I * n));
  c.ap = w.take(even(B * n));
  c.bp = kind == KIND_DISC ? w.take(even(B * n)) : nullptr;
  c.nm = w.take(even(B));
  return c;
}

// la <- crtInv (crt la . shat_(b / L)) on pQ: the integer products' residues
int ring_product(const lolhip_ringmul* h, hipStream_t s, int64_t* la, const int64_t* shat, int64_t I, int64_t L) {
  const Plan& R = h->pQ->P;
  int rc = do_crt(R, s, la, I * L, false); if (rc) return rc;
  if (launch_chall_as(s, la, nullptr, shat, la, I, L, R.n, R.T, R.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  return do_crt(R, s, la, I * L, true);
}

// x <- the decoding-basis residues of the folded la
int fold_dec(const lolhip_ringmul* h, const Plan& P, hipStream_t s, const int64_t* la, int64_t* x, int64_t B) {
  if (launch_ring_fold(s, la, x, B, P.n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  return run_prog_or_copy(P, P.prog_linv, s, x, B, nullptr);
}

}  // namespace

extern "C" {

int64_t lolhip_chall_work_len(const lolhip_plan* pq, int kind, int64_t I, int64_t L) {
  if (!shape_ok(pq, kind, I, L)) return LOLHIP_ERR_INVALID;
  return measure(chall_work, pq->P, kind, I, L);
}

// Launch plans: the I secrets as I items of domain 7 -> the plan of lolhip_rlwe_sample_batch over B = I L items with
// the grouped pass in place of the broadcast one -> crtInv, lInv of s, a (and the Disc b)
int lolhip_chall_generate_batch(const lolhip_plan* pq, void* stream, int kind, int64_t p, double svar,
                                const uint8_t key[32], uint64_t ctr_s, uint64_t ctr, int64_t I, int64_t L, int64_t* s_out,
                                int64_t* a_out, void* b_out, int64_t* work) {
  int rc = host_checks(pq, kind, p, I, L); if (rc) return rc;
  const Plan& P = pq->P;
  if (kind != KIND_RLWR) {
    if (!svar_ok(svar)) return LOLHIP_ERR_INVALID;
    rc = sampler_ok(P); if (rc) return rc;
  }
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  rc = need_device(pq); if (rc) return rc;
  if (I > 0 && (!key || !s_out || !a_out || !b_out || !work)) return LOLHIP_ERR_INVALID;
  if (I == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const ChaChaKey k = make_key(key);
  const int64_t n = P.n, B = I * L;
  Work w(work);
  const ChallWork c = chall_work(w, P, kind, I, L);
  if (launch_rlwe_uniform(s, RLWE_U_ONLY, s_out, nullptr, nullptr, I, n, P.T, P.d_mod, k, ctr_s, CHACHA_DOM_RLWE_SECRET) !=
      hipSuccess)
    return LOLHIP_ERR_HIP;
  if (kind == KIND_DISC) {
    int64_t* b = static_cast<int64_t*>(b_out);
    rc = sample_error(P, s, reinterpret_cast<double*>(c.v), nullptr, 1, b, ENC_WRITE, k, ctr, CHACHA_DOM_RLWE_GAUSS,
                      deviation(P, svar), B);
    if (rc) return rc;
    rc = to_crt(P, s, nullptr, b, B); if (rc) return rc;
    if (launch_chall_uniform(s, RLWE_U_ADD, a_out, s_out, b, I, L, n, P.T, P.d_mod, k, ctr, CHACHA_DOM_RLWE_UNIFORM) !=
        hipSuccess)
      return LOLHIP_ERR_HIP;
    rc = to_dec(P, s, b, B); if (rc) return rc;
  } else {
    int64_t* x = c.v;
    if (launch_chall_uniform(s, RLWE_U_PROD, a_out, s_out, x, I, L, n, 1, P.d_mod, k, ctr, CHACHA_DOM_RLWE_UNIFORM) !=
        hipSuccess)
      return LOLHIP_ERR_HIP;
    rc = to_dec(P, s, x, B); if (rc) return rc;
    if (kind == KIND_RLWR) {
      if (launch_rlwr_round(s, x, static_cast<int64_t*>(b_out), B * n, P.qs[0], (u64)p) != hipSuccess) return LOLHIP_ERR_HIP;
    } else {
      double* g = reinterpret_cast<double*>(c.e);
      if (launch_enc_gauss(s, g, B, n, k, ctr, CHACHA_DOM_RLWE_GAUSS, deviation(P, svar)) != hipSuccess) return LOLHIP_ERR_HIP;
      if (!two_power(P) &&
          launch_gauss(s, g, B, n, P.prog_gauss.d_stages, P.gauss_word, P.d_rconsts) != hipSuccess)
        return LOLHIP_ERR_HIP;
      if (launch_rlwe_cont_sample(s, x, g, static_cast<double*>(b_out), B * n, (double)P.qs[0]) != hipSuccess)
        return LOLHIP_ERR_HIP;
    }
  }
  rc = to_dec(P, s, a_out, B); if (rc) return rc;
  return to_dec(P, s, s_out, I);
}

// Launch plans: l, crt of s and a (and the Disc b) -> the grouped a s_i or b - a s_i -> crtInv, lInv -> the error and
// norm passes of lolhip_rlwe_error_batch / the counting pass of lolhip_rlwr_check_batch -> the verdict
int lolhip_chall_verify_batch(const lolhip_plan* pq, void* stream, int kind, int64_t p, int64_t bound_disc,
                              double bound_cont, int64_t I, int64_t L, const int64_t* s_dec, const int64_t* a_dec,
                              const void* b, int32_t* fails, void* worst, int64_t* work) {
  int rc = host_checks(pq, kind, p, I, L); if (rc) return rc;
  const Plan& P = pq->P;
  if (kind != KIND_RLWR && !norm_ok(P)) return LOLHIP_ERR_INVALID;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (kind == KIND_DISC && !P.lift_ok) return LOLHIP_ERR_MODULUS;
  rc = need_device(pq); if (rc) return rc;
  if (I > 0 && (!s_dec || !a_dec || !b || !fails || !worst || !work)) return LOLHIP_ERR_INVALID;
  if (I == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const int64_t n = P.n, B = I * L;
  Work w(work);
  const ChallWork c = chall_work(w, P, kind, I, L);
  rc = to_crt(P, s, s_dec, c.sc, I); if (rc) return rc;
  rc = to_crt(P, s, a_dec, c.v, B); if (rc) return rc;
  const int64_t* bc = nullptr;
  if (kind == KIND_DISC) {
    rc = to_crt(P, s, static_cast<const int64_t*>(b), c.bc, B); if (rc) return rc;
    bc = c.bc;
  }
  if (launch_chall_as(s, c.v, bc, c.sc, c.v, I, L, n, P.T, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = to_dec(P, s, c.v, B); if (rc) return rc;
  if (kind == KIND_DISC) {
    LiftParams lp = LiftParams();
    lp.T = P.T;
    if (launch_lift(s, c.v, nullptr, c.e, B * n, lp, false, P.d_lift, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
    if (launch_gsqnorm_i64(s, c.e, c.nm, B, n, norm_dims(P)) != hipSuccess) return LOLHIP_ERR_HIP;
    return hip_status(launch_chall_verdict_i64(s, c.nm, bound_disc, fails, static_cast<int64_t*>(worst), I, L));
  }
  if (kind == KIND_CONT) {
    double *e = reinterpret_cast<double*>(c.e), *nm = reinterpret_cast<double*>(c.nm);
    if (launch_rlwe_cont_error(s, c.v, static_cast<const double*>(b), e, B * n, (double)P.qs[0]) != hipSuccess)
      return LOLHIP_ERR_HIP;
    if (launch_gsqnorm_f64(s, e, nm, B, n, norm_dims(P)) != hipSuccess) return LOLHIP_ERR_HIP;
    return hip_status(launch_chall_verdict_f64(s, nm, bound_cont, fails, static_cast<double*>(worst), I, L));
  }
  int32_t* mm = reinterpret_cast<int32_t*>(c.nm);
  if (launch_rlwr_check(s, c.v, static_cast<const int64_t*>(b), mm, B, n, P.qs[0], (u64)p) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return hip_status(launch_chall_verdict_rlwr(s, mm, fails, static_cast<int64_t*>(worst), I, L));
}

// ---- the ring route ---------------------------------------------------------------------------------------------------
int64_t lolhip_chall_ring_work_len(const lolhip_ringmul* h, const lolhip_plan* pq, int kind, int64_t I, int64_t L) {
  if (!ring_shape_ok(h, pq, kind, I, L)) return LOLHIP_ERR_INVALID;
  return measure(ring_work, h, kind, I, L);
}

// Launch plans: the I secrets drawn and lifted in one launch, crt on pQ -> the plan of lolhip_rlwe_ring_sample_batch
// over B = I L items with the grouped product -> lInv on pq of s, a (and the Disc b)
int lolhip_chall_ring_generate_batch(const lolhip_ringmul* h, const lolhip_plan* pq, void* stream, int kind, int64_t p,
                                     double svar, const uint8_t key[32], uint64_t ctr_s, uint64_t ctr, int64_t I, int64_t L,
                                     int64_t* s_out, int64_t* a_out, void* b_out, int64_t* work) {
  if (!ring_shape_ok(h, pq, kind, I, L)) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  int rc;
  if (kind == KIND_RLWR) {
    if (!(p >= 2 && (u64)p < P.qs[0])) return LOLHIP_ERR_INVALID;
  } else {
    if (!svar_ok(svar)) return LOLHIP_ERR_INVALID;
    rc = sampler_ok(P); if (rc) return rc;
  }
  rc = ring_devices(h, pq); if (rc) return rc;
  if (I > 0 && (!key || !s_out || !a_out || !b_out || !work)) return LOLHIP_ERR_INVALID;
  if (I == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const Plan& R = h->pQ->P;
  const int64_t n = P.n, B = I * L;
  const bool fused = fused_route(P);
  Work w(work);
  const RingWork c = ring_work(w, h, kind, I, L);
  RrTail t = RrTail();
  t.key = make_key(key);
  t.ctr = ctr;
  t.p = (u64)p;
  if (kind != KIND_RLWR) t.sigma = deviation(P, svar);
  if (launch_rr_draw_lift(s, s_out, c.shat, I, n, h->rm, t.key, ctr_s, CHACHA_DOM_RLWE_SECRET) != hipSuccess)
    return LOLHIP_ERR_HIP;
  rc = do_crt(R, s, c.shat, I, false); if (rc) return rc;
  if (launch_rr_draw_lift(s, a_out, c.la, B, n, h->rm, t.key, ctr, CHACHA_DOM_RLWE_UNIFORM) != hipSuccess)
    return LOLHIP_ERR_HIP;
  rc = ring_product(h, s, c.la, c.shat, I, L); if (rc) return rc;
  if (fused) {
    const int tail = kind == KIND_DISC ? RR_DISC_SAMPLE : kind == KIND_CONT ? RR_CONT_SAMPLE : RR_RLWR;
    if (launch_rr_fold(s, tail, c.la, nullptr, b_out, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
  } else if (kind == KIND_DISC) {
    rc = sample_error(P, s, reinterpret_cast<double*>(c.e), nullptr, 1, c.x, ENC_WRITE, t.key, ctr, CHACHA_DOM_RLWE_GAUSS,
                      t.sigma, B);
    if (rc) return rc;
    rc = run_prog_or_copy(P, P.prog_l, s, c.x, B); if (rc) return rc;
    if (launch_rr_fold(s, RR_ADD, c.la, c.x, b_out, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
  } else {
    rc = fold_dec(h, P, s, c.la, c.x, B); if (rc) return rc;
    if (kind == KIND_RLWR) {
      if (launch_rlwr_round(s, c.x, static_cast<int64_t*>(b_out), B * n, P.qs[0], (u64)p) != hipSuccess) return LOLHIP_ERR_HIP;
    } else {
      double* g = reinterpret_cast<double*>(c.e);
      if (launch_enc_gauss(s, g, B, n, t.key, ctr, CHACHA_DOM_RLWE_GAUSS, t.sigma) != hipSuccess) return LOLHIP_ERR_HIP;
      if (!two_power(P) &&
          launch_gauss(s, g, B, n, P.prog_gauss.d_stages, P.gauss_word, P.d_rconsts) != hipSuccess)
        return LOLHIP_ERR_HIP;
      if (launch_rlwe_cont_sample(s, c.x, g, static_cast<double*>(b_out), B * n, (double)P.qs[0]) != hipSuccess)
        return LOLHIP_ERR_HIP;
    }
  }
  // powerful -> decoding basis
  if (kind == KIND_DISC) {
    rc = run_prog_or_copy(P, P.prog_linv, s, static_cast<int64_t*>(b_out), B, nullptr); if (rc) return rc;
  }
  rc = run_prog_or_copy(P, P.prog_linv, s, a_out, B, nullptr); if (rc) return rc;
  return run_prog_or_copy(P, P.prog_linv, s, s_out, I, nullptr);
}

// Launch plans: l on pq of s, a (and the Disc b) -> k_ring_lift of s and a, crt on pQ -> the grouped product -> the way
// out of lolhip_rlwe_ring_error_batch / lolhip_rlwr_ring_check_batch -> the verdict
int lolhip_chall_ring_verify_batch(const lolhip_ringmul* h, const lolhip_plan* pq, void* stream, int kind, int64_t p,
                                   int64_t bound_disc, double bound_cont, int64_t I, int64_t L, const int64_t* s_dec,
                                   const int64_t* a_dec, const void* b, int32_t* fails, void* worst, int64_t* work) {
  if (!ring_shape_ok(h, pq, kind, I, L)) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  int rc;
  if (kind == KIND_RLWR) {
    if (!(p >= 2 && (u64)p < P.qs[0])) return LOLHIP_ERR_INVALID;
  } else {
    rc = sampler_ok(P); if (rc) return rc;
    if (!norm_ok(P)) return LOLHIP_ERR_INVALID;
  }
  rc = ring_devices(h, pq); if (rc) return rc;
  if (I > 0 && (!s_dec || !a_dec || !b || !fails || !worst || !work)) return LOLHIP_ERR_INVALID;
  if (I == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  const Plan& R = h->pQ->P;
  const int64_t n = P.n, B = I * L;
  const bool fused = fused_route(P);
  Work w(work);
  const RingWork c = ring_work(w, h, kind, I, L);
  const RrTail t = RrTail();
  rc = run_prog_or_copy(P, P.prog_l, s, c.sp, I, s_dec); if (rc) return rc;
  if (launch_ring_lift(s, c.sp, c.shat, I, n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(R, s, c.shat, I, false); if (rc) return rc;
  rc = run_prog_or_copy(P, P.prog_l, s, c.ap, B, a_dec); if (rc) return rc;
  if (launch_ring_lift(s, c.ap, c.la, B, n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = ring_product(h, s, c.la, c.shat, I, L); if (rc) return rc;
  if (kind == KIND_DISC) {
    rc = run_prog_or_copy(P, P.prog_l, s, c.bp, B, static_cast<const int64_t*>(b)); if (rc) return rc;
    if (fused) {
      if (launch_rr_fold(s, RR_DISC_ERROR, c.la, c.bp, c.e, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
    } else {
      if (launch_rr_fold(s, RR_SUB, c.la, c.bp, c.x, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
      rc = run_prog_or_copy(P, P.prog_linv, s, c.x, B, nullptr); if (rc) return rc;
      if (launch_rr_centre(s, c.x, c.e, B * n, P.qs[0]) != hipSuccess) return LOLHIP_ERR_HIP;
    }
    if (launch_gsqnorm_i64(s, c.e, c.nm, B, n, norm_dims(P)) != hipSuccess) return LOLHIP_ERR_HIP;
    return hip_status(launch_chall_verdict_i64(s, c.nm, bound_disc, fails, static_cast<int64_t*>(worst), I, L));
  }
  if (kind == KIND_CONT) {
    double *e = reinterpret_cast<double*>(c.e), *nm = reinterpret_cast<double*>(c.nm);
    if (fused) {
      if (launch_rr_fold(s, RR_CONT_ERROR, c.la, b, e, B, n, h->rm, t) != hipSuccess) return LOLHIP_ERR_HIP;
    } else {
      rc = fold_dec(h, P, s, c.la, c.x, B); if (rc) return rc;
      if (launch_rlwe_cont_error(s, c.x, static_cast<const double*>(b), e, B * n, (double)P.qs[0]) != hipSuccess)
        return LOLHIP_ERR_HIP;
    }
    if (launch_gsqnorm_f64(s, e, nm, B, n, norm_dims(P)) != hipSuccess) return LOLHIP_ERR_HIP;
    return hip_status(launch_chall_verdict_f64(s, nm, bound_cont, fails, static_cast<double*>(worst), I, L));
  }
  int32_t* mm = reinterpret_cast<int32_t*>(c.nm);
  rc = fold_dec(h, P, s, c.la, c.x, B); if (rc) return rc;
  if (launch_rlwr_check(s, c.x, static_cast<const int64_t*>(b), mm, B, n, P.qs[0], (u64)p) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return hip_status(launch_chall_verdict_rlwr(s, mm, fails, static_cast<int64_t*>(worst), I, L));
}

}  // extern "C"
