// lol_amd/csrc/ctmul_api.cpp — the C ABI of the SymmSHE ciphertext product (*) of any degree (include/lolhip.h; lol-apps
// SymmSHE.hs:438-452): the rule of (enc, k, l), host checks and the launch plan over k_ct_mul (ctmul.hip), k_ctmul
// (pipeline.hip) for two linear operands without a factor, and the existing transforms.
#include <hip/hip_runtime_api.h>

#include "ctmul.h"
#include "she_host.h"

using namespace lolhip;

namespace {

// work (powerful-basis operands only): the operands' copies, transformed in place there: a [na][B][n][T] | b
// [nb][B][n][T] (none for the square)
struct MulWork { int64_t *a, *b; };
MulWork mul_work(Work& w, const Plan& P, int na, int nb, bool cs_crt, bool square, int64_t B) {
  if (cs_crt) return {nullptr, nullptr};
  const int64_t slab = B * P.n * P.T;
  int64_t* a = w.take(na * slab);
  return {a, square ? a : w.take(nb * slab)};
}

bool counts_ok(int na, int nb) { return na >= 1 && na <= LOLHIP_CT_MUL_MAX && nb >= 1 && nb <= LOLHIP_CT_MUL_MAX; }

}  // namespace

extern "C" {

int lolhip_ct_mul_rule(const lolhip_plan* pq, int64_t p, int enc1, int64_t k1, int64_t l1, int enc2, int64_t k2,
                       int64_t l2, int64_t* alpha, int* enc_out, int64_t* k_out, int64_t* l_out) {
  if (!pq || !alpha || !enc_out || !k_out || !l_out || pq->P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if ((enc1 != 0 && enc1 != 1) || (enc2 != 0 && enc2 != 1) || k1 < 0 || k2 < 0) return LOLHIP_ERR_INVALID;
  if (!p_ok(p)) return LOLHIP_ERR_MODULUS;
  const Plan& P = pq->P;
  const u64 up = (u64)p;
  u64 zq[PIPE_MAX_T], zp = 1;
  const bool both_msd = enc1 == 1 && enc2 == 1;
  if (both_msd) {                                                 // toLSD ct1 * ct2 (:444)
    const int rc = encode_scales(P, p, false, zq, &zp); if (rc) return rc;
  }
  for (int t = 0; t < P.T; ++t) alpha[t] = both_msd ? (int64_t)zq[t] : (int64_t)(1 % P.qs[(size_t)t]);
  *enc_out = (enc1 == 0 && enc2 == 0) ? 0 : 1;                    // (CT LSD ..) * (CT d2 ..) = CT d2 (:447-452)
  *k_out = k1 + k2 + 1;
  *l_out = (int64_t)mulmod(encode_l(l1, zp, up), canon(l2, up), up);
  return LOLHIP_OK;
}

int64_t lolhip_ct_mul_work_len(const lolhip_plan* pq, int na, int nb, int cs_crt, int square, int64_t B) {
  if (!pq || !counts_ok(na, nb) || B < 0 || (square && na != nb)) return LOLHIP_ERR_INVALID;
  return measure(mul_work, pq->P, na, nb, cs_crt != 0, square != 0, B);
}

int lolhip_ct_mul_batch(const lolhip_plan* pq, void* stream, const int64_t* a, int na, const int64_t* b, int nb,
                        int cs_crt, const int64_t* alpha, int64_t* out, int out_crt, int64_t* work, int64_t B) {
  if (!pq) return LOLHIP_ERR_INVALID;
  const Plan& P = pq->P;
  if (!counts_ok(na, nb) || B < 0 || P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (B > 0 && (!a || !b || !out || (!cs_crt && !work))) return LOLHIP_ERR_INVALID;
  if (B > 0 && (out == a || out == b)) return LOLHIP_ERR_INVALID;  // na + nb - 1 components do not fit either input
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  int rc = need_device(pq); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  CtMulScale sc = CtMulScale();
  sc.T = P.T;
  bool unit = true;                                                // alpha_t = 1 for every t
  for (int t = 0; t < P.T; ++t) {
    const u64 q = P.qs[(size_t)t];
    sc.a[t] = alpha ? canon(alpha[t], q) : 1 % q;
    sc.ap[t] = make_shoup(sc.a[t], q).wp;
    unit = unit && sc.a[t] == 1 % q;
  }
  const bool square = b == a && nb == na;
  const int64_t slab = B * P.n * P.T;
  if (!cs_crt) {
    Work w(work);
    const MulWork mw = mul_work(w, P, na, nb, false, square, B);
    const size_t word = sizeof(int64_t);
    if (hipMemcpyAsync(mw.a, a, word * (size_t)(na * slab), hipMemcpyDeviceToDevice, s) != hipSuccess) return LOLHIP_ERR_HIP;
    if (!square && hipMemcpyAsync(mw.b, b, word * (size_t)(nb * slab), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return LOLHIP_ERR_HIP;
    rc = do_crt(P, s, mw.a, (int64_t)(na + (square ? 0 : nb)) * B, false); if (rc) return rc;   // the regions are adjacent
    a = mw.a;
    b = mw.b;
  }
  // linear x linear without a factor is what k_ctmul (pipeline.hip) computes: over three runs k_ct_mul<2, 2> measured
  // between 5 % faster and 3 % slower than it, more than the 0.2 % either differs from itself by
  if (na == 2 && nb == 2 && unit && !square)                      // the square stays: it reads its operand once
    rc = hip_status(launch_ctmul(s, a, a + slab, b, b + slab, out, out + slab, out + 2 * slab, P.d_gcrt, B, P.n, P.T, P.d_mod));
  else
    rc = hip_status(launch_ct_mul(s, a, na, b, nb, out, B, P.n, sc, P.d_gcrt, P.d_mod));
  if (rc) return rc;
  return out_crt ? LOLHIP_OK : do_crt(P, s, out, (int64_t)(na + nb - 1) * B, true);
}

}  // extern "C"
