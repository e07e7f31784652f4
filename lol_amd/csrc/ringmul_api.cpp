// lol_amd/csrc/ringmul_api.cpp — the C ABI of the exact ring product over moduli without a CRT basis
// (include/lolhip.h; the exact counterpart of the reference's CRT-over-C fallback, lol Cyc.hs:262-297, UCyc.hs:422-444).
// This file chooses and certifies the NTT primes, derives the per-component constants and lays the launch plans over
// the existing poly-mul / crt / crtInv / pointwise product and the two passes of ringmul.hip.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "ringmul.h"
#include "she_host.h"

using namespace lolhip;

namespace {

// Unsigned integers below 2^256 for the exactness bound: 2 C H^2 reaches 2^185 and a product of three primes 2^183.
struct Wide {
  u64 w[4] = {0, 0, 0, 0};
  bool ovf = false;
  explicit Wide(u64 x = 0) { w[0] = x; }
  Wide& operator*=(u64 f) {
    u128 carry = 0;
    for (int i = 0; i < 4; ++i) {
      const u128 t = (u128)w[i] * f + carry;
      w[i] = (u64)t;
      carry = t >> 64;
    }
    ovf = ovf || carry != 0;
    return *this;
  }
};
bool operator<(const Wide& a, const Wide& b) {
  if (a.ovf != b.ovf) return b.ovf;
  for (int i = 3; i >= 0; --i) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}

const u64 PRIME_CAP = (u64)1 << 61;
const u64 MAX_INDEX = (u64)1 << 30;          // the largest m lolhip_ringmul_moduli looks for primes at

// 2 C_m H^2, H = max_t floor(q_t / 2); false when the growth constant saturates or a modulus is out of range
bool product_bound(const std::vector<PP>& pps, const std::vector<u64>& qs, Wide& bound) {
  const u64 C = growth(pps);
  if (C >= ((u64)1 << 62)) return false;
  u64 H = 0;
  for (u64 q : qs) {
    if (q < 2 || q >= ((u64)1 << 62)) return false;
    H = std::max(H, q / 2);
  }
  bound = Wide(2);
  bound *= C;
  bound *= H;
  bound *= H;
  return true;
}

Wide power(u64 x, int k) {
  Wide p(1);
  for (int i = 0; i < k; ++i) p *= x;
  return p;
}

// the smallest x with x^k >= bound, or 0 when that is above 2^61
u64 root_up(const Wide& bound, int k) {
  if (power(PRIME_CAP, k) < bound) return 0;
  u64 lo = 0, hi = PRIME_CAP;                  // hi^k >= bound > ... the answer is in (lo, hi]
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    if (power(mid, k) < bound) lo = mid; else hi = mid;
  }
  return hi;
}

int64_t slab(const lolhip_ringmul* h, int64_t B) { return B * h->rm.T * h->pQ->P.n * h->rm.K; }

// work: the lifted a, then the lifted b, [B T][n][K] each and rounded
struct RingWork { int64_t *la, *lb; };
RingWork ring_work(Work& w, const lolhip_ringmul* h, int64_t B) {
  return {w.take(even(slab(h, B))), w.take(even(slab(h, B)))};
}

// INVALID for a batch whose rows or pointwise period leave 31 bits
bool batch_fits(const lolhip_ringmul* h, int64_t B) { return B <= 0x7fffffff / h->rm.T; }

}  // namespace

extern "C" {

int lolhip_ringmul_moduli(const lolhip_pp* pps, int npps, const int64_t* qs, int T, int64_t Qs[3]) {
  std::vector<PP> f;
  if (!to_pps(pps, npps, f) || !qs || T < 1 || !Qs || !valid_pps(f, MAX_INDEX)) return LOLHIP_ERR_INVALID;
  std::vector<u64> q;
  for (int t = 0; t < T; ++t) {
    if (qs[t] < 2 || qs[t] >= ((int64_t)1 << 62)) return LOLHIP_ERR_MODULUS;
    q.push_back((u64)qs[t]);
  }
  Wide bound;
  if (!product_bound(f, q, bound)) return LOLHIP_ERR_MODULUS;
  const u64 m = (u64)value_pps(f);
  for (int K = 1; K <= RING_MAX_K; ++K) {
    const u64 root = root_up(bound, K);
    if (!root) continue;
    u64 Q[RING_MAX_K] = {0, 0, 0}, lower = root;
    bool ok = true;
    for (int i = 0; i < K && ok; ++i) {
      Q[i] = first_good_q(m, lower);
      ok = Q[i] < PRIME_CAP;
      lower = Q[i];
    }
    // every prime exceeds the root, so the product exceeds root^K >= the bound; slide on should rounding ever bite
    while (ok) {
      Wide prod(1);
      for (int i = 0; i < K; ++i) prod *= Q[i];
      if (bound < prod) break;
      for (int i = 0; i + 1 < K; ++i) Q[i] = Q[i + 1];
      Q[K - 1] = first_good_q(m, Q[K - 1]);
      ok = Q[K - 1] < PRIME_CAP;
    }
    if (!ok) continue;
    for (int i = 0; i < RING_MAX_K; ++i) Qs[i] = i < K ? (int64_t)Q[i] : 0;
    return K;
  }
  return LOLHIP_ERR_MODULUS;
}

void lolhip_ringmul_destroy(lolhip_ringmul* h) { delete h; }

int lolhip_ringmul_create(const lolhip_plan* pq, const lolhip_plan* pQ, lolhip_ringmul** out) {
  if (!out) return LOLHIP_ERR_INVALID;
  *out = nullptr;
  if (!pq || !pQ) return LOLHIP_ERR_INVALID;
  const Plan &P = pq->P, &R = pQ->P;
  if (!same_index(P, R) || R.T > RING_MAX_K || P.T > RING_MAX_T || R.T < 1 || P.T < 1) return LOLHIP_ERR_INVALID;
  const int T = P.T, K = R.T;
  for (int i = 0; i < K; ++i) for (int j = 0; j < i; ++j) if (R.qs[(size_t)i] == R.qs[(size_t)j]) return LOLHIP_ERR_MODULUS;
  if (!R.has_crt) return LOLHIP_ERR_NO_CRT;
  Wide bound, prod(1);
  if (!product_bound(P.pps, P.qs, bound) || !R.lift_ok || R.lift_consts.size() != (size_t)(K + K * K + K))
    return LOLHIP_ERR_MODULUS;
  for (u64 Q : R.qs) prod *= Q;
  if (!(bound < prod)) return LOLHIP_ERR_MODULUS;

  lolhip_ringmul* h = new lolhip_ringmul;
  h->pQ = pQ;
  h->device = P.device && R.device;
  RingMul& rm = h->rm;
  rm.T = T;
  rm.K = K;
  rm.pow2 = 1;
  u64 Hmax = 0, Qmin = ~(u64)0;
  for (int t = 0; t < T; ++t) {
    const u64 q = P.qs[(size_t)t];
    rm.q[t] = make_modctx(q);
    if (q & (q - 1)) rm.pow2 = 0;
    Hmax = std::max(Hmax, q / 2);
    u64 p = 1 % q;
    for (int i = 0; i < K; ++i) {
      rm.pw[t][i] = p;
      p = mulmod(p, R.qs[(size_t)i] % q, q);
    }
    rm.Qp[t] = p;
  }
  for (int i = 0; i < K; ++i) {
    rm.Q[i] = make_modctx(R.qs[(size_t)i]);
    Qmin = std::min(Qmin, R.qs[(size_t)i]);
    rm.pinv[i] = R.lift_consts[(size_t)i];
    for (int j = 0; j < K; ++j) rm.qmod[i * RING_MAX_K + j] = R.lift_consts[(size_t)(K + i * K + j)];
    rm.half[i] = R.lift_consts[(size_t)(K + K * K + i)];
  }
  rm.wide = Qmin <= Hmax;
  *out = h;
  return LOLHIP_OK;
}

int64_t lolhip_ringmul_work_len(const lolhip_ringmul* h, int64_t B) {
  if (!h || B < 0 || !batch_fits(h, B)) return LOLHIP_ERR_INVALID;
  return measure(ring_work, h, B);
}

int lolhip_ringmul_batch(const lolhip_ringmul* h, void* stream, int64_t* out, const int64_t* a, const int64_t* b,
                         int64_t* work, int64_t B) {
  if (!h || B < 0 || !batch_fits(h, B)) return LOLHIP_ERR_INVALID;
  if (!h->device) return LOLHIP_ERR_NO_DEVICE;
  int rc = need_device(h->pQ); if (rc) return rc;
  if (B > 0 && (!out || !a || !b || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = h->pQ->P.n;
  Work w(work);
  const RingWork rw = ring_work(w, h, B);
  int64_t *la = rw.la, *lb = a == b ? la : rw.lb;
  if (launch_ring_lift(s, a, la, B, n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  if (a != b && launch_ring_lift(s, b, lb, B, n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = lolhip_polymul_batch(h->pQ, stream, la, la, lb, B * h->rm.T); if (rc) return rc;
  return hip_status(launch_ring_fold(s, la, out, B, n, h->rm));
}

int lolhip_ringmul_prepare(const lolhip_ringmul* h, void* stream, int64_t* bhat, const int64_t* b, int64_t* work,
                           int64_t Bb) {
  (void)work;
  if (!h || Bb < 0 || !batch_fits(h, Bb)) return LOLHIP_ERR_INVALID;
  if (!h->device) return LOLHIP_ERR_NO_DEVICE;
  int rc = need_device(h->pQ); if (rc) return rc;
  if (Bb > 0 && (!bhat || !b)) return LOLHIP_ERR_INVALID;
  if (Bb == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (launch_ring_lift(s, b, bhat, Bb, h->pQ->P.n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;
  return do_crt(h->pQ->P, s, bhat, Bb * h->rm.T, false);
}

int lolhip_ringmul_prepared_batch(const lolhip_ringmul* h, void* stream, int64_t* out, const int64_t* a,
                                  const int64_t* bhat, int64_t Bb, int64_t* work, int64_t B) {
  if (!h || B < 0 || !batch_fits(h, B) || (B > 0 && Bb != 1 && Bb != B)) return LOLHIP_ERR_INVALID;
  const int64_t period = slab(h, 1);
  if (B > 1 && Bb == 1 && period > 0x7fffffff) return LOLHIP_ERR_INVALID;
  if (!h->device) return LOLHIP_ERR_NO_DEVICE;
  int rc = need_device(h->pQ); if (rc) return rc;
  if (B > 0 && (!out || !a || !bhat || !work)) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const Plan& R = h->pQ->P;
  const int64_t total = slab(h, B), polys = B * h->rm.T;
  if (launch_ring_lift(s, a, work, B, R.n, h->rm) != hipSuccess) return LOLHIP_ERR_HIP;       // work: the lifted a alone
  rc = do_crt(R, s, work, polys, false); if (rc) return rc;
  if (launch_pointwise_mul(s, work, bhat, total, Bb == B ? total : period, R.T, R.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(R, s, work, polys, true); if (rc) return rc;
  return hip_status(launch_ring_fold(s, work, out, B, R.n, h->rm));
}

}  // extern "C"
