// lol_amd/csrc/gadget_api.cpp — the C ABI of gadget error correction and Gadget.encode plus noise (include/lolhip.h;
// Correct gad (Cyc t m zq), lol Cyc.hs:615-621 over Gadget.hs:84-134 and ZqBasic.hs:234-314).  This file derives the
// per-component constants, decides the domain (the bound under which every value of the kernel fits
// int64) and lays the basis change in front of the one launch of gadget.hip.
#include <hip/hip_runtime_api.h>

#include <algorithm>

#include "gadget.h"
#include "she_host.h"

using namespace lolhip;

namespace {

// Saturating arithmetic for the bound: anything at or above 2^100 is "too large" (the limit is 2^63; operands are
// below 2^100, so no sum or product of two of them reaches 2^128 unnoticed).
const u128 SAT = (u128)1 << 100;
u128 sat_add(u128 a, u128 b) { return std::min(a + b, SAT); }
u128 sat_mul(u128 a, u128 b) {
  if (a == 0 || b == 0) return 0;
  return a >= SAT / b ? SAT : std::min(a * b, SAT);
}

// E >= |v'_i|, |e_i| over ALL inputs of one modulus with k >= 2 digits of base b, saturated; g = b^(k-1)
u128 error_bound(u64 q, u64 b, int k, u64 g) {
  const u128 h = q / 2;
  const u128 W = std::max(((u128)b + 2) * h / q, ((u128)b * h + q - 1) / q);          // >= |w_i|
  u64 bp[64], qf[64], rm[64];                                                         // b^i; floor(q / b^(j+1)); q mod b^(j+1)
  bp[0] = 1;
  for (int i = 1; i < k; ++i) bp[i] = bp[i - 1] * b;                                  // <= b^(k-1) <= q
  for (int j = 0; j + 1 < k; ++j) { qf[j] = q / bp[j + 1]; rm[j] = q % bp[j + 1]; }
  u128 Y[64];
  for (int i = 0; i < k; ++i) {
    u128 a = 0, f = 0;
    for (int j = 0; j < i; ++j) a += (u128)bp[i - 1 - j] * rm[j];                     // each term < b^i <= q
    for (int j = i; j + 1 < k; ++j) f += qf[j];                                       // <= q
    Y[i] = sat_mul(W, sat_add(a, sat_mul(bp[i], f)));                                 // >= |y_i|
  }
  const u128 S = sat_add(sat_add(h, Y[k - 1]), ((u128)g + 1) / 2) / g;                // >= |s|
  u128 E = 0;
  for (int i = 0; i < k; ++i) E = std::max(E, sat_add(sat_add(h, Y[i]), sat_mul(S, bp[i])));
  return E;
}

// the constants of one correct call over the plan's moduli, or why the tuple is refused
int make_correct(const Plan& P, int64_t base, CorrectParams& c) {
  if (P.T > GADGET_MAX_T) return LOLHIP_ERR_INVALID;
  int rc = make_decomp(P, base, c.d); if (rc) return rc;
  const u128 LIMIT = (u128)1 << 63;
  for (int t = 0; t < GADGET_MAX_T; ++t) {
    c.g[t] = 1; c.gmagic[t] = 1; c.gsh1[t] = c.gsh2[t] = 0;
    c.qo[t] = 1; c.qo_mod[t] = 1; c.qo_inv[t] = 1;
  }
  for (int t = 0; t < P.T; ++t) {
    const u64 q = P.qs[(size_t)t], qo = P.T == 2 ? P.qs[(size_t)(1 - t)] : 1;
    if (P.T == 2) {
      c.qo[t] = qo;
      c.qo_mod[t] = qo % q;
      c.qo_inv[t] = invmod(qo % q, q);
      if (c.qo_inv[t] == 0) return LOLHIP_ERR_MODULUS;                                // not coprime
    }
    const int k = c.d.k[t];
    if (k < 2) continue;                                                              // e' = [0]: the errors are the xo alone
    for (int i = 1; i < k; ++i) c.g[t] *= (u64)base;
    inv_div(c.g[t], c.gmagic[t], c.gsh1[t], c.gsh2[t]);
    const u128 E = error_bound(q, (u64)base, k, c.g[t]);
    if (sat_add(E, c.g[t]) >= LIMIT) return LOLHIP_ERR_MODULUS;
    if (P.T == 2 && sat_add(qo / 2, sat_mul(qo, E)) >= LIMIT) return LOLHIP_ERR_MODULUS;
  }
  return LOLHIP_OK;
}

bool basis_ok(int basis) { return basis == LOLHIP_BASIS_DEC || basis == LOLHIP_BASIS_POW || basis == LOLHIP_BASIS_CRT; }

// work: the copy the basis change runs on, [L][B][n][T] (nothing for the decoding basis)
int64_t* correct_work(Work& w, const Plan& P, int L, int basis, int64_t B) {
  return w.take(basis == LOLHIP_BASIS_DEC ? 0 : (int64_t)L * B * P.n * P.T);
}

// every status of a correct call that does not depend on its pointers
int correct_status(const lolhip_plan* p, int64_t base, int basis, int64_t B, CorrectParams& c) {
  if (!p) return LOLHIP_ERR_INVALID;
  int rc = make_correct(p->P, base, c); if (rc) return rc;
  if (!basis_ok(basis) || B < 0) return LOLHIP_ERR_INVALID;
  if (basis == LOLHIP_BASIS_CRT && !p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  return LOLHIP_OK;
}

}  // namespace

extern "C" {

int64_t lolhip_gadget_correct_work_len(const lolhip_plan* p, int64_t base, int basis, int64_t B) {
  CorrectParams c;
  int rc = correct_status(p, base, basis, B, c); if (rc) return rc;
  return measure(correct_work, p->P, c.d.L, basis, B);
}

int lolhip_gadget_correct_batch(const lolhip_plan* p, void* stream, const int64_t* xs, int64_t base, int basis,
                                int64_t* u_dec, int64_t* es_dec, int64_t* work, int64_t B) {
  CorrectParams c;
  int rc = correct_status(p, base, basis, B, c); if (rc) return rc;
  rc = need_device(p); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  const Plan& P = p->P;
  if (!xs || !u_dec || (basis != LOLHIP_BASIS_DEC && !work)) return LOLHIP_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const int64_t polys = (int64_t)c.d.L * B;
  if (basis != LOLHIP_BASIS_DEC) {
    Work w(work);
    int64_t* copy = correct_work(w, P, c.d.L, basis, B);
    if (basis == LOLHIP_BASIS_CRT) {
      if (hipMemcpyAsync(copy, xs, sizeof(int64_t) * (size_t)(polys * P.n * P.T), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return LOLHIP_ERR_HIP;
      rc = do_crt(P, s, copy, polys, true); if (rc) return rc;
      rc = run_prog_or_copy(P, P.prog_linv, s, copy, polys); if (rc) return rc;
    } else {
      rc = run_prog_or_copy(P, P.prog_linv, s, copy, polys, xs); if (rc) return rc;
    }
    xs = copy;
  }
  return hip_status(launch_gadget_correct(s, xs, u_dec, es_dec, B * P.n, c, P.d_mod));
}

int lolhip_gadget_encode_batch(const lolhip_plan* p, void* stream, const int64_t* sv, int64_t base, const int64_t* e,
                               int64_t* out, int64_t B) {
  if (!p) return LOLHIP_ERR_INVALID;
  DecompParams d;
  int rc = make_decomp(p->P, base, d); if (rc) return rc;
  if (B < 0) return LOLHIP_ERR_INVALID;
  rc = need_device(p); if (rc) return rc;
  if (B == 0) return LOLHIP_OK;
  if (!sv || !out) return LOLHIP_ERR_INVALID;
  return hip_status(launch_gadget_encode((hipStream_t)stream, sv, e, out, B * p->P.n, d, p->P.d_mod));
}

}  // extern "C"
