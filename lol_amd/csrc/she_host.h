// lol_amd/csrc/she_host.h — what the host translation units of the C ABI share: the handle types behind
// include/lolhip.h, the launch helpers capi.cpp owns (defined there) and the one definition of every small piece of
// SymmSHE host arithmetic, glue and shared work-buffer layout the *_api.cpp files need.  Pure host
// C++; not part of the public interface.  A new feature adds here rather than copying.
#pragma once
#include <hip/hip_runtime_api.h>

#include "hostmath.h"
#include "lolhip.h"
#include "pipeline.h"
#include "plan.h"
#include "public.h"
#include "rlwe.h"
#include "work.h"

struct lolhip_plan { lolhip::Plan P; };
struct lolhip_ext { lolhip::ExtPlan X; };

namespace lolhip {

// ---- defined in capi.cpp -----------------------------------------------------------------------------------------
// LOLHIP_OK, or why the plan cannot compute on the calling thread's current device
int need_device(const lolhip_plan* p);
int need_device(const Plan& P);
// y = program(src or y) over B polynomials (the vector interpreter or the scalar one)
int run_prog(const Plan& P, const StageProgram& sp, hipStream_t s, int64_t* y, int64_t B, const int64_t* src = nullptr);
// crt / crtInv of B polynomials in place, through whichever path the plan has
int do_crt(const Plan& P, hipStream_t s, int64_t* y, int64_t B, bool inverse);
// 1 when divG is possible modulo every q_t of the plan
int divg_ok(const Plan& P);
// digit counts (gadlen, ZqBasic.hs:238-240) and the invariant-divisor constants of `base` over the plan's moduli
int make_decomp(const Plan& P, int64_t base, DecompParams& d);

// ---- defined in public_api.cpp --------------------------------------------------------------------------------------
// lifted [items][n_m][T] = linv g_m^k b over P's moduli at index m = lo, in the CRT basis when crt: the passes addPublic
// and ptRound's constants share.  pp: the plan of index m over p, pw [items][n_m]: its scratch (both for k > 0 only)
int public_lift(const Plan& P, const Plan& lo, const Plan* pp, hipStream_t s, const int64_t* b, int64_t stride, int64_t items,
                int64_t k, u64 linv, u64 p, bool crt, int64_t* pw, int64_t* lifted);

// ---- the work-buffer layouts more than one entry carves (work.h) -------------------------------------------------------
// evalLin over B elements: the coefficient vectors [rel][B][n_E][T] | their embeddings into S [rel][B][n_S][T]
struct EvalLinWork { int64_t *tmp_e, *tmp_s; };
inline EvalLinWork evallin_work(Work& w, const ExtPlan& ER, const ExtPlan& ES, int64_t B) {
  const int64_t rel = ER.host.phi2 / ER.host.phi, T = ER.lo->T;
  return {w.take(rel * B * ER.host.phi * T), w.take(rel * B * ES.host.phi2 * T)};
}
// the digit polynomials of one key switch: [L][B][n][T]
inline int64_t* ks_digits(Work& w, int64_t L, int64_t B, int64_t n, int64_t T) { return w.take(L * B * n * T); }
// one tunnel hop: evalLin's regions (used twice: c_0, then c_1's coefficient vectors) | its key switches' digits
struct TunnelWork { EvalLinWork ev; int64_t* dig; };
inline TunnelWork tunnel_work(Work& w, const ExtPlan& ER, const ExtPlan& ES, int64_t L, int64_t B) {
  return {evallin_work(w, ER, ES, B), ks_digits(w, L, B, ES.host.phi2, ER.lo->T)};
}
// one modSwitch out of plan F: [ncs][B][n][T(F)]
inline int64_t* modswitch_work(Work& w, const Plan& F, int ncs, int64_t B) { return w.take((int64_t)ncs * B * F.n * F.T); }

// ---- glue --------------------------------------------------------------------------------------------------------
inline int hip_status(hipError_t e) { return e == hipSuccess ? LOLHIP_OK : LOLHIP_ERR_HIP; }

// y = program(src or y), or a copy when the program is empty (L and L^-1 of m = 2^k: the powerful and decoding
// bases coincide)
inline int run_prog_or_copy(const Plan& P, const StageProgram& sp, hipStream_t s, int64_t* y, int64_t B,
                            const int64_t* src = nullptr) {
  if (!sp.stages.empty()) return run_prog(P, sp, s, y, B, src);
  if (!src || src == y || B == 0) return LOLHIP_OK;
  return hip_status(hipMemcpyAsync(y, src, sizeof(int64_t) * (size_t)(B * P.n * P.T), hipMemcpyDeviceToDevice, s));
}

// the same index with the same tensor order: m and every (p, e)
inline bool same_index(const Plan& a, const Plan& b) { return a.m == b.m && same_pps(a.pps, b.pps); }

// the odd primes' dimensions of the plan's index (rlwe.h NormDims)
inline NormDims norm_dims(const Plan& P) {
  NormDims nd = {};
  i64 rts = 1;
  for (const PP& pe : P.pps) {
    if (pe.p != 2 && nd.k < NORM_MAX_PRIMES) {
      nd.d[nd.k] = pe.p - 1;
      nd.rts[nd.k] = (int)rts;
      ++nd.k;
    }
    rts *= totient_pp(pe.p, pe.e);
  }
  return nd;
}

// x rounded up to an even count of words: work-buffer regions keep the 16-byte alignment of the buffer
inline int64_t even(int64_t x) { return (x + 1) & ~(int64_t)1; }

// the constants of floor division by the invariant divisor d >= 1 (elementwise_dev.h floor_div_inv):
// magic = floor(2^64 (2^l - d) / d) + 1, l = ceil(log2 d), sh1 = min(l, 1), sh2 = max(l - 1, 0)
inline void inv_div(u64 d, u64& magic, int& sh1, int& sh2) {
  int l = 0;
  while (((u128)1 << l) < (u128)d) ++l;
  magic = (u64)((((u128)1 << 64) * (((u128)1 << l) - (u128)d)) / (u128)d) + 1;
  sh1 = l < 1 ? l : 1;
  sh2 = l > 1 ? l - 1 : 0;
}

// floor(2^32 (2^l - base) / base) + 1, l = ceil(log2 base): the 32-bit invariant-divisor constant of the fused key
// switches (1 for TrivGad, base = 0)
inline uint32_t magic32(int64_t base) {
  if (base < 2) return 1;
  int lg = 0;
  while (((u64)1 << lg) < (u64)base) ++lg;
  return (uint32_t)((((u64)1 << 32) * (((u64)1 << lg) - (u64)base)) / (u64)base) + 1;
}

// the per-modulus Shoup pairs of two scalars over the plan's moduli (a null: 1, b null: 0), P.T <= PIPE_MAX_T
inline void set_scale(PubScales& sc, const Plan& P, const u64* a, const u64* b) {
  sc = PubScales();
  sc.T = P.T;
  for (int t = 0; t < P.T; ++t) {
    const u64 q = P.qs[(size_t)t];
    sc.q[t] = q;
    sc.a[t] = a ? a[t] : 1 % q;
    sc.ap[t] = make_shoup(sc.a[t], q).wp;
    sc.b[t] = b ? b[t] : 0;
    sc.bp[t] = make_shoup(sc.b[t], q).wp;
  }
}

// the plan of index m behind x_q (P itself for x_q = NULL); null when x_q does not end in P's ring and moduli
inline const Plan* lo_plan(const Plan& P, const lolhip_ext* x_q) {
  if (!x_q) return &P;
  const ExtPlan& X = x_q->X;
  if (!same_index(*X.hi, P) || X.hi->qs != P.qs) return nullptr;
  return X.lo;
}

// ---- arithmetic over the plaintext modulus -------------------------------------------------------------------------
// a plaintext modulus the SHE entries take: 2 <= p < 2^62
inline bool p_ok(int64_t p) { return p >= 2 && p < ((int64_t)1 << 62); }

// x mod q in [0, q) for any int64 x
inline u64 canon(int64_t x, u64 q) {
  const int64_t r = (int64_t)((__int128)x % (__int128)q);
  return r < 0 ? (u64)(r + (int64_t)q) : (u64)r;
}

// Q mod p, Q = prod q_t
inline u64 q_mod(const Plan& P, u64 p) {
  u64 r = 1 % p;
  for (u64 q : P.qs) r = mulmod(r, q % p, p);
  return r;
}

// the encoding factors of ZqBasic.hs:132-137 over the product ring (Prelude.hs:310-315), P.T <= PIPE_MAX_T:
//   lsdToMSD = (zp = -Q mod p, zq[t] = p^-1 mod q_t),   msdToLSD = (zp = (-Q)^-1 mod p, zq[t] = p mod q_t)
// LOLHIP_ERR_MODULUS for a p out of range or where an inverse is missing
inline int encode_scales(const Plan& P, int64_t p, bool to_msd, u64* zq, u64* zp) {
  if (!p_ok(p)) return LOLHIP_ERR_MODULUS;
  const u64 up = (u64)p;
  const u64 negq = (up - q_mod(P, up)) % up;
  for (int t = 0; t < P.T; ++t) {
    const u64 q = P.qs[(size_t)t];
    zq[t] = to_msd ? invmod(up % q, q) : up % q;
    if (to_msd && zq[t] == 0) return LOLHIP_ERR_MODULUS;
  }
  *zp = to_msd ? negq : invmod(negq, up);
  if (!to_msd && *zp == 0) return LOLHIP_ERR_MODULUS;
  return LOLHIP_OK;
}

// the ciphertext scalar after the conversion whose factor is zp: l' = l zp mod p (zp = 1: l mod p)
inline u64 encode_l(int64_t l, u64 zp, u64 p) { return mulmod(canon(l, p), zp, p); }

}  // namespace lolhip
