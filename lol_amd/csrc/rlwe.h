// lol_amd/csrc/rlwe.h — launcher interface of rlwe.hip: gSqNormDec (the last Tensor member, Tensor.hs:147-151) and
// the element-wise passes of RLWE / RLWR sampling and instance verification (lol RLWE/{Continuous,Discrete,RLWR}.hs;
// rlwe-challenges Generate.hs / Verify.hs).  Used by rlwe_api.cpp only.
#pragma once
#include <hip/hip_runtime_api.h>

#include "zq_dev.h"

namespace lolhip {

struct ChaChaKey;

constexpr i64 NORM_MAX_N = 16384;     // one sample is LDS-resident (rlwe.hip k_gsqnorm)
constexpr int NORM_MAX_PRIMES = 8;    // odd primes of an index with n <= 16384: at most 5

// the odd primes' dimensions of the decoding basis, first prime power fastest-varying (tensor.h:40-80): prime i owns
// the coordinate (j / rts[i]) mod d[i], d = p - 1
struct NormDims {
  int k;                              // odd primes
  int d[NORM_MAX_PRIMES];
  int rts[NORM_MAX_PRIMES];
};

// out[b] = <e_b, (⊗ I_{p^(e-1)} ⊗ (I+J)_{p-1}) e_b> over B samples e [B][n], n <= NORM_MAX_N.  int64: exact, or
// INT64_MAX when the value exceeds it or a coefficient is INT64_MIN; double: a fixed summation order per n.
hipError_t launch_gsqnorm_i64(hipStream_t s, const i64* e, i64* out, i64 B, i64 n, const NormDims& nd);
hipError_t launch_gsqnorm_f64(hipStream_t s, const double* e, double* out, i64 B, i64 n, const NormDims& nd);

// a [B][n][T] uniform residues of `domain` at items ctr + b (CRT basis), and with them
//   RLWE_U_ONLY  nothing else (the secret: B = 1)
//   RLWE_U_PROD  out = a s
//   RLWE_U_ADD   out = out + a s   (out holds reduce e in the CRT basis)
enum { RLWE_U_ONLY = 0, RLWE_U_PROD = 1, RLWE_U_ADD = 2 };
hipError_t launch_rlwe_uniform(hipStream_t s, int mode, i64* a, const i64* s_crt, i64* out, i64 B, i64 n, int T,
                               const ModCtx* mod, const ChaChaKey& key, u64 ctr, int domain);

// out = a s (b null) or b - a s, one pointwise pass over [B][n][T] with s [n][T] broadcast (CRT basis)
hipError_t launch_rlwe_as(hipStream_t s, const i64* a, const i64* b, const i64* s_crt, i64* out, i64 B, i64 n, int T,
                          const ModCtx* mod);

// K/(qR) arithmetic of RRq.hs:47-84 in IEEE doubles, x [total] int64 residues in [0, q):
//   sample:  b = xd + reduce' g, one conditional subtraction             (Continuous.hs:45-54)
//   error:   e = lift (b + reduce' (-xd)), one conditional subtraction   (Continuous.hs:57-68)
hipError_t launch_rlwe_cont_sample(hipStream_t s, const i64* x, const double* g, double* b, i64 total, double q);
hipError_t launch_rlwe_cont_error(hipStream_t s, const i64* x, const double* b, double* e, i64 total, double q);

// RLWR (RLWR.hs:34-44): per residue x in [0, q), l = 2x < q ? x : x - q, r = floor((p l + floor(q/2)) / q) mod p.
// out [B][n] = r (given null), or mismatch [B] = the coefficients of sample b where r differs from given.
hipError_t launch_rlwr_round(hipStream_t s, const i64* x, i64* out, i64 total, u64 q, u64 p);
hipError_t launch_rlwr_check(hipStream_t s, const i64* x, const i64* given, int32_t* mismatch, i64 B, i64 n, u64 q, u64 p);

}  // namespace lolhip
