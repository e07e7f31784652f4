// lol_amd/csrc/challenge.h — launcher interface of challenge.hip: the passes of a whole rlwe-challenges challenge
// (Generate.hs:105-218, Verify.hs:236-366) that the single-secret units do not provide.  A batch is I instances of L
// samples; item b = i L + l uses secret row i = b / L.  Used by challenge_api.cpp only.
#pragma once
#include <hip/hip_runtime_api.h>

#include "zq_dev.h"

namespace lolhip {

struct ChaChaKey;

constexpr i64 CHALL_MAX_ITEMS = 0x7fffffff;   // I L: the item index and b / L stay 32-bit scalars

// a [I L][n][T] uniform residues of `domain` at items ctr + b (CRT basis, the stream of launch_rlwe_uniform), and with
// them against the secrets s_crt [I][n][T]
//   RLWE_U_PROD  out = a s_i
//   RLWE_U_ADD   out = out + a s_i   (out holds reduce e in the CRT basis)
// The secrets themselves (RLWE_U_ONLY) are I items of launch_rlwe_uniform: that mode reads no secret.
hipError_t launch_chall_uniform(hipStream_t s, int mode, i64* a, const i64* s_crt, i64* out, i64 I, i64 L, i64 n, int T,
                                const ModCtx* mod, const ChaChaKey& key, u64 ctr, int domain);

// out = a s_i (b null) or b - a s_i over [I L][n][T] with s_crt [I][n][T] (CRT basis).  out may alias a or b.
hipError_t launch_chall_as(hipStream_t s, const i64* a, const i64* b, const i64* s_crt, i64* out, i64 I, i64 L, i64 n,
                           int T, const ModCtx* mod);

// the verdict of Verify.hs:346-366 per instance, one segmented reduction over the L values of instance i:
//   i64     norm [I L] (launch_gsqnorm_i64): fails = #{not (bound > norm)}, worst = max norm; INT64_MAX never passes
//   f64     norm [I L] (launch_gsqnorm_f64): the same in doubles; a NaN fails and makes worst NaN
//   rlwr    mismatch [I L] int32 (launch_rlwr_check): fails = #{mismatch != 0}, worst = max mismatch (int64)
hipError_t launch_chall_verdict_i64(hipStream_t s, const i64* norm, i64 bound, int32_t* fails, i64* worst, i64 I, i64 L);
hipError_t launch_chall_verdict_f64(hipStream_t s, const double* norm, double bound, int32_t* fails, double* worst, i64 I,
                                    i64 L);
hipError_t launch_chall_verdict_rlwr(hipStream_t s, const int32_t* mismatch, int32_t* fails, i64* worst, i64 I, i64 L);

}  // namespace lolhip
