// lol_amd/csrc/ctmul.h — launcher interface of ctmul.hip: the SymmSHE ciphertext product (*) of any degree (lol-apps
// SymmSHE.hs:438-452).  Slabs are [.][B][n'][T] int64, component t innermost, CRT basis.
#pragma once
#include <hip/hip_runtime_api.h>

#include "lolhip.h"               // LOLHIP_CT_MUL_MAX: components of either operand
#include "pipeline.h"

#define LOLHIP_CT_MUL_LAZY 4     // raw products (each < q^2) one 128-bit accumulator takes between reductions (ctmul.hip)

namespace lolhip {

// per-modulus Shoup pairs (w, floor(w 2^64 / q_t)) of the product's scalar alpha, w < q_t
struct CtMulScale {
  int T;
  u64 a[PIPE_MAX_T], ap[PIPE_MAX_T];
};

// out_k = alpha_t g (sum_{i + j = k} a_i b_j) mod q_t for k < na + nb - 1, g = gcrt [n'][T]; a [na][B][n'][T],
// b [nb][B][n'][T], out [na + nb - 1][B][n'][T], 1 <= na, nb <= LOLHIP_CT_MUL_MAX.  b == a with nb == na squares: every
// input word is read once.  Inputs in (-q_t, q_t), outputs canonical.  out must not overlap a or b.
hipError_t launch_ct_mul(hipStream_t s, const i64* a, int na, const i64* b, int nb, i64* out, i64 B, i64 n,
                         const CtMulScale& sc, const i64* gcrt, const ModCtx* mod);

}  // namespace lolhip
