// lol_amd/csrc/public.h — launcher interface of public.hip: the SymmSHE public operations and ciphertext addition
// (lol-apps SymmSHE.hs:214-230, 381-436).  Slabs are [.][B][n][T] int64, component t innermost.
#pragma once
#include <hip/hip_runtime_api.h>

#include "pipeline.h"

namespace lolhip {

// per-modulus Shoup pairs (w, floor(w 2^64 / q_t)) of two scalars, w < q_t
struct PubScales {
  int T;
  u64 q[PIPE_MAX_T];
  u64 a[PIPE_MAX_T], ap[PIPE_MAX_T];
  u64 b[PIPE_MAX_T], bp[PIPE_MAX_T];
};

// out_i = a_t a_i + b_t b_i for i < max(na, nb); a missing (i >= na) or b missing (i >= nb, b null) term is zero.
// Components are `slab` words apart; out may alias a or b.
hipError_t launch_ct_lincomb(hipStream_t s, const i64* a, int na, const i64* b, int nb, i64* out, i64 slab,
                             const PubScales& sc);

// out [items][n][T] = decode'(x * mul mod p) reduced mod q_t, x = in[item * stride + j] (any int64, taken mod p).
// mod: the T target moduli (the p plan's own context gives x * mul mod p).
hipError_t launch_pub_lift(hipStream_t s, const i64* in, i64 stride, i64 items, i64 n, i64* out, int T,
                           const ModCtx* mod, const ModCtx& mp, u64 mul);

enum { PUB_MUL = 0, PUB_ADD = 1 };
// out_i[b][j][t], i < ncs, b < B, j < n' (per = n' T):
//   PUB_MUL  a[b_a][e(j)][t] * c_i[b_c][j][t]
//   PUB_ADD  a_t c_i[b_c][j][t] (+ a[b_a][e(j)][t] for i = 0), a_t the Shoup pair sc.a / sc.ap
// e = idx (-1: zero) or the identity (idx null); b_a = 0 when a_item = 0, b_c = 0 when c is shared.  out may alias c
// unless c is shared and B > 1.
hipError_t launch_pub_apply(hipStream_t s, int mode, const i64* a, i64 a_item, const int32_t* idx, const i64* c,
                            bool c_shared, i64* out, int ncs, i64 B, i64 n, const PubScales& sc, const ModCtx* mod);

}  // namespace lolhip
