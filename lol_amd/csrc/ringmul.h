// lol_amd/csrc/ringmul.h — the two passes of the exact ring product over moduli without a CRT basis (ringmul.hip), as
// ringmul_api.cpp launches them.
#pragma once
#include <hip/hip_runtime_api.h>

#include "zq_dev.h"

namespace lolhip {

constexpr int RING_MAX_T = 16;     // moduli q_t of the ring the product lives in
constexpr int RING_MAX_K = 3;      // NTT primes Q_i the integer product is computed over

// Everything both passes need, by value in the launch (as Relift is, pttunnel.h).
struct RingMul {
  int T, K;
  int pow2;                             // every q_t is a power of two: reductions mod q_t are masks
  int wide;                             // some Q_i <= max_t floor(q_t / 2): a lift can exceed Q_i, full reductions
  ModCtx q[RING_MAX_T];
  u64 pw[RING_MAX_T][RING_MAX_K];       // P_i mod q_t, P_i = Q_0 ... Q_(i-1)
  u64 Qp[RING_MAX_T];                   // Q_0 ... Q_(K-1) mod q_t
  ModCtx Q[RING_MAX_K];
  u64 pinv[RING_MAX_K];                 // P_i^-1 mod Q_i                            (the lift constants of the plan
  u64 qmod[RING_MAX_K * RING_MAX_K];    // Q_j mod Q_i at [i * RING_MAX_K + j]        over the Q_i, plan.h lift_consts)
  u64 half[RING_MAX_K];                 // mixed-radix digits of floor((prod Q - 1) / 2)
};

// k_ring_lift: in [rows][n][T], any int64 taken mod q_t -> out [rows * T][n][K]: polynomial r T + t holds component t
// of row r, coefficient j the K residues in [0, Q_i) of the centred lift.  in and out must not overlap.
hipError_t launch_ring_lift(hipStream_t s, const i64* in, i64* out, i64 rows, i64 n, const RingMul& c);
// k_ring_fold: in [rows * T][n][K] residues of integers X with |X| < prod Q / 2 -> out [rows][n][T]: X mod q_t in
// [0, q_t).  in and out must not overlap.
hipError_t launch_ring_fold(hipStream_t s, const i64* in, i64* out, i64 rows, i64 n, const RingMul& c);

}  // namespace lolhip

// the handle behind include/lolhip.h's lolhip_ringmul (ringmul_api.cpp makes it; rlwe_ring_api.cpp reads it)
struct lolhip_plan;
struct lolhip_ringmul {
  const lolhip_plan* pQ = nullptr;   // the transforms run on it; pq's moduli live on in rm
  lolhip::RingMul rm{};
  bool device = false;
};
