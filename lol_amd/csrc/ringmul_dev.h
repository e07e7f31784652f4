// lol_amd/csrc/ringmul_dev.h — the per-word arithmetic of the exact ring product's way in and way out,
// shared by the passes of ringmul.hip and the fused passes of rlwe_ring.hip: one definition, the same bits.
// Included by .hip files only.
#pragma once
#include "elementwise_dev.h"
#include "ringmul.h"

namespace lolhip {

constexpr int RING_TPB = 256;
constexpr i64 RING_MAX_BLOCKS = 1 << 16;      // grid-stride above, in both grid dimensions

// W coefficients per thread: `per` threads cover a row, grid.x strides over them, grid.y over the rows
struct RingShape { dim3 grid, block; };
inline RingShape ring_shape_for(i64 rows, i64 per) {
  unsigned threads = 64;
  while (threads < (unsigned)RING_TPB && (i64)threads < per) threads <<= 1;
  i64 gx = (per + threads - 1) / threads;
  gx = gx < 1 ? 1 : (gx < RING_MAX_BLOCKS ? gx : RING_MAX_BLOCKS);
  i64 gy = RING_MAX_BLOCKS / gx;
  gy = gy < 1 ? 1 : (gy < rows ? gy : rows);
  if (gy > 65535) gy = 65535;
  return RingShape{dim3((unsigned)gx, (unsigned)gy), dim3(threads)};
}

// a residue r in [0, q) -> the K residues in [0, Q_k) of its centred lift
template <int K>
__device__ __forceinline__ void lift_residue(u64 r, u64 q, const RingMul& c, u64* y) {
  const i64 v = centred(r, q);
#pragma unroll
  for (int k = 0; k < K; ++k) y[k] = c.wide ? mod_any(v, c.Q[k]) : canon_in(v, c.Q[k].q);
}

// any int64 x taken mod q (mc) -> the K residues of its centred lift
template <int K, bool POW2>
__device__ __forceinline__ void lift_word(i64 x, const ModCtx& mc, const RingMul& c, u64* y) {
  lift_residue<K>(POW2 ? (u64)x & (mc.q - 1) : mod_any(x, mc), mc.q, c, y);
}

// K residues of an integer X, |X| < prod Q / 2 -> X mod q_t in [0, q_t): mixed-radix digits, the sign from a most-
// significant-first comparison, the digits' sum reduced mod q_t.  No wide integers.
template <int K, bool POW2>
__device__ __forceinline__ u64 fold_word(const u64* xs, const ModCtx& mc, int t, const RingMul& c) {
  u64 x[K], v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = canon_in((i64)xs[k], c.Q[k].q);
  garner_digits<K>(v, [&](int k) { return x[k]; }, c.Q, c.pinv, c.qmod, RING_MAX_K);
  const bool neg = above_half<K>(v, c.half);
  if constexpr (POW2) {
    u64 acc = v[0];                            // mod 2^64, of which q_t is a divisor
#pragma unroll
    for (int k = 1; k < K; ++k) acc += v[k] * c.pw[t][k];
    if (neg) acc -= c.Qp[t];
    return acc & (mc.q - 1);
  } else {
    u64 r;
    if constexpr (K == 1) {
      r = rem128(0, v[0], mc);
    } else {
      unsigned __int128 acc = v[0];            // K terms below 2^124 each
#pragma unroll
      for (int k = 1; k < K; ++k) acc += (unsigned __int128)v[k] * c.pw[t][k];
      r = reduce128((u64)(acc >> 64), (u64)acc, mc);
    }
    return neg ? submod(r, c.Qp[t], mc.q) : r;
  }
}

}  // namespace lolhip
