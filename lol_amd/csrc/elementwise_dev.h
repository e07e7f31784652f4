// lol_amd/csrc/elementwise_dev.h — the building blocks the element-wise passes share (pipeline.hip, decrypt.hip,
// encrypt.hip, kshint.hip, khprf.hip, public.hip, modswitch.hip, ptround.hip, pttunnel.hip, ringmul.hip, gadget.hip,
// ctmul.hip and the element-wise launches of kernels.hip).  Host side of a launch: the tile count (tiles_for), the capped
// block count of a grid-stride launch (grid_stride_blocks) and the 16-byte alignment test of the two-words-per-lane
// variants (aligned16).  Device side: the 16-byte store type, two scalar reductions (trim, mod_any), the floor division
// by an invariant divisor (floor_div_inv), the centred lift (centred), the mixed-radix digits of an RNS value
// (garner_digits) and their sign test (above_half).
// Included by .hip files only.  A new pass adds here rather than copying.
#pragma once
#include "zq_dev.h"

namespace lolhip {

// blocks = the `tile`-element tiles that cover `total` elements (at least one); false above 0x7fffffff blocks
inline bool tiles_for(i64 total, i64 tile, unsigned* blocks) {
  const i64 b = (total + tile - 1) / tile;
  if (b > 0x7fffffff) return false;
  *blocks = (unsigned)(b < 1 ? 1 : b);
  return true;
}

// blocks of a grid-stride launch of `tpb` threads over `total` elements: ceil(total / tpb), at least 1, at most `cap`
inline unsigned grid_stride_blocks(i64 total, i64 tpb, i64 cap) {
  const i64 b = (total + tpb - 1) / tpb;
  return (unsigned)(b < 1 ? 1 : (b < cap ? b : cap));
}

// every pointer 16-byte aligned (null counts as aligned): what a two-words-per-lane variant needs of its slabs
template <typename... P>
inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// two words as one 16-byte global store
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// [0, 2q) -> [0, q)
__device__ __forceinline__ u64 trim(u64 r, u64 q) { return r >= q ? r - q : r; }

// x mod q of any int64 (INT64_MIN included)
__device__ __forceinline__ u64 mod_any(i64 x, const ModCtx& mc) {
  const u64 a = x >= 0 ? (u64)x : 0 - (u64)x;
  const u64 r = rem128(0, a, mc);
  return (x < 0 && r != 0) ? mc.q - r : r;
}

// floor(x / d) for any signed x through the invariant-divisor multiply: magic = floor(2^64 (2^l - d) / d) + 1,
// l = ceil(log2 d), sh1 = min(l, 1), sh2 = max(l - 1, 0) (she_host.h inv_div), d >= 1
__device__ __forceinline__ i64 floor_div_inv(i64 x, u64 magic, int sh1, int sh2) {
  const u64 n = x >= 0 ? (u64)x : (u64)(-x - 1);
  const u64 t1 = __umul64hi(magic, n);
  const u64 q = (t1 + ((n - t1) >> sh1)) >> sh2;
  return x >= 0 ? (i64)q : -(i64)q - 1;
}

// the centred lift of a residue r in [0, q): r when 2 r < q, else r - q; at most floor(q / 2) in absolute value
__device__ __forceinline__ i64 centred(u64 r, u64 q) { return 2 * r < q ? (i64)r : (i64)r - (i64)q; }

// Mixed-radix (Garner) digits of the X in [0, prod q_i) with X = x(i) mod q_i, x(i) in [0, q_i): X = sum_i v[i] P_i,
// P_i = q_0 ... q_(i-1).  pinv[i] = P_i^-1 mod q_i, qmod[i * stride + j] = q_j mod q_i (plan.h lift_consts).  x is a
// callable, called once per component in ascending order, each right before its digit: k_lift loads and prepares its
// residue there (with all 16 residues prepared up front its decrypt measured 3 to 4 % slower on the MI355X).
template <int NT, typename X>
__device__ __forceinline__ void garner_digits(u64 (&v)[NT], X x, const ModCtx* mod, const u64* pinv, const u64* qmod,
                                              int stride) {
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const ModCtx mc = mod[i];
    const u64 xi = x(i);
    u64 s = 0;                                // sum_{j<i} v_j P_j mod q_i, Horner from the top digit
#pragma unroll
    for (int j = i - 1; j >= 0; --j) {
      const u128 t = (u128)s * qmod[i * stride + j] + v[j];   // < q_i^2 + 2^62 < q_i 2^64
      s = rem128((u64)(t >> 64), (u64)t, mc);
    }
    v[i] = i == 0 ? xi : mulmod(submod(xi, s, mc.q), pinv[i], mc);
  }
}

// X > floor((Q - 1) / 2), i.e. X is negative as a centred value: most significant digit first against the digits
// half[] of floor((Q - 1) / 2)
template <int NT>
__device__ __forceinline__ bool above_half(const u64 (&v)[NT], const u64* half) {
  bool neg = false, decided = false;
#pragma unroll
  for (int i = NT - 1; i >= 0; --i) {
    const u64 h = half[i];
    if (!decided && v[i] != h) { neg = v[i] > h; decided = true; }
  }
  return neg;
}

}  // namespace lolhip
