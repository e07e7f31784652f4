// lol_amd/csrc/elementwise_dev.h — the building blocks the element-wise passes share (pipeline.hip, decrypt.hip,
// encrypt.hip, kshint.hip, khprf.hip, public.hip, modswitch.hip): the tile count of a launch, the
// 16-byte store type and two scalar reductions.  Included by .hip files only.  A new pass adds here rather than copying.
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

}  // namespace lolhip
