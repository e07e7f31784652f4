// lol_amd/csrc/public.hip — the SymmSHE public operations and ciphertext addition (lol-apps SymmSHE.hs:214-230,
// 381-436).  gfx950 only; three HBM-bound element-wise passes over [.][B][n][T] int64 slabs (component t innermost).
//
//   k_ct_lincomb  out_i = alpha_t a_i + beta_t b_i: toMSD / toLSD, mulScalar, negate, subtraction and the
//                 componentwise part of (+) (SymmSHE.hs:214-230, 392-399, 420-436)
//   k_pub_lift    public values of R_m (any int64) -> decode'(x * mul mod p) reduced into T moduli (ZqBasic.hs:92-94)
//   k_pub_apply   out_i = a(e(j)) * c_i (mulPublic, :405-411) or scale * c_i (+ a(e(j)) for i = 0) (addPublic, :381-390):
//                 the embedding m -> m' is the gather e of the ext's tables, folded into the pass
//
// Tiling follows k_ctmul (pipeline.hip): a workgroup owns one tile of consecutive words, divides its start once in
// 64 bits and walks its words in 32 bits.  V2: two words per lane, 16-byte loads and plain 16-byte global stores.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "public.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;
constexpr int EPT = 2;                       // accesses per thread

__device__ __forceinline__ u64 scale_mod(u64 x, u64 w, u64 wp, u64 q) { return trim(shoup_lazy(x, w, wp, q), q); }
}  // namespace

// ---------------------------------------------------------------------------------------
// linear combination of two ciphertexts' components
// ---------------------------------------------------------------------------------------
template <bool V2, bool HAS_B>
__global__ void __launch_bounds__(TPB)
k_ct_lincomb(const i64* a, int na, const i64* b, int nb, i64* out, i64 total, i64 slab, PubScales sc) {
  constexpr int W = V2 ? 2 : 1;
  constexpr i64 TILE = (i64)TPB * EPT * W;
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
  const i64 i_s = s0 / slab;
  const i64 r_s = s0 - i_s * slab;
  const u32 t_s = (u32)((u64)s0 % (u64)sc.T);
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const u32 l = ((u32)e * TPB + threadIdx.x) * W;
    const i64 g = s0 + l;
    if (g >= total) continue;
    i64 r = r_s + l, i = i_s;
    while (r >= slab) { r -= slab; ++i; }                     // a tile may run into the next component
    const bool ha = i < na, hb = HAS_B && i < nb;
    u64 x[W], y[W];
#pragma unroll
    for (int k = 0; k < W; ++k) x[k] = y[k] = 0;
    if constexpr (V2) {
      if (ha) { const longlong2 v = *reinterpret_cast<const longlong2*>(a + g); x[0] = (u64)v.x; x[1] = (u64)v.y; }
      if (hb) { const longlong2 v = *reinterpret_cast<const longlong2*>(b + g); y[0] = (u64)v.x; y[1] = (u64)v.y; }
    } else {
      if (ha) x[0] = (u64)a[g];
      if (hb) y[0] = (u64)b[g];
    }
    u64 o[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      u32 t = t_s + l + (u32)k;
      t %= (u32)sc.T;
      const u64 q = sc.q[t];
      const u64 xa = ha ? scale_mod(canon_in((i64)x[k], q), sc.a[t], sc.ap[t], q) : 0;
      const u64 yb = hb ? scale_mod(canon_in((i64)y[k], q), sc.b[t], sc.bp[t], q) : 0;
      o[k] = addmod(xa, yb, q);
    }
    // every input word is read before the store: out may alias a or b
    if constexpr (V2) {
      u64x2 v; v.x = o[0]; v.y = o[1];
      *reinterpret_cast<u64x2*>(out + g) = v;
    } else {
      out[g] = (i64)o[0];
    }
  }
}

hipError_t launch_ct_lincomb(hipStream_t s, const i64* a, int na, const i64* b, int nb, i64* out, i64 slab,
                             const PubScales& sc) {
  const int nc = na > nb ? na : nb;
  const i64 total = (i64)nc * slab;
  if (total == 0) return hipSuccess;
  if (sc.T < 1 || sc.T > PIPE_MAX_T || slab % sc.T) return hipErrorInvalidValue;
  const bool v2 = (slab & 1) == 0 && aligned16(a, b, out);
  unsigned blocks;
  if (!tiles_for(total, (i64)TPB * EPT * (v2 ? 2 : 1), &blocks)) return hipErrorInvalidValue;
  const bool hb = b && nb > 0;
#define LOLHIP_LC(VV, BB) \
  hipLaunchKernelGGL((k_ct_lincomb<VV, BB>), dim3(blocks), dim3(TPB), 0, s, a, na, b, hb ? nb : 0, out, total, slab, sc)
  if (v2) { if (hb) LOLHIP_LC(true, true); else LOLHIP_LC(true, false); }
  else { if (hb) LOLHIP_LC(false, true); else LOLHIP_LC(false, false); }
#undef LOLHIP_LC
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// public values -> decode' -> T moduli; one thread per coefficient, T words out
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_pub_lift(const i64* __restrict__ in, i64 stride, i64 n, i64* __restrict__ out, i64 rows, int T,
           const ModCtx* __restrict__ mod, ModCtx mp, u64 mul) {
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < rows; g += (i64)gridDim.x * TPB) {
    const i64 item = g / n, j = g - item * n;
    const u64 x = mulmod(mod_any(in[item * stride + j], mp), mul, mp);
    const bool neg = 2 * x >= mp.q;                           // decode': v - p for v >= p/2 (p/2 itself included)
    const u64 mag = neg ? mp.q - x : x;
    for (int t = 0; t < T; ++t) {
      const ModCtx& mc = mod[t];
      const u64 r = mag < mc.q ? mag : rem128(0, mag, mc);
      out[g * T + t] = (i64)((neg && r != 0) ? mc.q - r : r);
    }
  }
}

hipError_t launch_pub_lift(hipStream_t s, const i64* in, i64 stride, i64 items, i64 n, i64* out, int T,
                           const ModCtx* mod, const ModCtx& mp, u64 mul) {
  const i64 rows = items * n;
  if (rows == 0) return hipSuccess;
  if (T < 1 || mul >= mp.q) return hipErrorInvalidValue;
  const unsigned grid = grid_stride_blocks(rows, TPB, 1 << 20);
  hipLaunchKernelGGL(k_pub_lift, dim3(grid), dim3(TPB), 0, s, in, stride, n, out, rows, T, mod, mp, mul);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// mulPublic / addPublic with the embedding folded in
// ---------------------------------------------------------------------------------------
template <int MODE, bool V2>
__global__ void __launch_bounds__(TPB)
k_pub_apply(const i64* __restrict__ a, i64 a_item, const int32_t* __restrict__ idx, const i64* c, i64 c_item,
            i64 c_comp, i64* out, i64 B, i64 total, u32 per, PubScales sc, const ModCtx* __restrict__ mod) {
  constexpr int W = V2 ? 2 : 1;
  constexpr i64 TILE = (i64)TPB * EPT * W;
  const int T = sc.T;
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
  const i64 row_s = s0 / per;                                 // (component, item) of the tile's first word
  const u32 r_s = (u32)(s0 - row_s * per);
  const i64 i_s = row_s / B, b_s = row_s - i_s * B;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const u32 l = ((u32)e * TPB + threadIdx.x) * W;
    const i64 g = s0 + l;
    if (g >= total) continue;
    u32 r = r_s + l;
    i64 b = b_s, i = i_s;
    while (r >= per) {                                        // a tile may run into the next item or component
      r -= per;
      if (++b == B) { b = 0; ++i; }
    }
    const i64* cp = c + i * c_comp + b * c_item + r;
    const i64* ap = a + b * a_item;
    u64 x[W];
    if constexpr (V2) {
      const longlong2 v = *reinterpret_cast<const longlong2*>(cp);
      x[0] = (u64)v.x; x[1] = (u64)v.y;
    } else {
      x[0] = (u64)cp[0];
    }
    u64 o[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const u32 rk = r + (u32)k;
      const u32 j = rk / (u32)T, t = rk - j * (u32)T;
      const u64 q = sc.q[t];
      const i64 src = (MODE == PUB_MUL || i == 0) ? (idx ? (i64)idx[j] : (i64)j) : -1;   // a joins c_0 only
      const u64 av = src >= 0 ? canon_in(ap[src * T + t], q) : 0;
      const u64 cv = canon_in((i64)x[k], q);
      if constexpr (MODE == PUB_MUL) {
        o[k] = mulmod(av, cv, mod[t]);
      } else {
        const u64 sv = scale_mod(cv, sc.a[t], sc.ap[t], q);
        o[k] = i == 0 ? addmod(sv, av, q) : sv;
      }
    }
    if constexpr (V2) {
      u64x2 v; v.x = o[0]; v.y = o[1];
      *reinterpret_cast<u64x2*>(out + g) = v;
    } else {
      out[g] = (i64)o[0];
    }
  }
}

hipError_t launch_pub_apply(hipStream_t s, int mode, const i64* a, i64 a_item, const int32_t* idx, const i64* c,
                            bool c_shared, i64* out, int ncs, i64 B, i64 n, const PubScales& sc, const ModCtx* mod) {
  const int T = sc.T;
  const i64 per = n * T, total = (i64)ncs * B * per;
  if (total == 0) return hipSuccess;
  if (T < 1 || T > PIPE_MAX_T || per > 0x7fffffff || (mode != PUB_MUL && mode != PUB_ADD)) return hipErrorInvalidValue;
  const i64 c_item = c_shared ? 0 : per, c_comp = c_shared ? per : B * per;
  const bool v2 = (per & 1) == 0 && aligned16(c, out);
  unsigned blocks;
  if (!tiles_for(total, (i64)TPB * EPT * (v2 ? 2 : 1), &blocks)) return hipErrorInvalidValue;
#define LOLHIP_PA(MM, VV)                                                                                       \
  hipLaunchKernelGGL((k_pub_apply<MM, VV>), dim3(blocks), dim3(TPB), 0, s, a, a_item, idx, c, c_item, c_comp, out, B, \
                     total, (u32)per, sc, mod)
  if (mode == PUB_MUL) { if (v2) LOLHIP_PA(PUB_MUL, true); else LOLHIP_PA(PUB_MUL, false); }
  else { if (v2) LOLHIP_PA(PUB_ADD, true); else LOLHIP_PA(PUB_ADD, false); }
#undef LOLHIP_PA
  return hipGetLastError();
}

}  // namespace lolhip
