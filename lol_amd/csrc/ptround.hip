// lol_amd/csrc/ptround.hip — the ciphertext product of HomomPRF's ptRound (lol-apps HomomPRF.hs:232-270) with both
// affine pre-steps folded in.  gfx950 only; one HBM-bound element-wise pass over [.][B][n'][T] int64 slabs (component
// t innermost, CRT basis), no LDS.
//
//   k_ct_affine_mul  (alpha a + va) * (beta b + vb) for two linear ciphertexts, times gCRT: addPublic (SymmSHE.hs:381-390:
//                    the toLSD factor on every component, the public polynomial on c_0), the toMSD / toLSD factors of
//                    modSwitchPT and (*), and mulG <$> (c * d) (SymmSHE.hs:444-449) in one pass
//
// Tiling follows k_ctmul (pipeline.hip) and public.hip: a workgroup owns one tile of consecutive words of one pair,
// divides its start once in 64 bits and walks its words in 32 bits.  V2: two words per lane, 16-byte loads and plain
// 16-byte global stores.  blockIdx.y is the pair of the fan-out form.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "ptround.h"

namespace lolhip {

namespace {

constexpr int TPB = 256;
constexpr int EPT = 2;                       // accesses per thread

// alpha x (+ v): x, v in (-q, q) -> [0, q)
template <bool HAS_V>
__device__ __forceinline__ u64 affine(i64 x, u64 w, u64 wp, i64 v, u64 q) {
  const u64 s = trim(shoup_lazy(canon_in(x, q), w, wp, q), q);
  return HAS_V ? addmod(s, canon_in(v, q), q) : s;
}

template <int W>
__device__ __forceinline__ void load_words(const i64* p, u64* x) {
  if constexpr (W == 2) {
    const longlong2 v = *reinterpret_cast<const longlong2*>(p);
    x[0] = (u64)v.x; x[1] = (u64)v.y;
  } else {
    x[0] = (u64)p[0];
  }
}

template <int W>
__device__ __forceinline__ void store_words(i64* p, const u64* o) {
  if constexpr (W == 2) {
    u64x2 v; v.x = o[0]; v.y = o[1];
    *reinterpret_cast<u64x2*>(p) = v;
  } else {
    p[0] = (i64)o[0];
  }
}
}  // namespace

template <bool V2, bool HAS_VA, bool HAS_VB>
__global__ void __launch_bounds__(TPB)
k_ct_affine_mul(const i64* a, i64 a_pair, const i64* va, const i64* b, i64 b_pair, const i64* vb, i64* out,
                const i64* __restrict__ gcrt, i64 slab, u32 per, PubScales sc, const ModCtx* __restrict__ mod) {
  constexpr int W = V2 ? 2 : 1;
  constexpr i64 TILE = (i64)TPB * EPT * W;
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
  const u32 r_s = (u32)((u64)s0 % per);
  const i64 pair = (i64)blockIdx.y;
  const i64* ap = a + pair * a_pair;
  const i64* bp = b + pair * b_pair;
  const bool same = ap == bp;                                 // x * (beta x + v): the second operand is not read again
  const i64* vap = HAS_VA ? va + pair * per : nullptr;
  const i64* vbp = HAS_VB ? vb + pair * per : nullptr;
  i64* op = out + pair * 3 * slab;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const u32 l = ((u32)e * TPB + threadIdx.x) * W;
    const i64 g = s0 + l;
    if (g >= slab) continue;
    u32 r = r_s + l;
    if (r >= per) r %= per;                                   // V2: per is even, so r and r + 1 are one polynomial's
    u64 x0[W], x1[W], y0[W], y1[W], gv[W], pa[W], pb[W];
    load_words<W>(ap + g, x0);
    load_words<W>(ap + slab + g, x1);
    if (same) {
#pragma unroll
      for (int k = 0; k < W; ++k) { y0[k] = x0[k]; y1[k] = x1[k]; }
    } else {
      load_words<W>(bp + g, y0);
      load_words<W>(bp + slab + g, y1);
    }
    load_words<W>(gcrt + r, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) pa[k] = pb[k] = 0;
    if constexpr (HAS_VA) load_words<W>(vap + r, pa);
    if constexpr (HAS_VB) load_words<W>(vbp + r, pb);
    u32 t = r % (u32)sc.T;
    u64 o0[W], o1[W], o2[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const ModCtx mc = mod[t];
      const u64 q = mc.q;
      const u64 A0 = affine<HAS_VA>((i64)x0[k], sc.a[t], sc.ap[t], (i64)pa[k], q);
      const u64 A1 = affine<false>((i64)x1[k], sc.a[t], sc.ap[t], 0, q);
      const u64 B0 = affine<HAS_VB>((i64)y0[k], sc.b[t], sc.bp[t], (i64)pb[k], q);
      const u64 B1 = affine<false>((i64)y1[k], sc.b[t], sc.bp[t], 0, q);
      const u64 p0 = mulmod(A0, B0, mc);
      const u64 p2 = mulmod(A1, B1, mc);
      const u128 cross = (u128)A0 * B1 + (u128)A1 * B0;        // < 2 q^2 < q * 2^64
      const u64 p1 = rem128((u64)(cross >> 64), (u64)cross, mc);
      o0[k] = mulmod(gv[k], p0, mc);
      o1[k] = mulmod(gv[k], p1, mc);
      o2[k] = mulmod(gv[k], p2, mc);
      if (++t == (u32)sc.T) t = 0;
    }
    // every input word is read before the stores: out may alias a or b (one pair)
    store_words<W>(op + g, o0);
    store_words<W>(op + slab + g, o1);
    store_words<W>(op + 2 * slab + g, o2);
  }
}

hipError_t launch_ct_affine_mul(hipStream_t s, const i64* a, i64 a_pair, const i64* va, const i64* b, i64 b_pair,
                                const i64* vb, int npairs, i64* out, i64 B, i64 n, const PubScales& sc, const i64* gcrt,
                                const ModCtx* mod) {
  const int T = sc.T;
  const i64 per = n * T, slab = B * per;
  if (slab == 0 || npairs == 0) return hipSuccess;
  if (T < 1 || T > PIPE_MAX_T || per > 0x7fffffff || npairs < 0 || npairs > 65535 || a_pair < 0 || b_pair < 0)
    return hipErrorInvalidValue;
  const bool v2 = (per & 1) == 0 && ((a_pair | b_pair) & 1) == 0 && aligned16(a, b, va, vb, out, gcrt);
  unsigned blocks;
  if (!tiles_for(slab, (i64)TPB * EPT * (v2 ? 2 : 1), &blocks)) return hipErrorInvalidValue;
#define LOLHIP_AM(VV, AA, BB)                                                                                     \
  hipLaunchKernelGGL((k_ct_affine_mul<VV, AA, BB>), dim3(blocks, (unsigned)npairs), dim3(TPB), 0, s, a, a_pair, va, b, \
                     b_pair, vb, out, gcrt, slab, (u32)per, sc, mod)
#define LOLHIP_AM_V(VV)                                                       \
  do {                                                                        \
    if (va) { if (vb) LOLHIP_AM(VV, true, true); else LOLHIP_AM(VV, true, false); } \
    else { if (vb) LOLHIP_AM(VV, false, true); else LOLHIP_AM(VV, false, false); }  \
  } while (0)
  if (v2) LOLHIP_AM_V(true); else LOLHIP_AM_V(false);
#undef LOLHIP_AM_V
#undef LOLHIP_AM
  return hipGetLastError();
}

}  // namespace lolhip
