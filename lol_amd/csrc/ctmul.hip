// lol_amd/csrc/ctmul.hip — the SymmSHE ciphertext product (*) of any degree (lol-apps SymmSHE.hs:438-452).  gfx950 only;
// one element-wise pass over [.][B][n'][T] int64 slabs (component t innermost, CRT basis), no LDS.
//
//   k_ct_mul  out_k = alpha_t gCRT sum_{i + j = k} a_i b_j for a of na and b of nb components, k < na + nb - 1: the
//             polynomial product of c1 * c2, mulG <$> on every coefficient (:449) and the toLSD factor of the MSD x MSD
//             case (:444) in one pass.  b == a: the square, every input word read once, cross terms doubled
//
// Tiling follows k_ct_affine_mul (ptround.hip) and k_ct_lincomb (public.hip): a workgroup owns one tile of consecutive
// words of a slab, divides its start once in 64 bits and walks its words in 32 bits.  V2: two words per lane, 16-byte
// loads and plain 16-byte global stores.  Up to 3 x 3 components the counts are template arguments; beyond, one form
// over 8 x 8 register slots takes them at run time (DYN, one word per lane): its loops are unrolled over the slots, so
// that every register index is a constant, and a slot beyond na / nb is skipped by a wave-uniform branch.
#include <hip/hip_runtime.h>

#include <utility>

#include "ctmul.h"
#include "elementwise_dev.h"

namespace lolhip {

namespace {

constexpr int TPB = 256;
constexpr int EPT = 2;                       // accesses per thread
constexpr int STATIC_MAX = 3;                // component counts up to here are template arguments
constexpr int LAZY = LOLHIP_CT_MUL_LAZY;

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

__device__ __forceinline__ u64 rem(u128 v, const ModCtx& mc) { return rem128((u64)(v >> 64), (u64)v, mc); }

// The lazy accumulator of one output coefficient.  Every term it holds is below q^2: a raw product x y of x, y < q, or
// the residue (< q) a reduction leaves behind.  rem128 needs its argument below q 2^64, and
//     LAZY q^2 <= q 2^64   <=>   q <= 2^64 / LAZY = 2^62        (LAZY = 4; plans accept q < 2^62),
// so LAZY terms may be added before a reduction, and a fifth may not: 5 (q - 1)^2 > q 2^64 for q just below 2^62.  The
// accumulator is reduced when it holds LAZY terms and another one arrives; the residue counts as the first term of the
// next run.  pos: the term's slot in its sum, a constant once the loops are unrolled: the first LAZY slots need no test.
__device__ __forceinline__ void add_term(u128& acc, int& cnt, u64 x, u64 y, const ModCtx& mc, int pos) {
  if (pos >= LAZY && cnt == LAZY) { acc = rem(acc, mc); cnt = 1; }
  acc += (u128)x * y;
  ++cnt;
}

}  // namespace

template <bool V2, int NA, int NB, bool SQ, bool DYN>
__global__ void __launch_bounds__(TPB)
k_ct_mul(const i64* a, int na_rt, const i64* b, int nb_rt, i64* out, const i64* __restrict__ gcrt, i64 slab, u32 per,
         CtMulScale sc, const ModCtx* __restrict__ mod) {
  constexpr int W = V2 ? 2 : 1;
  constexpr i64 TILE = (i64)TPB * EPT * W;
  constexpr int UNROLL_E = DYN ? 1 : EPT;                     // the run-time form is long enough as a loop
  const int na = DYN ? na_rt : NA, nb = DYN ? nb_rt : NB;     // wave-uniform
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
  const u32 r_s = (u32)((u64)s0 % per);
#pragma unroll UNROLL_E
  for (int e = 0; e < EPT; ++e) {
    const u32 l = ((u32)e * TPB + threadIdx.x) * W;
    const i64 g = s0 + l;
    if (g >= slab) continue;
    u32 r = r_s + l;
    if (r >= per) r %= per;                                   // V2: per is even, so r and r + 1 are one polynomial's
    // x: a, taken times ga below; y: b, or a itself for the square (read once)
    u64 x[NA][W], y[NB][W], gv[W];
#pragma unroll
    for (int i = 0; i < NA; ++i)
      if (i < na) load_words<W>(a + i * slab + g, x[i]);
    if constexpr (!SQ) {
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (j < nb) load_words<W>(b + j * slab + g, y[j]);
    }
    load_words<W>(gcrt + r, gv);
    // per word: its modulus and ga = alpha_t gCRT, which the shorter operand a takes before the products: na reductions
    // in place of one more per output
    u32 t = r % (u32)sc.T;
    ModCtx mc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      mc[w] = mod[t];
      const u64 q = mc[w].q;
      const u64 ga = trim(shoup_lazy(gv[w], sc.a[t], sc.ap[t], q), q);
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < na) {
          const u64 v = canon_in((i64)x[i][w], q);
          if constexpr (SQ) y[i][w] = v;
          x[i][w] = mulmod(ga, v, mc[w]);
        }
      if constexpr (!SQ) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
          if (j < nb) y[j][w] = canon_in((i64)y[j][w], q);
      }
      if (++t == (u32)sc.T) t = 0;
    }
    // out never overlaps a or b (the output has more components than either), so each component is stored as it is made
#pragma unroll
    for (int k = 0; k < NA + NB - 1; ++k) {
      if (k >= na + nb - 1) continue;
      u64 o[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        u128 acc = 0;
        int cnt = 0;
        if constexpr (SQ) {
          // 2 sum_{i < j, i + j = k} (ga a_i) a_j + (ga a_(k/2)) a_(k/2): the cross terms once, doubled; the doubled sum
          // counts as twice its terms
#pragma unroll
          for (int i = 0; i < NA; ++i) {
            const int j = k - i;
            if (j <= i || j >= NA) continue;
            if (j < na) add_term(acc, cnt, x[i][w], y[j][w], mc[w], i - (k - (NA - 1) > 0 ? k - (NA - 1) : 0));
          }
          const bool diag = (k & 1) == 0 && k / 2 < na;
          if (2 * cnt + (diag ? 1 : 0) <= LAZY) acc <<= 1;
          else acc = (u128)(2 * rem(acc, mc[w]));                                     // < 2 q: not more than one term
          if (diag) acc += (u128)x[k / 2][w] * y[k / 2][w];
          o[w] = rem(acc, mc[w]);
        } else {
          const int i0 = k - (NB - 1) > 0 ? k - (NB - 1) : 0;                     // the sum's first slot
#pragma unroll
          for (int i = 0; i < NA; ++i) {
            const int j = k - i;
            if (j < 0 || j >= NB) continue;
            if (i < na && j < nb) add_term(acc, cnt, x[i][w], y[j][w], mc[w], i - i0);
          }
          o[w] = rem(acc, mc[w]);
        }
      }
      store_words<W>(out + k * slab + g, o);
    }
  }
}

hipError_t launch_ct_mul(hipStream_t s, const i64* a, int na, const i64* b, int nb, i64* out, i64 B, i64 n,
                         const CtMulScale& sc, const i64* gcrt, const ModCtx* mod) {
  const int T = sc.T;
  const i64 per = n * T, slab = B * per;
  if (slab == 0) return hipSuccess;
  if (T < 1 || T > PIPE_MAX_T || per > 0x7fffffff || na < 1 || nb < 1 || na > LOLHIP_CT_MUL_MAX || nb > LOLHIP_CT_MUL_MAX)
    return hipErrorInvalidValue;
  const bool sq = a == b && na == nb;
  if (na > nb) { std::swap(a, b); std::swap(na, nb); }         // the product commutes: a is the shorter operand
  // the run-time form stays with one word per lane: with two it holds 2 x 16 operand words per lane and measured slower
  // (4 x 4: 0.158 against 0.136 ms, 8 x 8: 0.322 against 0.281 ms at m = 2^15, T = 4, B = 64)
  const bool dyn = nb > STATIC_MAX;
  const bool v2 = !dyn && (per & 1) == 0 && aligned16(a, b, out, gcrt);
  unsigned blocks;
  if (!tiles_for(slab, (i64)TPB * EPT * (v2 ? 2 : 1), &blocks)) return hipErrorInvalidValue;
#define LOLHIP_CM(VV, NA, NB, SQ, DYN)                                                                              \
  hipLaunchKernelGGL((k_ct_mul<VV, NA, NB, SQ, DYN>), dim3(blocks), dim3(TPB), 0, s, a, na, b, nb, out, gcrt, slab, \
                     (u32)per, sc, mod)
#define LOLHIP_CM_V(NA, NB, SQ, DYN) \
  do { if (v2) LOLHIP_CM(true, NA, NB, SQ, DYN); else LOLHIP_CM(false, NA, NB, SQ, DYN); } while (0)
  constexpr int M = LOLHIP_CT_MUL_MAX;
  if (dyn) { if (sq) LOLHIP_CM(false, M, M, true, true); else LOLHIP_CM(false, M, M, false, true); }
  else if (sq) { if (na == 1) LOLHIP_CM_V(1, 1, true, false); else if (na == 2) LOLHIP_CM_V(2, 2, true, false); else LOLHIP_CM_V(3, 3, true, false); }
  else if (na == 1) { if (nb == 1) LOLHIP_CM_V(1, 1, false, false); else if (nb == 2) LOLHIP_CM_V(1, 2, false, false); else LOLHIP_CM_V(1, 3, false, false); }
  else if (na == 2) { if (nb == 2) LOLHIP_CM_V(2, 2, false, false); else LOLHIP_CM_V(2, 3, false, false); }
  else LOLHIP_CM_V(3, 3, false, false);
#undef LOLHIP_CM_V
#undef LOLHIP_CM
  return hipGetLastError();
}

}  // namespace lolhip
