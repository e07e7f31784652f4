// lol_amd/csrc/khprf.hip — the kernels of the key-homomorphic ring PRF of [BP14] (lol-apps KeyHomomorphicPRF.hs:
// buildDecTree, ringPRF') that no other file provides.  gfx950 only.  One modulus (T = 1): slabs are [.][n] int64.
//
//   k_khprf_node    A_v = A_l * G^-1(A_r) for every slot of node v over an input window: out[k][j][c] =
//                   sum_i L[slot_l(k)][i][c] * D[i][slot_r(k)][j][c] mod q, CRT basis, the slots derived in the kernel
//                   from KhprfNode (by value)
//   k_khprf_keymul  s_key * A for nkeys keys in one pass: [nkeys][B][ell][n], CRT basis
//   k_khprf_round   rescaleDec to Z_p of decoding-basis residues, in place: fst (divModCent (p lift x) q) mod p
//   k_khprf_lift    the lifted family (q = 2^k, products exact mod an NTT prime Q): Z_Q -> Z_q (centred lift, mod q),
//                   Z_q -> Z_Q (centred lift) or both, and the 2-power rescaleMod to Z_p fused behind the first; two
//                   words per thread, 16-byte accesses
//
// The slot scheme (include/lolhip.h, lolhip_khprf_eval_batch): node v sees w_v = x >> s_v; its slot is w_v & (2^c_v - 1)
// when every one of the 2^c_v sub-inputs occurs in the window ("full") and w_v - (x0 >> s_v) otherwise.  Slot k of v
// stands for w_v = k (full) or (x0 >> s_v) + k, and its children's prefixes are w_v >> (s_child - s_v).  When the
// right child r is full, slots k, k + 2^c_r, k + 2 * 2^c_r, ... have one right slot: a thread takes KG of them, so
// each D word it loads serves KG left slots (and each L word JG entries) from registers.  When r is not full no two
// slots of v share a right slot (R = U_v: every group holds one slot).  A leaf child always counts as full: its two
// slots are a0 and a1, picked by the low bit of its prefix.  A full v has full children; the root's slots are the
// window itself (U = B, slot k = input x0 + k).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "elementwise_dev.h"
#include "pipeline.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;
constexpr int KG = 4;          // slots of v per thread that share one right slot
constexpr int JG = 4;          // output entries per thread
constexpr i64 MAX_BLOCKS = 1 << 20;

__device__ __forceinline__ i64 child_slot(i64 w_v, const KhprfChild& ch) {
  const i64 w = w_v >> ch.shift;
  return ch.full ? (w & ch.mask) : w - ch.lo;
}

unsigned grid_for(i64 total) { return grid_stride_blocks(total, TPB, MAX_BLOCKS); }
}  // namespace

// ---------------------------------------------------------------------------------------
// One thread per (coefficient c, group of JG entries, group of KG slots sharing a right slot): acc[KG][JG] over the ell
// digits.  Q32 (q < 2^32): 32x32-bit products into 64-bit sums, folded (Barrett, mu = floor(2^64/q)) every `fold` digits,
// fold (q - 1)^2 + q < 2^64 (the knapsack's q32 bound, per modulus).  Otherwise 128-bit sums folded every 8 digits
// (each term < q^2 < 2^124).  Threads are ordered c fastest, then the entry group, then the slot group: a wave reads
// 64 consecutive coefficients of one row, and the waves that read the same L rows are neighbours.
// ---------------------------------------------------------------------------------------
template <bool Q32>
__global__ void __launch_bounds__(TPB)
k_khprf_node(const i64* __restrict__ Lv, const i64* __restrict__ D, i64* __restrict__ out, KhprfNode nd, ModCtx mc,
             int fold, i64 nT, i64 nJ, i64 total) {
  const i64 n = nd.n, ln = (i64)nd.ell * n;
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
    const i64 tile = g / n, c = g - tile * n;
    const i64 kq = tile / nJ, jg = tile - kq * nJ;
    const i64 k0 = kq / nT, tg = kq - k0 * nT;
    const i64 kb = k0 + tg * KG * nd.R;                         // first slot of the group
    if (kb >= nd.U) continue;
    const i64 wb = nd.full ? kb : nd.lo + kb;
    const i64* dp = D + child_slot(wb, nd.r) * ln + c;         // right slot: one for the whole group
    const i64* lp[KG];
    bool kok[KG];
#pragma unroll
    for (int t = 0; t < KG; ++t) {
      const i64 k = kb + t * nd.R;
      kok[t] = k < nd.U;
      const i64 w = (nd.full ? 0 : nd.lo) + (kok[t] ? k : kb);  // a slot past U repeats the first one (not stored)
      lp[t] = Lv + child_slot(w, nd.l) * ln + c;
    }
    int jc[JG];
#pragma unroll
    for (int jj = 0; jj < JG; ++jj) {
      const int j = (int)jg * JG + jj;
      jc[jj] = j < nd.ell ? j : nd.ell - 1;                     // an entry past ell repeats the last one (not stored)
    }
    using Acc = std::conditional_t<Q32, u64, u128>;
    Acc acc[KG][JG];
#pragma unroll
    for (int t = 0; t < KG; ++t)
#pragma unroll
      for (int jj = 0; jj < JG; ++jj) acc[t][jj] = 0;
    auto red = [&](Acc a) -> u64 {
      if constexpr (Q32) {
        return trim(a - __umul64hi(a, mc.mu) * mc.q, mc.q);
      } else {
        return reduce128((u64)(a >> 64), (u64)a, mc);
      }
    };
    for (int i0 = 0; i0 < nd.ell; i0 += fold) {
      const int i1 = i0 + fold < nd.ell ? i0 + fold : nd.ell;
      for (int i = i0; i < i1; ++i) {
        u64 d[JG], a[KG];
#pragma unroll
        for (int jj = 0; jj < JG; ++jj) d[jj] = (u64)dp[i * nd.d_digit + (i64)jc[jj] * n];
#pragma unroll
        for (int t = 0; t < KG; ++t) a[t] = (u64)lp[t][(i64)i * n];
#pragma unroll
        for (int t = 0; t < KG; ++t)
#pragma unroll
          for (int jj = 0; jj < JG; ++jj) {
            if constexpr (Q32) acc[t][jj] += (u64)(u32)a[t] * (u32)d[jj];
            else acc[t][jj] += (u128)a[t] * d[jj];
          }
      }
#pragma unroll
      for (int t = 0; t < KG; ++t)
#pragma unroll
        for (int jj = 0; jj < JG; ++jj) acc[t][jj] = red(acc[t][jj]);
    }
#pragma unroll
    for (int t = 0; t < KG; ++t) {
      if (!kok[t]) continue;
      i64* o = out + (kb + t * nd.R) * ln + c;
#pragma unroll
      for (int jj = 0; jj < JG; ++jj)
        if ((int)jg * JG + jj < nd.ell) o[(i64)((int)jg * JG + jj) * n] = (i64)acc[t][jj];
    }
  }
}

hipError_t launch_khprf_node(hipStream_t s, const i64* L, const i64* D, i64* out, const KhprfNode& nd, const ModCtx& mc,
                             int fold) {
  if (nd.U <= 0 || nd.ell <= 0 || nd.n <= 0) return hipSuccess;
  if (nd.R < 1 || fold < 1) return hipErrorInvalidValue;
  const i64 nk0 = nd.R < nd.U ? nd.R : nd.U;
  const i64 per = (nd.U + nd.R - 1) / nd.R;                     // slots per right slot
  const i64 nT = (per + KG - 1) / KG, nJ = (nd.ell + JG - 1) / JG;
  const i64 total = nk0 * nT * nJ * nd.n;
  const bool q32 = mc.q < ((u64)1 << 32);
  if (q32) hipLaunchKernelGGL(k_khprf_node<true>, dim3(grid_for(total)), dim3(TPB), 0, s, L, D, out, nd, mc, fold, nT, nJ, total);
  else hipLaunchKernelGGL(k_khprf_node<false>, dim3(grid_for(total)), dim3(TPB), 0, s, L, D, out, nd, mc, 8, nT, nJ, total);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// out[key][r] = s[key][r % n] * A[r] mod q, r over the B*ell*n words of A: the nkeys products in one pass (A is read
// once per key, from L2 after the first)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_khprf_keymul(const i64* __restrict__ A, const i64* __restrict__ s_crt, i64* __restrict__ out, i64 per, i64 n,
               i64 total, ModCtx mc) {
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
    const i64 key = g / per, r = g - key * per;
    const i64 c = r % n;
    out[g] = (i64)mulmod(canon_in(s_crt[key * n + c], mc.q), canon_in(A[r], mc.q), mc);
  }
}

hipError_t launch_khprf_keymul(hipStream_t s, const i64* A, const i64* s_crt, i64* out, i64 nkeys, i64 rows, i64 n,
                               const ModCtx& mc) {
  const i64 per = rows * n, total = nkeys * per;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_khprf_keymul, dim3(grid_for(total)), dim3(TPB), 0, s, A, s_crt, out, per, n, total, mc);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// rescaleMod (Prelude.hs:144-153) of every word, in place: v = lift x (centred, q odd), y = floor((p v + q div 2) / q)
// mod p.  Shifted by p q to stay unsigned: a = p (v + q) + q div 2 < 1.5 p q + q / 2 < 2^64 (p q < 2^63, q < 2^62), the
// quotient floor(a / q) < 2p is exact through q^-1 mod 2^64 once the remainder is off, and equals y + p mod p.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_khprf_round(i64* __restrict__ y, i64 total, u64 p, ModCtx mc, u64 qinv) {
  const u64 q = mc.q;
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
    const u64 x = canon_in(y[g], q);
    const u64 vq = 2 * x < q ? x + q : x;                       // lift x + q, in (q/2, 3q/2)
    const u64 a = p * vq + (q >> 1);
    const u64 quot = (a - rem128(0, a, mc)) * qinv;
    y[g] = (i64)(quot >= p ? quot - p : quot);
  }
}

hipError_t launch_khprf_round(hipStream_t s, i64* y, i64 total, i64 p, const ModCtx& mc) {
  if (total == 0) return hipSuccess;
  if (!(mc.q & 1) || p < 2) return hipErrorInvalidValue;
  const u64 qinv = 0 - mc.nqinv;                                // q^-1 mod 2^64
  hipLaunchKernelGGL(k_khprf_round, dim3(grid_for(total)), dim3(TPB), 0, s, y, total, (u64)p, mc, qinv);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The lifted family's pass over powerful-basis (or decoding-basis) words, two per thread:
//   LIFT_FROM_Q  x in [0, Q) -> v = lift_Q x (centred) -> r = v mod q (q = 2^k: the low k bits), else r = x mod q
//   LIFT_TO_Q    r -> lift_q r in [-q/2, q/2) -> mod Q
//   LIFT_ROUND   r -> fst (divModCent (p lift_q r) q) mod p = ((p lift_q r + q/2) >> k) mod p (arithmetic shift:
//                floor; |p lift r| <= p q / 2 < 2^62), in [-p/2, p/2] before the final + p
// In place (src == dst) is allowed: every word is read and written by one thread.
// ---------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ i64 lift_one(i64 x, const KhprfLift& c) {
  const u64 mask = ((u64)1 << c.qbits) - 1;
  u64 r;
  if constexpr ((MODE & LIFT_FROM_Q) != 0) {
    const u64 xq = canon_in(x, c.Q);
    r = (u64)centred(xq, c.Q) & mask;
  } else {
    r = (u64)x & mask;
  }
  const i64 half = (i64)1 << (c.qbits - 1);
  const i64 lr = (i64)r >= half ? (i64)r - 2 * half : (i64)r;     // lift_q: [-q/2, q/2)
  if constexpr ((MODE & LIFT_TO_Q) != 0) {
    return lr < 0 ? lr + (i64)c.Q : lr;
  } else if constexpr ((MODE & LIFT_ROUND) != 0) {
    const i64 y = ((i64)c.p * lr + half) >> c.qbits;
    return y < 0 ? y + (i64)c.p : y;
  } else {
    return (i64)r;
  }
}

template <int MODE, bool V2>
__global__ void __launch_bounds__(TPB)
k_khprf_lift(const i64* src, i64* dst, i64 total, KhprfLift c) {
  if constexpr (V2) {
    const i64 pairs = total >> 1;
    for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < pairs; g += (i64)gridDim.x * TPB) {
      const longlong2 a = reinterpret_cast<const longlong2*>(src)[g];
      longlong2 b;
      b.x = lift_one<MODE>(a.x, c);
      b.y = lift_one<MODE>(a.y, c);
      reinterpret_cast<longlong2*>(dst)[g] = b;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (total & 1)) dst[total - 1] = lift_one<MODE>(src[total - 1], c);
  } else {                                                      // a slab not 16-byte aligned
    for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB)
      dst[g] = lift_one<MODE>(src[g], c);
  }
}

hipError_t launch_khprf_lift(hipStream_t s, const i64* src, i64* dst, i64 total, int mode, const KhprfLift& c) {
  if (total == 0) return hipSuccess;
  if (c.qbits < 1 || c.qbits > 62) return hipErrorInvalidValue;
  if ((mode & LIFT_ROUND) && ((mode & LIFT_TO_Q) || c.p < 2)) return hipErrorInvalidValue;
  const bool v2 = aligned16(src, dst);
  const unsigned grid = grid_for(v2 ? (total + 1) >> 1 : total);
#define LOLHIP_LIFT(M)                                                                                      \
  do {                                                                                                       \
    if (v2) hipLaunchKernelGGL((k_khprf_lift<M, true>), dim3(grid), dim3(TPB), 0, s, src, dst, total, c);    \
    else hipLaunchKernelGGL((k_khprf_lift<M, false>), dim3(grid), dim3(TPB), 0, s, src, dst, total, c);      \
  } while (0)
  switch (mode) {
    case LIFT_FROM_Q: LOLHIP_LIFT(LIFT_FROM_Q); break;
    case LIFT_TO_Q: LOLHIP_LIFT(LIFT_TO_Q); break;
    case LIFT_FROM_Q | LIFT_TO_Q: LOLHIP_LIFT(LIFT_FROM_Q | LIFT_TO_Q); break;
    case LIFT_ROUND: LOLHIP_LIFT(LIFT_ROUND); break;
    case LIFT_FROM_Q | LIFT_ROUND: LOLHIP_LIFT(LIFT_FROM_Q | LIFT_ROUND); break;
    default: return hipErrorInvalidValue;
  }
#undef LOLHIP_LIFT
  return hipGetLastError();
}

}  // namespace lolhip
