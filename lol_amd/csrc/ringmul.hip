// lol_amd/csrc/ringmul.hip — the two element-wise passes of the exact ring product a * b in R_q = Z_q[zeta_m] for
// moduli q_0 .. q_(T-1) that need no CRT basis (2^e, p^e, odd composites): the product runs over the
// integers modulo K <= 3 NTT primes Q_i whose product exceeds twice the largest product coefficient (the existing
// poly-mul over the plan of the Q_i), and these passes are the way in and the way out.
//
//   k_ring_lift   [rows][n][T] any int64 -> centred lift mod q_t -> its K residues, [rows * T][n][K]
//   k_ring_fold   [rows * T][n][K] -> mixed-radix digits (Garner, as decrypt.hip's k_lift) -> sign by a most-
//                 significant-first comparison with the digits of floor((prod Q - 1) / 2) -> sum_i v_i (P_i mod q_t),
//                 minus prod Q mod q_t for a negative value -> [rows][n][T] in [0, q_t).  No wide integers.
//
// One thread per coefficient (pair) of a row, the T components in a wave-uniform loop: the constants of a component
// are scalar loads from the launch struct, the K-residue side moves 16 bytes per access and lane, the [n][T] side
// 16 bytes when T = 1 and T strided 8-byte words otherwise (consecutive lanes and iterations fill every line).
// HBM-bound: 8 bytes on the [n][T] side and 8 K bytes on the other per word.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "ringmul.h"
#include "ringmul_dev.h"

namespace lolhip {

namespace {
// V2: every slab is 16-byte aligned and n is even; two coefficients per thread
template <int K, bool POW2, bool V2>
__global__ void __launch_bounds__(RING_TPB)
k_ring_lift(const i64* __restrict__ in, i64* __restrict__ out, i64 rows, i64 n, RingMul c) {
  constexpr int W = V2 ? 2 : 1;
  const int T = c.T;
  const i64 per = n / W;
  for (i64 r = blockIdx.y; r < rows; r += gridDim.y) {
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < per; g += (i64)gridDim.x * blockDim.x) {
      const i64 j = g * W;
      const i64* src = in + (r * n + j) * T;
      for (int t = 0; t < T; ++t) {
        const ModCtx mc = c.q[t];
        i64 x[W];
        if (V2 && T == 1) {
          const longlong2 a = *reinterpret_cast<const longlong2*>(src);
          x[0] = a.x;
          x[W - 1] = a.y;
        } else {
#pragma unroll
          for (int w = 0; w < W; ++w) x[w] = src[(i64)w * T + t];
        }
        u64 y[W * K];
#pragma unroll
        for (int w = 0; w < W; ++w) lift_word<K, POW2>(x[w], mc, c, y + w * K);
        i64* dst = out + ((r * T + t) * n + j) * K;
        if constexpr (V2) {
#pragma unroll
          for (int i = 0; i < K; ++i) reinterpret_cast<u64x2*>(dst)[i] = u64x2{y[2 * i], y[2 * i + 1]};
        } else {
#pragma unroll
          for (int k = 0; k < K; ++k) dst[k] = (i64)y[k];
        }
      }
    }
  }
}

template <int K, bool POW2, bool V2>
__global__ void __launch_bounds__(RING_TPB)
k_ring_fold(const i64* __restrict__ in, i64* __restrict__ out, i64 rows, i64 n, RingMul c) {
  constexpr int W = V2 ? 2 : 1;
  const int T = c.T;
  const i64 per = n / W;
  for (i64 r = blockIdx.y; r < rows; r += gridDim.y) {
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < per; g += (i64)gridDim.x * blockDim.x) {
      const i64 j = g * W;
      i64* dst = out + (r * n + j) * T;
      for (int t = 0; t < T; ++t) {
        const ModCtx mc = c.q[t];
        const i64* src = in + ((r * T + t) * n + j) * K;
        u64 x[W * K];
        if constexpr (V2) {
#pragma unroll
          for (int i = 0; i < K; ++i) {
            const u64x2 a = reinterpret_cast<const u64x2*>(src)[i];
            x[2 * i] = a.x;
            x[2 * i + 1] = a.y;
          }
        } else {
#pragma unroll
          for (int k = 0; k < K; ++k) x[k] = (u64)src[k];
        }
        u64 y[W];
#pragma unroll
        for (int w = 0; w < W; ++w) y[w] = fold_word<K, POW2>(x + w * K, mc, t, c);
        if (V2 && T == 1) {
          *reinterpret_cast<u64x2*>(dst) = u64x2{y[0], y[W - 1]};
        } else {
#pragma unroll
          for (int w = 0; w < W; ++w) dst[(i64)w * T + t] = (i64)y[w];
        }
      }
    }
  }
}

bool params_ok(const i64* in, const i64* out, i64 rows, i64 n, const RingMul& c) {
  return in && out && rows > 0 && n > 0 && c.T >= 1 && c.T <= RING_MAX_T && c.K >= 1 && c.K <= RING_MAX_K &&
         rows <= 0x7fffffff / c.T;
}
}  // namespace

#define LOLHIP_RING_LAUNCH(KERNEL)                                                                                  \
  do {                                                                                                              \
    const bool v2 = aligned16(in, out) && n % 2 == 0;                                                               \
    const RingShape sh = ring_shape_for(rows, v2 ? n / 2 : n);                                                      \
    const bool p2 = c.pow2 != 0;                                                                                    \
    switch (c.K * 4 + (p2 ? 2 : 0) + (v2 ? 1 : 0)) {                                                                \
      case 4:  hipLaunchKernelGGL((KERNEL<1, false, false>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;  \
      case 5:  hipLaunchKernelGGL((KERNEL<1, false, true>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;   \
      case 6:  hipLaunchKernelGGL((KERNEL<1, true, false>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;   \
      case 7:  hipLaunchKernelGGL((KERNEL<1, true, true>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;    \
      case 8:  hipLaunchKernelGGL((KERNEL<2, false, false>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;  \
      case 9:  hipLaunchKernelGGL((KERNEL<2, false, true>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;   \
      case 10: hipLaunchKernelGGL((KERNEL<2, true, false>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;   \
      case 11: hipLaunchKernelGGL((KERNEL<2, true, true>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;    \
      case 12: hipLaunchKernelGGL((KERNEL<3, false, false>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;  \
      case 13: hipLaunchKernelGGL((KERNEL<3, false, true>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;   \
      case 14: hipLaunchKernelGGL((KERNEL<3, true, false>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;   \
      default: hipLaunchKernelGGL((KERNEL<3, true, true>), sh.grid, sh.block, 0, s, in, out, rows, n, c); break;    \
    }                                                                                                               \
  } while (0)

hipError_t launch_ring_lift(hipStream_t s, const i64* in, i64* out, i64 rows, i64 n, const RingMul& c) {
  if (rows == 0 || n == 0) return hipSuccess;
  if (!params_ok(in, out, rows, n, c)) return hipErrorInvalidValue;
  LOLHIP_RING_LAUNCH(k_ring_lift);
  return hipGetLastError();
}

hipError_t launch_ring_fold(hipStream_t s, const i64* in, i64* out, i64 rows, i64 n, const RingMul& c) {
  if (rows == 0 || n == 0) return hipSuccess;
  if (!params_ok(in, out, rows, n, c)) return hipErrorInvalidValue;
  LOLHIP_RING_LAUNCH(k_ring_fold);
  return hipGetLastError();
}
#undef LOLHIP_RING_LAUNCH

}  // namespace lolhip
