// lol_amd/csrc/rlwe.hip — the kernels of RLWE / RLWR sampling and instance verification (lol
// RLWE/{Continuous,Discrete,RLWR}.hs; rlwe-challenges Generate.hs:192-218, Verify.hs:346-366) that no other unit
// provides.  gfx950 only.
//
//   k_gsqnorm        gSqNormDec (Tensor.hs:147-151; norm.cpp:15-75): <e, y>, y = (⊗_p I_{p^(e-1)} ⊗ (I+J)_{p-1}) e over the
//                    odd primes of the index, one LDS-resident copy of the sample, int64 (exact or saturated) or double
//   k_rlwe_uniform   uniform a from the ChaCha20 stream (the layout of encrypt.hip's c^1), alone, with a s, or added
//                    into reduce e
//   k_rlwe_as        a s or b - a s, one pointwise pass (the sibling of decrypt.hip k_sk_eval for operands that are not
//                    one [ncomp] slab and carry a sign)
//   k_rlwe_cont_*    the K/(qR) arithmetic of RRq.hs:47-84 in IEEE doubles, no contraction
//   k_rlwr_*         the rounding R_q -> R_p of RLWR.hs:34-44, written out or compared and counted per sample
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "kernel_dev.h"
#include "rlwe.h"
#include "rlwe_dev.h"
#include "rng_dev.h"

// b = f(x, g) and e = f(x, b) are pure functions of their IEEE double operations in the stated order (include/lolhip.h)
#pragma clang fp contract(off)

namespace lolhip {

typedef __int128 i128;

namespace {
constexpr int TPB = 256;
constexpr unsigned MAX_GRID_Y = 65535;
constexpr int EPT = 2;                       // elements per thread (k_rlwe_as)
constexpr i64 TILE = 256 * EPT;

// ---------------------------------------------------------------------------------------
// gSqNorm.  A workgroup holds S whole samples (S n contiguous words) in LDS; a team of R = 2^lgR lanes owns one sample
// and keeps its coefficients r, r + R, ... in registers (at most NORM_EPT each), so e is read from HBM once:
//   n <= 256          S = floor(256 / n) samples per 256 threads, R = 2^floor(log2 (256 / S)) (the teams fill the workgroup)
//   n <= 4096         S = 1, R = 256
//   n <= 16384        S = 1, R = 1024 (128 KiB of LDS at n = 16384)
// The odd primes' stages run in place on the S n words as one array (a batch of samples is the same operator with
// S times the left identity), one thread per vector of p - 1.  Then each lane sums its products in coefficient
// order, the team's lanes are added by a halving tree of shuffles and, for R > 64, the team's waves' partials in wave
// order: the order is a function of n alone.
// ---------------------------------------------------------------------------------------
constexpr int NORM_EPT = 16;
constexpr int NORM_GRID = 1024;

template <typename V> struct NormAcc;
template <> struct NormAcc<i64> { typedef i128 type; };
template <> struct NormAcc<double> { typedef double type; };

__device__ __forceinline__ double team_down(double v, int off, int w) { return __shfl_down(v, off, w); }
__device__ __forceinline__ i128 team_down(i128 v, int off, int w) {
  const unsigned long long lo = __shfl_down((unsigned long long)(u128)v, off, w);
  const unsigned long long hi = __shfl_down((unsigned long long)((u128)v >> 64), off, w);
  return (i128)((u128)hi << 64 | lo);
}

template <typename V>
__global__ void __launch_bounds__(1024)
k_gsqnorm(const V* __restrict__ e, V* __restrict__ out, i64 B, int n, int S, int lgR, NormDims nd) {
  typedef typename NormAcc<V>::type A;
  extern __shared__ unsigned char norm_lds[];
  V* y = reinterpret_cast<V*>(norm_lds);
  __shared__ A wpart[16];
  __shared__ int sflag[256];                   // int64: the sample saturates (a coefficient beyond 32 bits)
  const int t = threadIdx.x, R = 1 << lgR;
  const int s = t >> lgR, r = t & (R - 1);
  const int len = S * n;
  const i64 tiles = (B + S - 1) / S;
  if (t < 256) sflag[t] = 0;
  __syncthreads();
  for (i64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const i64 b = tile * S + s;
    const bool own = s < S, live = own && b < B;
    V ev[NORM_EPT];
    bool sat = false;
#pragma unroll
    for (int i = 0; i < NORM_EPT; ++i) {
      const int j = r + (i << lgR);
      V v = 0;
      if (live && j < n) v = e[b * n + j];
      if constexpr (sizeof(A) == 16) {         // |e_j| >= 2^32 (INT64_MIN included): the form is >= e_j^2 > INT64_MAX
        if (v >= ((i64)1 << 32) || v <= -((i64)1 << 32)) { sat = true; v = 0; }
      }
      ev[i] = v;
      if (own && j < n) y[s * n + j] = v;
    }
    if constexpr (sizeof(A) == 16) {
      if (sat) atomicOr(&sflag[s], 1);
    }
    __syncthreads();
    for (int k = 0; k < nd.k; ++k) {           // y += the sum over its prime dimension (pNormSq, norm.cpp:15-37)
      const int d = nd.d[k], rts = nd.rts[k];
      const int groups = len / d;
      for (int g = t; g < groups; g += blockDim.x) {
        const int blk = g / rts, mo = g - blk * rts;
        V* v = y + blk * rts * d + mo;
        V sum = 0;
        for (int i = 0; i < d; ++i) sum += v[i * rts];
        for (int i = 0; i < d; ++i) v[i * rts] += sum;
      }
      __syncthreads();
    }
    A acc = 0;
#pragma unroll
    for (int i = 0; i < NORM_EPT; ++i) {
      const int j = r + (i << lgR);
      if (own && j < n) acc += (A)ev[i] * (A)y[s * n + j];
    }
    const int w = R < 64 ? R : 64;
    for (int off = w >> 1; off > 0; off >>= 1) acc += team_down(acc, off, w);
    if (R > 64) {                              // a team of whole waves: their partials, added in wave order
      if ((t & 63) == 0) wpart[t >> 6] = acc;
      __syncthreads();
      if (r == 0)
        for (int i = 1; i < (R >> 6); ++i) acc += wpart[(t >> 6) + i];
    }
    if (live && r == 0) {
      if constexpr (sizeof(A) == 16) {
        const bool over = sflag[s] != 0 || acc > (i128)INT64_MAX;
        out[b] = over ? INT64_MAX : (i64)acc;
      } else {
        out[b] = acc;
      }
    }
    __syncthreads();                           // y, wpart and sflag are free again
    if constexpr (sizeof(A) == 16) {
      if (t < 256) sflag[t] = 0;
      __syncthreads();
    }
  }
}

template <typename V>
hipError_t launch_gsqnorm(hipStream_t st, const V* e, V* out, i64 B, i64 n, const NormDims& nd) {
  if (B == 0) return hipSuccess;
  if (n < 1 || n > NORM_MAX_N || nd.k < 0 || nd.k > NORM_MAX_PRIMES) return hipErrorInvalidValue;
  for (int k = 0; k < nd.k; ++k)
    if (nd.d[k] < 1 || nd.rts[k] < 1 || n % ((i64)nd.d[k] * nd.rts[k])) return hipErrorInvalidValue;
  int S = 1, lgR = 0, threads = TPB;
  if (n <= 256) {
    S = (int)(256 / n);
    while ((2 << lgR) * S <= 256) ++lgR;
  } else {
    threads = n <= 4096 ? 256 : 1024;
    lgR = n <= 4096 ? 8 : 10;
  }
  const size_t lds = (size_t)S * (size_t)n * sizeof(V);
  if (lds > 64 * 1024) {
    hipError_t er = allow_big_lds<&k_gsqnorm<V>>(128 * 1024);
    if (er != hipSuccess) return er;
  }
  const i64 tiles = (B + S - 1) / S;
  const unsigned grid = (unsigned)(tiles < NORM_GRID ? tiles : NORM_GRID);
  hipLaunchKernelGGL(k_gsqnorm<V>, dim3(grid), dim3((unsigned)threads), lds, st, e, out, B, (int)n, S, lgR, nd);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_gsqnorm_i64(hipStream_t s, const i64* e, i64* out, i64 B, i64 n, const NormDims& nd) {
  return launch_gsqnorm<i64>(s, e, out, B, n, nd);
}
hipError_t launch_gsqnorm_f64(hipStream_t s, const double* e, double* out, i64 B, i64 n, const NormDims& nd) {
  return launch_gsqnorm<double>(s, e, out, B, n, nd);
}

// ---------------------------------------------------------------------------------------
// uniform a (CRT basis), 4 residues per block: r = j*T + t -> (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q_t, and
// out = a s / out += a s.  One thread per ChaCha20 block, batch items over the grid's y dimension.
// ---------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(TPB)
k_rlwe_uniform(i64* __restrict__ a, const i64* __restrict__ s_crt, i64* __restrict__ out, i64 B, i64 nT, int T,
               const ModCtx* __restrict__ mod, ChaChaKey key, u64 ctr, int domain) {
  const i64 nblk = (nT + 3) >> 2;
  const i64 k = (i64)blockIdx.x * TPB + threadIdx.x;
  if (k >= nblk) return;
  const int cnt = nT - 4 * k < 4 ? (int)(nT - 4 * k) : 4;
  for (i64 b = blockIdx.y; b < B; b += gridDim.y) {
    u32 w[16];
    stream_block(key, ctr, domain, b, (u32)k, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= cnt) continue;
      const i64 r = 4 * k + i;
      const ModCtx mc = mod[(u32)r % (u32)T];
      const u64 lo = (u64)w[4 * i] | (u64)w[4 * i + 1] << 32, hi = (u64)w[4 * i + 2] | (u64)w[4 * i + 3] << 32;
      const u64 u = reduce128(hi, lo, mc);
      const i64 g = b * nT + r;
      a[g] = (i64)u;
      if constexpr (MODE != RLWE_U_ONLY) {
        const u64 us = mulmod(u, canon_in(s_crt[r], mc.q), mc);
        out[g] = (i64)(MODE == RLWE_U_ADD ? addmod(canon_in(out[g], mc.q), us, mc.q) : us);
      }
    }
  }
}

hipError_t launch_rlwe_uniform(hipStream_t s, int mode, i64* a, const i64* s_crt, i64* out, i64 B, i64 n, int T,
                               const ModCtx* mod, const ChaChaKey& key, u64 ctr, int domain) {
  const i64 nT = n * T;
  if (B == 0 || nT == 0) return hipSuccess;
  if (T < 1) return hipErrorInvalidValue;
  unsigned x;
  if (!tiles_for((nT + 3) >> 2, TPB, &x)) return hipErrorInvalidValue;
  const dim3 grid(x, (unsigned)(B < (i64)MAX_GRID_Y ? B : MAX_GRID_Y)), block(TPB);
  if (mode == RLWE_U_ONLY)
    hipLaunchKernelGGL(k_rlwe_uniform<RLWE_U_ONLY>, grid, block, 0, s, a, s_crt, out, B, nT, T, mod, key, ctr, domain);
  else if (mode == RLWE_U_PROD)
    hipLaunchKernelGGL(k_rlwe_uniform<RLWE_U_PROD>, grid, block, 0, s, a, s_crt, out, B, nT, T, mod, key, ctr, domain);
  else if (mode == RLWE_U_ADD)
    hipLaunchKernelGGL(k_rlwe_uniform<RLWE_U_ADD>, grid, block, 0, s, a, s_crt, out, B, nT, T, mod, key, ctr, domain);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// out = a s, or b - a s: [B][n][T] in the CRT basis, s [n][T] broadcast.  out may alias a or b.
// ---------------------------------------------------------------------------------------
template <bool SUB>
__global__ void __launch_bounds__(256)
k_rlwe_as(const i64* a, const i64* b, const i64* __restrict__ s_crt, i64* out, i64 total, u32 per, int T,
          const ModCtx* __restrict__ mod) {
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
  const u32 r_s = (u32)((u64)s0 % per);
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const u32 l = (u32)e * 256u + threadIdx.x;
    const i64 g = s0 + l;
    if (g >= total) continue;
    u32 r = r_s + l;
    if (r >= per) r %= per;
    const ModCtx mc = mod[r % (u32)T];
    const u64 as = mulmod(canon_in(a[g], mc.q), canon_in(s_crt[r], mc.q), mc);
    out[g] = (i64)(SUB ? submod(canon_in(b[g], mc.q), as, mc.q) : as);
  }
}

hipError_t launch_rlwe_as(hipStream_t s, const i64* a, const i64* b, const i64* s_crt, i64* out, i64 B, i64 n, int T,
                          const ModCtx* mod) {
  const i64 total = B * n * T;
  if (total == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(total, TILE, &blocks)) return hipErrorInvalidValue;
  if (b) hipLaunchKernelGGL(k_rlwe_as<true>, dim3(blocks), dim3(256), 0, s, a, b, s_crt, out, total, (u32)(n * T), T, mod);
  else hipLaunchKernelGGL(k_rlwe_as<false>, dim3(blocks), dim3(256), 0, s, a, b, s_crt, out, total, (u32)(n * T), T, mod);
  return hipGetLastError();
}

template <bool ERR>
__global__ void __launch_bounds__(256)
k_rlwe_cont(const i64* __restrict__ x, const double* __restrict__ in, double* __restrict__ out, i64 total, double q) {
  const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const double xd = (double)x[g];
  if constexpr (ERR) {
    const double yv = rrq_add(in[g], rrq_reduce(-xd, q), q);
    out[g] = yv + yv < q ? yv : yv - q;
  } else {
    out[g] = rrq_add(xd, rrq_reduce(in[g], q), q);
  }
}

hipError_t launch_rlwe_cont_sample(hipStream_t s, const i64* x, const double* g, double* b, i64 total, double q) {
  if (total == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(total, 256, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rlwe_cont<false>, dim3(blocks), dim3(256), 0, s, x, g, b, total, q);
  return hipGetLastError();
}

hipError_t launch_rlwe_cont_error(hipStream_t s, const i64* x, const double* b, double* e, i64 total, double q) {
  if (total == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(total, 256, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rlwe_cont<true>, dim3(blocks), dim3(256), 0, s, x, b, e, total, q);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256)
k_rlwr_round(const i64* __restrict__ x, i64* __restrict__ out, i64 total, u64 q, u64 p) {
  const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  out[g] = rlwr_round(canon_in(x[g], q), q, p);
}

// one wave per sample, four samples per workgroup; the counts are integers, so the shuffle tree's order is immaterial
__global__ void __launch_bounds__(256)
k_rlwr_check(const i64* __restrict__ x, const i64* __restrict__ given, int32_t* __restrict__ mismatch, i64 B, int n,
             u64 q, u64 p) {
  const int lane = threadIdx.x & 63;
  for (i64 b = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += (i64)gridDim.x * 4) {
    int c = 0;
    for (int j = lane; j < n; j += 64) c += rlwr_round(canon_in(x[b * n + j], q), q, p) != given[b * n + j];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if (lane == 0) mismatch[b] = c;
  }
}

hipError_t launch_rlwr_round(hipStream_t s, const i64* x, i64* out, i64 total, u64 q, u64 p) {
  if (total == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(total, 256, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rlwr_round, dim3(blocks), dim3(256), 0, s, x, out, total, q, p);
  return hipGetLastError();
}

hipError_t launch_rlwr_check(hipStream_t s, const i64* x, const i64* given, int32_t* mismatch, i64 B, i64 n, u64 q,
                             u64 p) {
  if (B == 0) return hipSuccess;
  const i64 groups = (B + 3) / 4;
  const unsigned grid = (unsigned)(groups < 8192 ? groups : 8192);
  hipLaunchKernelGGL(k_rlwr_check, dim3(grid), dim3(256), 0, s, x, given, mismatch, B, (int)n, q, p);
  return hipGetLastError();
}

}  // namespace lolhip
