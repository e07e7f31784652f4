// lol_amd/csrc/encrypt.hip — the kernels of SymmSHE encrypt and genSK (lol-apps SymmSHE.hs:120-146) that no Tensor
// member provides: samplers over the ChaCha20 stream of rng_dev.h.  gfx950 only.
//
//   k_enc_gauss    Box-Muller Gaussians of scaled deviation sigma as a double slab [B][n] (the input of the
//                  decoding-basis map k_gauss for an index that is not a power of two)
//   k_enc_error    coset rounding e_j = rep_j + p round((g_j - rep_j) / p) (roundCoset, Prelude.hs:156-161; Haskell's
//                  round: half to even), Gaussians from the stream (m' = 2^k: the map is the identity) or from a
//                  double slab; written as T residues, added to T residues, or written as int64 (errorRounded:
//                  p = 1, rep = 0)
//   k_enc_combine  c^1 uniform from the stream, c^0 = e^ - c^1 s^ (CRT basis; e^ read in place)
//   k_enc_uniform  c^1 and -c^1 s^ as a [2][B] slab (CRT basis), for one batched crtInv
//
// One thread per ChaCha20 block: 8 Gaussian coefficients (4 Box-Muller pairs) or 4 uniform residues.  Batch items
// run over the grid's y dimension; the key and the stream offset travel by value.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "pipeline.h"
#include "rlwe_dev.h"
#include "rng_dev.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;
constexpr unsigned MAX_GRID_Y = 65535;

bool grid_for(i64 nblk, i64 B, dim3* grid) {
  unsigned x;
  if (!tiles_for(nblk, TPB, &x)) return false;
  *grid = dim3(x, (unsigned)(B < (i64)MAX_GRID_Y ? B : MAX_GRID_Y));
  return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Gaussians into a double slab [B][n]
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_enc_gauss(double* __restrict__ d, i64 B, i64 n, ChaChaKey key, u64 ctr, int domain, double sigma) {
  const i64 nblk = (n + 7) >> 3;
  const i64 k = (i64)blockIdx.x * TPB + threadIdx.x;
  if (k >= nblk) return;
  for (i64 b = blockIdx.y; b < B; b += gridDim.y) {
    double g[8];
    gauss8(key, ctr, domain, b, (u32)k, sigma, g);
    double* o = d + b * n + 8 * k;
    const int cnt = n - 8 * k < 8 ? (int)(n - 8 * k) : 8;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < cnt) o[i] = g[i];
  }
}

hipError_t launch_enc_gauss(hipStream_t s, double* d, i64 B, i64 n, const ChaChaKey& key, u64 ctr, int domain,
                            double sigma) {
  if (B == 0 || n == 0) return hipSuccess;
  dim3 grid;
  if (!grid_for((n + 7) >> 3, B, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_enc_gauss, grid, dim3(TPB), 0, s, d, B, n, key, ctr, domain, sigma);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// coset rounding and reduction.  FROM_D: Gaussians read from d (else generated); rep [B][n] (any representative in
// (-p, p), lifted centred here) or null for 0.  MODE: ENC_WRITE / ENC_ADD residues [B][n][T], ENC_INT int64 [B][n].
// ENC_INT may run in place over d (each thread reads its 8 doubles before it writes the same 8 words).  Every thread of
// a workgroup reaches the barriers of the residue modes (no early exit).
// ---------------------------------------------------------------------------------------
template <bool FROM_D, int MODE>
__global__ void __launch_bounds__(TPB)
k_enc_error(const double* d, const i64* __restrict__ rep, i64 p, i64* out, i64 B, i64 n, int T,
            const ModCtx* __restrict__ mod, ChaChaKey key, u64 ctr, int domain, double sigma) {
  __shared__ i64 se[TPB * 8];                                   // the block's coefficients, for coalesced residue stores
  const i64 nblk = (n + 7) >> 3;
  const i64 k = (i64)blockIdx.x * TPB + threadIdx.x;
  const bool live = k < nblk;
  const int cnt = !live ? 0 : n - 8 * k < 8 ? (int)(n - 8 * k) : 8;
  const i64 cb = (i64)blockIdx.x * TPB * 8;                     // first coefficient of the workgroup
  const u32 ncb = n - cb < TPB * 8 ? (u32)(n - cb) : (u32)(TPB * 8);
  const double pd = (double)p;
  for (i64 b = blockIdx.y; b < B; b += gridDim.y) {
    const i64 j0 = b * n + 8 * k;
    double g[8];
    if constexpr (FROM_D) {
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i] = i < cnt ? d[j0 + i] : 0.0;
    } else {
      if (live) gauss8(key, ctr, domain, b, (u32)k, sigma, g);
    }
    i64 e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      i64 r = 0;
      if (rep && i < cnt) {
        const i64 x = rep[j0 + i];                              // (-p, p)
        r = x < 0 ? x + p : x;
        if (2 * r >= p) r -= p;                                 // [-p/2, p/2)
      }
      const double rd = (double)r;
      e[i] = i < cnt ? r + p * (i64)rint((g[i] - rd) / pd) : 0;
    }
    if constexpr (MODE == ENC_INT) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < cnt) out[j0 + i] = e[i];
    } else {
      // the workgroup's ncb coefficients x T residues are one contiguous run of the output: stage e in LDS, then
      // consecutive lanes store consecutive words
      __syncthreads();                                          // the previous item's reads of se are done
#pragma unroll
      for (int i = 0; i < 8; ++i) se[threadIdx.x * 8 + i] = e[i];
      __syncthreads();
      i64* ob = out + (b * n + cb) * T;
      const u32 words = ncb * (u32)T;
      for (u32 w = threadIdx.x; w < words; w += TPB) {
        const u32 c = w / (u32)T, t = w - c * (u32)T;
        const ModCtx mc = mod[t];
        const u64 v = mod_any(se[c], mc);
        ob[w] = (i64)(MODE == ENC_ADD ? addmod(canon_in(ob[w], mc.q), v, mc.q) : v);
      }
    }
  }
}

hipError_t launch_enc_error(hipStream_t s, const double* d, const i64* rep, i64 p, i64* out, i64 B, i64 n, int T,
                            const ModCtx* mod, int mode, const ChaChaKey& key, u64 ctr, int domain, double sigma) {
  if (B == 0 || n == 0) return hipSuccess;
  dim3 grid;
  if (!grid_for((n + 7) >> 3, B, &grid)) return hipErrorInvalidValue;
  const dim3 block(TPB);
#define LOLHIP_ENC_ERROR(FD, MD) \
  hipLaunchKernelGGL((k_enc_error<FD, MD>), grid, block, 0, s, d, rep, p, out, B, n, T, mod, key, ctr, domain, sigma)
  if (d) {
    if (mode == ENC_WRITE) LOLHIP_ENC_ERROR(true, ENC_WRITE);
    else if (mode == ENC_ADD) LOLHIP_ENC_ERROR(true, ENC_ADD);
    else LOLHIP_ENC_ERROR(true, ENC_INT);
  } else {
    if (mode == ENC_WRITE) LOLHIP_ENC_ERROR(false, ENC_WRITE);
    else if (mode == ENC_ADD) LOLHIP_ENC_ERROR(false, ENC_ADD);
    else LOLHIP_ENC_ERROR(false, ENC_INT);
  }
#undef LOLHIP_ENC_ERROR
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// uniform c^1 (CRT basis), 4 residues per block: r = j*T + t -> (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q_t
//   COMBINE: c1 = c^1, c0 = c0 - c^1 s^   (c0 holds e^)
//   else:    c1 = c^1, c0 = -c^1 s^
// ---------------------------------------------------------------------------------------
template <bool COMBINE>
__device__ __forceinline__ void enc_c1(i64* __restrict__ c0, i64* __restrict__ c1, const i64* __restrict__ s_crt,
                                       i64 B, i64 nT, int T, const ModCtx* __restrict__ mod, const ChaChaKey& key,
                                       u64 ctr) {
  const i64 nblk = (nT + 3) >> 2;
  const i64 k = (i64)blockIdx.x * TPB + threadIdx.x;
  if (k >= nblk) return;
  const int cnt = nT - 4 * k < 4 ? (int)(nT - 4 * k) : 4;
  for (i64 b = blockIdx.y; b < B; b += gridDim.y) {
    u32 w[16];
    stream_block(key, ctr, CHACHA_DOM_UNIFORM, b, (u32)k, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= cnt) continue;
      const i64 r = 4 * k + i;
      const ModCtx mc = mod[(u32)r % (u32)T];
      const u64 lo = (u64)w[4 * i] | (u64)w[4 * i + 1] << 32, hi = (u64)w[4 * i + 2] | (u64)w[4 * i + 3] << 32;
      const u64 u = reduce128(hi, lo, mc);
      const u64 us = mulmod(u, canon_in(s_crt[r], mc.q), mc);
      const i64 g = b * nT + r;
      c1[g] = (i64)u;
      c0[g] = (i64)submod(COMBINE ? canon_in(c0[g], mc.q) : 0, us, mc.q);
    }
  }
}

__global__ void __launch_bounds__(TPB)
k_enc_combine(i64* __restrict__ c0, i64* __restrict__ c1, const i64* __restrict__ s_crt, i64 B, i64 nT, int T,
              const ModCtx* __restrict__ mod, ChaChaKey key, u64 ctr) {
  enc_c1<true>(c0, c1, s_crt, B, nT, T, mod, key, ctr);
}

__global__ void __launch_bounds__(TPB)
k_enc_uniform(i64* __restrict__ c0, i64* __restrict__ c1, const i64* __restrict__ s_crt, i64 B, i64 nT, int T,
              const ModCtx* __restrict__ mod, ChaChaKey key, u64 ctr) {
  enc_c1<false>(c0, c1, s_crt, B, nT, T, mod, key, ctr);
}

hipError_t launch_enc_c1(hipStream_t s, bool combine, i64* c0, i64* c1, const i64* s_crt, i64 B, i64 n, int T,
                         const ModCtx* mod, const ChaChaKey& key, u64 ctr) {
  const i64 nT = n * T;
  if (B == 0 || nT == 0) return hipSuccess;
  if (T < 1) return hipErrorInvalidValue;
  dim3 grid;
  if (!grid_for((nT + 3) >> 2, B, &grid)) return hipErrorInvalidValue;
  if (combine) hipLaunchKernelGGL(k_enc_combine, grid, dim3(TPB), 0, s, c0, c1, s_crt, B, nT, T, mod, key, ctr);
  else hipLaunchKernelGGL(k_enc_uniform, grid, dim3(TPB), 0, s, c0, c1, s_crt, B, nT, T, mod, key, ctr);
  return hipGetLastError();
}

}  // namespace lolhip
