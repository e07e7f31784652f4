// lol_amd/csrc/kshint.hip — the kernels of SymmSHE's key-switch hints (ksHint / lweSample, lol-apps SymmSHE.hs:262-296;
// tunnelHint :531-545) that no other file provides.  gfx950 only.
//
//   k_kshint_combine  row j of hint b: h1 = c^1 uniform from the stream (domain 4), h0 = g_j val^ + e^ - c^1 s^, all in
//                     the CRT basis; e^ (the crt'd rounded Gaussians) read from a slab [B][L][n][T], the output
//                     written as [B][L][2][n][T]
//   k_unit_rows       the relative powerful-basis elements of tunnelHint as powerful-basis unit vectors [rel][n][T]
//
// The gadget entry g_j is derived in the kernel from DecompParams (by value): b^k mod q_t in its own component t, 0
// elsewhere, 1 for TrivGad, where row j is digit k of component t (components concatenated first to last, Gadget.hs:96-101)
// — the values lolhip_gadget returns, with no per-call table to upload.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "pipeline.h"
#include "rng_dev.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;
constexpr unsigned MAX_GRID_Y = 65535;

// x^k mod q (k < 64), once per row
__device__ __forceinline__ u64 powmod_dev(u64 x, int k, const ModCtx& mc) {
  u64 r = 1;                                               // q >= 2
  while (k) {
    if (k & 1) r = mulmod(r, x, mc);
    x = mulmod(x, x, mc);
    k >>= 1;
  }
  return r;
}
}  // namespace

// ---------------------------------------------------------------------------------------
// One thread per ChaCha20 block: 4 residues r = c*T + t of one row.  Rows (b, j) run over the grid's y dimension as
// row = b*L + j, so the L rows of one b are dispatched back to back and their reads of val^_b hit L2 after the first.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_kshint_combine(const i64* __restrict__ e_crt, const i64* __restrict__ vals, const i64* __restrict__ s_crt,
                 i64* __restrict__ hints, i64 B, i64 nT, DecompParams dp, const ModCtx* __restrict__ mod, ChaChaKey key,
                 u64 ctr) {
  const i64 nblk = (nT + 3) >> 2;
  const i64 k = (i64)blockIdx.x * TPB + threadIdx.x;
  if (k >= nblk) return;
  const int T = dp.T;
  const int cnt = nT - 4 * k < 4 ? (int)(nT - 4 * k) : 4;
  const i64 rows = B * dp.L;
  for (i64 row = blockIdx.y; row < rows; row += gridDim.y) {
    const i64 b = row / dp.L;
    const int j = (int)(row - b * dp.L);
    // g_j: digit kj of component tj (unrolled over the by-value digit counts: no runtime index into the parameters)
    int tj = 0, kj = j, acc = 0;
#pragma unroll
    for (int t = 0; t < PIPE_MAX_T; ++t) {
      if (t < T && j >= acc) { tj = t; kj = j - acc; }
      if (t < T) acc += dp.k[t];
    }
    const ModCtx mg = mod[tj];
    const u64 g = dp.base == 0 ? 1 : powmod_dev(rem128(0, (u64)dp.base, mg), kj, mg);
    u32 w[16];
    const u64 item = ctr + (u64)row;
    chacha20_block(key, (u32)k, (u32)CHACHA_DOM_HINT_UNIFORM, (u32)item, (u32)(item >> 32), w);
    const i64* e = e_crt + row * nT;
    const i64* v = vals + b * nT;
    i64* h0 = hints + row * 2 * nT;
    i64* h1 = h0 + nT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= cnt) continue;
      const i64 r = 4 * k + i;
      const u32 t = (u32)r % (u32)T;
      const ModCtx mc = mod[t];
      const u64 lo = (u64)w[4 * i] | (u64)w[4 * i + 1] << 32, hi = (u64)w[4 * i + 2] | (u64)w[4 * i + 3] << 32;
      const u64 u = reduce128(hi, lo, mc);
      u64 x = canon_in(e[r], mc.q);
      if ((int)t == tj) x = addmod(x, mulmod(g, canon_in(v[r], mc.q), mc), mc.q);
      h0[r] = (i64)submod(x, mulmod(u, canon_in(s_crt[r], mc.q), mc), mc.q);
      h1[r] = (i64)u;
    }
  }
}

hipError_t launch_kshint_combine(hipStream_t s, const i64* e_crt, const i64* vals, const i64* s_crt, i64* hints, i64 B,
                                 i64 n, const DecompParams& dp, const ModCtx* mod, const ChaChaKey& key, u64 ctr) {
  const i64 nT = n * dp.T, rows = B * dp.L;
  if (rows == 0 || nT == 0) return hipSuccess;
  if (dp.T < 1 || dp.T > PIPE_MAX_T) return hipErrorInvalidValue;
  unsigned x;
  if (!tiles_for((nT + 3) / 4, TPB, &x)) return hipErrorInvalidValue;
  const dim3 grid(x, (unsigned)(rows < (i64)MAX_GRID_Y ? rows : MAX_GRID_Y));
  hipLaunchKernelGGL(k_kshint_combine, grid, dim3(TPB), 0, s, e_crt, vals, s_crt, hints, B, nT, dp, mod, key, ctr);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// out[i][j][t] = (j == coeffs[i * n_lo]) for i < rel: the unit vector of the relative powerful-basis element i (the
// pairing of lolhip_coeffs_batch, Tensor.hs:472-477)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_unit_rows(i64* __restrict__ out, const int32_t* __restrict__ coeffs, i64 rel, i64 n, int T, i64 n_lo) {
  const i64 total = rel * n * T;
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
    const i64 i = g / (n * T), j = (g - i * n * T) / T;
    out[g] = j == (i64)coeffs[i * n_lo] ? 1 : 0;
  }
}

hipError_t launch_unit_rows(hipStream_t s, i64* out, const int32_t* coeffs, i64 rel, i64 n, int T, i64 n_lo) {
  const i64 total = rel * n * T;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_unit_rows, dim3(grid_stride_blocks(total, TPB, 2048)), dim3(TPB), 0, s, out, coeffs, rel, n, T,
                     n_lo);
  return hipGetLastError();
}

}  // namespace lolhip
