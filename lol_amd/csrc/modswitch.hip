// lol_amd/csrc/modswitch.hip — k_modswitch: the coefficient-wise part of a ciphertext's modSwitch (lol-apps
// SymmSHE.hs:236-246) as ONE streaming pass, gfx950 only.  Per coefficient row (all T residues in registers):
//
//   scale   c_t <- s_t c_t                       toMSD's p^-1 mod q_t (ZqBasic.hs:132-137), folded in
//   down    for i < d:  z = lift c_i;  c_s <- q_i^-1 (c_s - z) mod q_s, s > i      Prelude.hs:227-232, iterated
//   up      u zero components in front, c_s <- (prod of the new moduli) c_s        Prelude.hs:274-286, iterated
//                                                                                  (the product rides in s_t)
//
// The composition this replaces reads the row once per dropped modulus (k_rescale) after a scaling pass of its own;
// here every word is read once and every result written once: (T + T') 8 bytes per coefficient.  A workgroup owns
// one tile of consecutive rows, takes its start once in 64 bits and walks its rows in 32 bits (k_ctmul, k_rescale).
// The constants travel by value in the kernel arguments (wave-uniform: they stay in SGPRs).  No LDS.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "modswitch.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;                     // one row per thread: a tile is TPB rows
}  // namespace

// SH = d - u: D = SH leading components dropped or U = -SH zero components added.  VIN / VOUT: the rows of the input /
// output are whole 16-byte pairs (T / To even, 16-byte aligned slabs).
template <int SH, bool VIN, bool VOUT>
__global__ void __launch_bounds__(TPB)
k_modswitch(const i64* __restrict__ in0, i64 rows0, const i64* __restrict__ in, i64* __restrict__ out, i64 rows,
            ModSwitchParams p) {
  constexpr int D = SH > 0 ? SH : 0, U = SH < 0 ? -SH : 0;
  const int T = p.T, To = T - SH;
  const i64 s0 = (i64)blockIdx.x * TPB;                       // wave-uniform
  const i64* tile0 = in0 + s0 * T;
  const i64* tile1 = in + s0 * T;
  i64* otile = out + s0 * To;
  const u32 l = threadIdx.x;
  const i64 g = s0 + l;
  if (g >= rows) return;
  const i64* src = (g < rows0 ? tile0 : tile1) + l * (u32)T;
  u64 c[PIPE_MAX_T];
  if constexpr (VIN) {
#pragma unroll
    for (int t = 0; t < PIPE_MAX_T; t += 2)
      if (t < T) {
        const longlong2 v = *reinterpret_cast<const longlong2*>(src + t);
        c[t] = (u64)v.x; c[t + 1] = (u64)v.y;
      }
  } else {
#pragma unroll
    for (int t = 0; t < PIPE_MAX_T; ++t)
      if (t < T) c[t] = (u64)src[t];
  }
#pragma unroll
  for (int t = 0; t < PIPE_MAX_T; ++t)
    if (t < T) {
      const u64 q = p.q[t];
      u64 x = canon_in((i64)c[t], q);
      if (p.scaled) x = trim(shoup_lazy(x, p.s[t], p.sp[t], q), q);
      c[t] = x;
    }
  // one reference step per dropped modulus.  With y = c_s + (q_i - a) > 0:  c_s - lift a = y for the negative
  // lifts (a - q_i) and y - q_i for the others, and q_i^-1 q_i = 1 mod q_s: one Shoup product, then minus one
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const u64 qi = p.q[i], a = c[i];
    const bool pos = 2 * a < qi;                            // lift a = a, else a - q_i (the tie q_i / 2 goes down)
    const u64 y0 = qi - a;
#pragma unroll
    for (int s = i + 1; s < PIPE_MAX_T; ++s)
      if (s < T) {
        const u64 q = p.q[s];
        u64 r = trim(shoup_lazy(c[s] + y0, p.inv[i][s], p.invp[i][s], q), q);
        if (pos) r = r == 0 ? q - 1 : r - 1;
        c[s] = r;
      }
  }
  i64* dst = otile + l * (u32)To;
  auto o = [&](int j) -> u64 { return j < U ? 0 : c[j < U ? 0 : j - U + D]; };    // j, U, D constant after unrolling
  if constexpr (VOUT) {
#pragma unroll
    for (int j = 0; j + 1 < PIPE_MAX_T - D + U && j < PIPE_MAX_T; j += 2)
      if (j < To) {
        u64x2 v; v.x = o(j); v.y = o(j + 1);
        *reinterpret_cast<u64x2*>(dst + j) = v;
      }
  } else {
#pragma unroll
    for (int j = 0; j < PIPE_MAX_T - D + U && j < PIPE_MAX_T; ++j)
      if (j < To) dst[j] = (i64)o(j);
  }
}

hipError_t launch_modswitch(hipStream_t s, const i64* in0, i64 rows0, const i64* in, i64* out, i64 rows,
                            const ModSwitchParams& p) {
  if (rows == 0) return hipSuccess;
  const int To = p.T - p.d + p.u;
  if (p.T < 1 || p.T > PIPE_MAX_T || p.d < 0 || p.d > MODSW_MAX_D || p.u < 0 || p.u > MODSW_MAX_D || (p.d && p.u) ||
      To < 1 || To > PIPE_MAX_T || rows0 < 0 || rows0 > rows)
    return hipErrorInvalidValue;
  unsigned blocks;
  if (!tiles_for(rows, TPB, &blocks)) return hipErrorInvalidValue;
  const bool vin = (p.T & 1) == 0 && aligned16(in0, in);
  const bool vout = (To & 1) == 0 && aligned16(out);
  const dim3 grid(blocks), block(TPB);
#define LOLHIP_MS(SS)                                                                                             \
  case SS:                                                                                                        \
    if (vin) { if (vout) hipLaunchKernelGGL((k_modswitch<SS, true, true>), grid, block, 0, s, in0, rows0, in, out, rows, p);   \
               else hipLaunchKernelGGL((k_modswitch<SS, true, false>), grid, block, 0, s, in0, rows0, in, out, rows, p); }     \
    else { if (vout) hipLaunchKernelGGL((k_modswitch<SS, false, true>), grid, block, 0, s, in0, rows0, in, out, rows, p);      \
           else hipLaunchKernelGGL((k_modswitch<SS, false, false>), grid, block, 0, s, in0, rows0, in, out, rows, p); }        \
    break;
  switch (p.d - p.u) {
    LOLHIP_MS(-5) LOLHIP_MS(-4) LOLHIP_MS(-3) LOLHIP_MS(-2) LOLHIP_MS(-1) LOLHIP_MS(0)
    LOLHIP_MS(1) LOLHIP_MS(2) LOLHIP_MS(3) LOLHIP_MS(4) LOLHIP_MS(5)
    default: return hipErrorInvalidValue;
  }
#undef LOLHIP_MS
  return hipGetLastError();
}

}  // namespace lolhip
