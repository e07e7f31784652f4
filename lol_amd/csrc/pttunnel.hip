// lol_amd/csrc/pttunnel.hip — the element-wise passes of the clear-text tunnel (ptTunnel, lol-apps HomomPRF.hs:510-531)
// and of crtSet's powering (lol UCyc.hs:540-565) over a plaintext modulus p^e that has no CRT basis: every ring product
// runs exactly over the integers mod an NTT prime Q (the existing crt / crtInv / poly-mul), and k_relift is the one
// pass in between: centred lift mod Q, reduction mod p^e, the residues out and / or their centred lift into the next
// prime.  HBM-bound: 8 bytes in, 8 or 16 bytes out per word, 16-byte accesses per lane when every slab is aligned.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "pttunnel.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;
constexpr i64 MAX_BLOCKS = 1 << 16;     // grid-stride above: 256 CUs x 8 waves are covered many times over

unsigned grid_for(i64 total) { return grid_stride_blocks(total, TPB, MAX_BLOCKS); }

template <bool FROMQ, bool POW2>
__device__ __forceinline__ u64 relift_res(i64 x, const Relift& c) {
  i64 v = x;
  if constexpr (FROMQ) v = centred(canon_in(x, c.Qin), c.Qin);
  if constexpr (POW2) return (u64)v & (c.pe.q - 1);
  return mod_any(v, c.pe);
}

__device__ __forceinline__ i64 relift_lift(u64 r, const Relift& c) {
  return 2 * r >= c.pe.q ? (i64)(r + c.Qout - c.pe.q) : (i64)r;
}

template <bool FROMQ, bool POW2, bool V2>
__global__ void __launch_bounds__(TPB)
k_relift(const i64* src, i64* res, i64* lift, i64 total, Relift c) {
  if constexpr (V2) {
    const i64 pairs = total >> 1;
    for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < pairs; g += (i64)gridDim.x * TPB) {
      const longlong2 a = reinterpret_cast<const longlong2*>(src)[g];
      const u64 r0 = relift_res<FROMQ, POW2>(a.x, c), r1 = relift_res<FROMQ, POW2>(a.y, c);
      if (res) reinterpret_cast<longlong2*>(res)[g] = longlong2{(i64)r0, (i64)r1};
      if (lift) reinterpret_cast<longlong2*>(lift)[g] = longlong2{relift_lift(r0, c), relift_lift(r1, c)};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (total & 1)) {
      const u64 r = relift_res<FROMQ, POW2>(src[total - 1], c);
      if (res) res[total - 1] = (i64)r;
      if (lift) lift[total - 1] = relift_lift(r, c);
    }
  } else {                                                      // a slab that is not 16-byte aligned: 8-byte accesses
    for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
      const u64 r = relift_res<FROMQ, POW2>(src[g], c);
      if (res) res[g] = (i64)r;
      if (lift) lift[g] = relift_lift(r, c);
    }
  }
}

__global__ void __launch_bounds__(TPB)
k_embed_rows(const i64* in, i64* out, const int32_t* idx, i64 rows, i64 n_in, i64 n_out) {
  const i64 total = rows * n_out;
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
    const i64 r = g / n_out;
    const int32_t src = idx[g - r * n_out];
    out[g] = src < 0 ? 0 : in[r * n_in + src];
  }
}
}  // namespace

hipError_t launch_relift(hipStream_t s, const i64* src, i64* res, i64* lift, i64 total, const Relift& c) {
  if (total == 0) return hipSuccess;
  if (total < 0 || !src || (!res && !lift) || c.pe.q < 2 || (lift && c.Qout < c.pe.q)) return hipErrorInvalidValue;
  const bool v2 = aligned16(src, res, lift);
  const unsigned grid = grid_for(v2 ? (total + 1) >> 1 : total);
  const bool fromq = c.Qin != 0, pow2 = c.pebits != 0;
#define LOLHIP_RELIFT(F, P)                                                                                     \
  do {                                                                                                           \
    if (v2) hipLaunchKernelGGL((k_relift<F, P, true>), dim3(grid), dim3(TPB), 0, s, src, res, lift, total, c);   \
    else hipLaunchKernelGGL((k_relift<F, P, false>), dim3(grid), dim3(TPB), 0, s, src, res, lift, total, c);     \
  } while (0)
  if (fromq && pow2) LOLHIP_RELIFT(true, true);
  else if (fromq) LOLHIP_RELIFT(true, false);
  else if (pow2) LOLHIP_RELIFT(false, true);
  else LOLHIP_RELIFT(false, false);
#undef LOLHIP_RELIFT
  return hipGetLastError();
}

hipError_t launch_embed_rows(hipStream_t s, const i64* in, i64* out, const int32_t* idx, i64 rows, i64 n_in, i64 n_out) {
  if (rows * n_out == 0) return hipSuccess;
  if (rows < 0 || !in || !out || !idx || n_in < 1 || n_out < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed_rows, dim3(grid_for(rows * n_out)), dim3(TPB), 0, s, in, out, idx, rows, n_in, n_out);
  return hipGetLastError();
}

}  // namespace lolhip
