// lol_amd/csrc/challenge.hip — the kernels of a whole rlwe-challenges challenge (Generate.hs:105-218,
// Verify.hs:236-366): I instances of L samples in one launch, each instance against its own secret.  gfx950 only.
//
//   k_chall_uniform  k_rlwe_uniform (rlwe.hip) with the secret row of the item's instance: uniform a from the ChaCha20
//                    stream with a s_i, or added into reduce e
//   k_chall_as       k_rlwe_as with the secret row of the item's instance: a s_i or b - a s_i
//   k_chall_verdict  fails and worst per instance from the per-sample norms or mismatch counts
//
// Index arithmetic of the two grouped passes.  One WAVE owns one (item b, range of residues): the wave number goes
// through readfirstlane, so b, the instance i = b / L (one 32-bit scalar division per item; L is a run-time value) and
// the row bases of a, out and s_i live in scalar registers, and a lane adds its residue index only.  Four waves make
// a workgroup, so at the small indices of the challenges (n = 22 ... 256) a workgroup serves four items, which may
// belong to different instances.  Items stride over the grid's y dimension.  Where the row length n T is even and the
// slabs are 16-byte aligned, a lane moves two words per access.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "challenge.h"
#include "elementwise_dev.h"
#include "rlwe.h"
#include "rlwe_dev.h"
#include "rng_dev.h"

namespace lolhip {

namespace {
constexpr int WAVES = 4;                     // items per workgroup
constexpr unsigned MAX_GRID_Y = 65535;
constexpr u32 U_TILE = 64;                   // ChaCha20 blocks (of 4 residues) per wave and x tile (k_chall_uniform)
constexpr int AS_ITERS = 4;                  // k_chall_as: a wave covers AS_ITERS x 64 lanes x 2 residues per x tile
constexpr u32 AS_TILE = AS_ITERS * 128;

__device__ __forceinline__ u32 wave_id() { return (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ ModCtx mod_of(const ModCtx* __restrict__ mod, u32 r, int T) {
  return mod[T == 1 ? 0u : r % (u32)T];
}

// ---------------------------------------------------------------------------------------
// uniform a, 4 residues per ChaCha20 block: r = j*T + t -> (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q_t, the words of
// k_rlwe_uniform, and out = a s_i / out += a s_i
// ---------------------------------------------------------------------------------------
template <int MODE, bool VEC>
__global__ void __launch_bounds__(64 * WAVES)
k_chall_uniform(i64* __restrict__ a, const i64* __restrict__ s_crt, i64* __restrict__ out, u32 B, u32 L, u32 nT, int T,
                const ModCtx* __restrict__ mod, ChaChaKey key, u64 ctr, int domain) {
  const u32 nblk = (nT + 3) >> 2;
  const u32 k = blockIdx.x * U_TILE + (threadIdx.x & 63);
  if (k >= nblk) return;
  const u32 r0 = 4 * k;
  const int cnt = nT - r0 < 4 ? (int)(nT - r0) : 4;
  for (u32 b = blockIdx.y * WAVES + wave_id(); b < B; b += gridDim.y * WAVES) {
    const i64* __restrict__ srow = s_crt + (i64)(b / L) * nT;     // scalar: the secret of the item's instance
    i64* __restrict__ arow = a + (i64)b * nT;
    i64* __restrict__ orow = out + (i64)b * nT;
    u32 w[16];
    stream_block(key, ctr, domain, (i64)b, k, w);
    u64 u[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0}, ov[4] = {0, 0, 0, 0};
    const bool whole = VEC && cnt == 4;                          // VEC: nT is even and the slabs are 16-byte aligned
    if (whole) {
      const u64x2 s01 = *reinterpret_cast<const u64x2*>(srow + r0), s23 = *reinterpret_cast<const u64x2*>(srow + r0 + 2);
      sv[0] = s01.x; sv[1] = s01.y; sv[2] = s23.x; sv[3] = s23.y;
      if constexpr (MODE == RLWE_U_ADD) {
        const u64x2 o01 = *reinterpret_cast<const u64x2*>(orow + r0), o23 = *reinterpret_cast<const u64x2*>(orow + r0 + 2);
        ov[0] = o01.x; ov[1] = o01.y; ov[2] = o23.x; ov[3] = o23.y;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i >= cnt) continue;
        sv[i] = (u64)srow[r0 + i];
        if constexpr (MODE == RLWE_U_ADD) ov[i] = (u64)orow[r0 + i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= cnt) continue;
      const ModCtx mc = mod_of(mod, r0 + i, T);
      const u64 lo = (u64)w[4 * i] | (u64)w[4 * i + 1] << 32, hi = (u64)w[4 * i + 2] | (u64)w[4 * i + 3] << 32;
      u[i] = reduce128(hi, lo, mc);
      const u64 us = mulmod(u[i], canon_in((i64)sv[i], mc.q), mc);
      o[i] = MODE == RLWE_U_ADD ? addmod(canon_in((i64)ov[i], mc.q), us, mc.q) : us;
    }
    if (whole) {
      *reinterpret_cast<u64x2*>(arow + r0) = u64x2{u[0], u[1]};
      *reinterpret_cast<u64x2*>(arow + r0 + 2) = u64x2{u[2], u[3]};
      *reinterpret_cast<u64x2*>(orow + r0) = u64x2{o[0], o[1]};
      *reinterpret_cast<u64x2*>(orow + r0 + 2) = u64x2{o[2], o[3]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i >= cnt) continue;
        arow[r0 + i] = (i64)u[i];
        orow[r0 + i] = (i64)o[i];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// out = a s_i, or b - a s_i.  out may alias a or b: a lane reads its residues before it writes them.
// ---------------------------------------------------------------------------------------
template <bool SUB, bool VEC>
__global__ void __launch_bounds__(64 * WAVES)
k_chall_as(const i64* a, const i64* b_in, const i64* __restrict__ s_crt, i64* out, u32 B, u32 L, u32 nT, int T,
           const ModCtx* __restrict__ mod) {
  const u32 lane2 = (threadIdx.x & 63) * 2;
  for (u32 b = blockIdx.y * WAVES + wave_id(); b < B; b += gridDim.y * WAVES) {
    const i64* __restrict__ srow = s_crt + (i64)(b / L) * nT;     // scalar: the secret of the item's instance
    const i64 base = (i64)b * nT;
#pragma unroll
    for (int it = 0; it < AS_ITERS; ++it) {
      const u32 r = blockIdx.x * AS_TILE + (u32)it * 128u + lane2;
      if (r >= nT) break;
      if constexpr (VEC) {                                       // nT is even, so r + 1 < nT
        const u64x2 av = *reinterpret_cast<const u64x2*>(a + base + r);
        const u64x2 sv = *reinterpret_cast<const u64x2*>(srow + r);
        u64x2 bv = {0, 0};
        if constexpr (SUB) bv = *reinterpret_cast<const u64x2*>(b_in + base + r);
        const ModCtx m0 = mod_of(mod, r, T), m1 = mod_of(mod, r + 1, T);
        const u64 p0 = mulmod(canon_in((i64)av.x, m0.q), canon_in((i64)sv.x, m0.q), m0);
        const u64 p1 = mulmod(canon_in((i64)av.y, m1.q), canon_in((i64)sv.y, m1.q), m1);
        u64x2 res;
        res.x = SUB ? submod(canon_in((i64)bv.x, m0.q), p0, m0.q) : p0;
        res.y = SUB ? submod(canon_in((i64)bv.y, m1.q), p1, m1.q) : p1;
        *reinterpret_cast<u64x2*>(out + base + r) = res;
      } else {
#pragma unroll
        for (u32 e = 0; e < 2; ++e) {
          if (r + e >= nT) continue;
          const ModCtx mc = mod_of(mod, r + e, T);
          const u64 as = mulmod(canon_in(a[base + r + e], mc.q), canon_in(srow[r + e], mc.q), mc);
          out[base + r + e] = (i64)(SUB ? submod(canon_in(b_in[base + r + e], mc.q), as, mc.q) : as);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// The verdict: one wave owns one instance and reduces its L values; integers and a maximum, so the order of the
// shuffle tree is immaterial.  No atomics.
// ---------------------------------------------------------------------------------------
struct VerdictI64 {
  typedef i64 In; typedef i64 Worst;
  static __device__ __forceinline__ bool fail(i64 x, i64 bound) { return !(bound > x); }
};
struct VerdictF64 {
  typedef double In; typedef double Worst;
  static __device__ __forceinline__ bool fail(double x, double bound) { return !(bound > x); }
};
struct VerdictRlwr {
  typedef int32_t In; typedef i64 Worst;
  static __device__ __forceinline__ bool fail(int32_t x, int32_t) { return x != 0; }
};

template <typename K>
__global__ void __launch_bounds__(64)
k_chall_verdict(const typename K::In* __restrict__ v, typename K::In bound, int32_t* __restrict__ fails,
                typename K::Worst* __restrict__ worst, u32 I, u32 L) {
  typedef typename K::Worst W;
  const u32 lane = threadIdx.x;
  for (u32 i = blockIdx.x; i < I; i += gridDim.x) {
    const typename K::In* __restrict__ row = v + (i64)i * L;
    int f = 0, nan = 0;
    W w = std::numeric_limits<W>::lowest();
    for (u32 l = lane; l < L; l += 64) {
      const typename K::In x = row[l];
      f += K::fail(x, bound);
      if constexpr (std::numeric_limits<W>::has_quiet_NaN) nan |= !(x == x);
      if ((W)x > w) w = (W)x;
    }
    for (int off = 32; off > 0; off >>= 1) {
      f += __shfl_down(f, off, 64);
      nan |= __shfl_down(nan, off, 64);
      const W o = __shfl_down(w, off, 64);
      if (o > w) w = o;
    }
    if (lane == 0) {
      fails[i] = f;
      if constexpr (std::numeric_limits<W>::has_quiet_NaN) {
        worst[i] = nan ? std::numeric_limits<W>::quiet_NaN() : w;
      } else {
        worst[i] = w;
      }
    }
  }
}

bool dims_ok(i64 I, i64 L, i64 nT) {
  return I >= 0 && L >= 1 && nT >= 0 && nT <= 0x7fffffff && I <= CHALL_MAX_ITEMS / L;
}

dim3 item_grid(unsigned x, i64 B) {
  const i64 groups = (B + WAVES - 1) / WAVES;
  return dim3(x, (unsigned)(groups < (i64)MAX_GRID_Y ? groups : MAX_GRID_Y));
}

template <typename K>
hipError_t launch_verdict(hipStream_t s, const typename K::In* v, typename K::In bound, int32_t* fails,
                          typename K::Worst* worst, i64 I, i64 L) {
  if (!dims_ok(I, L, 0)) return hipErrorInvalidValue;
  if (I == 0) return hipSuccess;
  hipLaunchKernelGGL(k_chall_verdict<K>, dim3((unsigned)(I < 65536 ? I : 65536)), dim3(64), 0, s, v, bound, fails, worst,
                     (u32)I, (u32)L);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_chall_uniform(hipStream_t s, int mode, i64* a, const i64* s_crt, i64* out, i64 I, i64 L, i64 n, int T,
                                const ModCtx* mod, const ChaChaKey& key, u64 ctr, int domain) {
  if (T < 1 || n < 0 || n > 0x7fffffff / T || !dims_ok(I, L, n * T)) return hipErrorInvalidValue;
  if (mode != RLWE_U_PROD && mode != RLWE_U_ADD) return hipErrorInvalidValue;
  const i64 B = I * L, nT = n * T;
  if (B == 0 || nT == 0) return hipSuccess;
  unsigned x;
  if (!tiles_for((nT + 3) >> 2, U_TILE, &x)) return hipErrorInvalidValue;
  const dim3 grid = item_grid(x, B), block(64 * WAVES);
  const bool vec = nT % 2 == 0 && aligned16(a, s_crt, out);
#define LH_CHALL_U(MODE, VEC)                                                                                        \
  hipLaunchKernelGGL((k_chall_uniform<MODE, VEC>), grid, block, 0, s, a, s_crt, out, (u32)B, (u32)L, (u32)nT, T, mod, key, \
                     ctr, domain)
  if (mode == RLWE_U_PROD) { if (vec) LH_CHALL_U(RLWE_U_PROD, true); else LH_CHALL_U(RLWE_U_PROD, false); }
  else { if (vec) LH_CHALL_U(RLWE_U_ADD, true); else LH_CHALL_U(RLWE_U_ADD, false); }
#undef LH_CHALL_U
  return hipGetLastError();
}

hipError_t launch_chall_as(hipStream_t s, const i64* a, const i64* b, const i64* s_crt, i64* out, i64 I, i64 L, i64 n,
                           int T, const ModCtx* mod) {
  if (T < 1 || n < 0 || n > 0x7fffffff / T || !dims_ok(I, L, n * T)) return hipErrorInvalidValue;
  const i64 B = I * L, nT = n * T;
  if (B == 0 || nT == 0) return hipSuccess;
  unsigned x;
  if (!tiles_for(nT, AS_TILE, &x)) return hipErrorInvalidValue;
  const dim3 grid = item_grid(x, B), block(64 * WAVES);
  const bool vec = nT % 2 == 0 && aligned16(a, b, s_crt, out);
#define LH_CHALL_AS(SUB, VEC) \
  hipLaunchKernelGGL((k_chall_as<SUB, VEC>), grid, block, 0, s, a, b, s_crt, out, (u32)B, (u32)L, (u32)nT, T, mod)
  if (b) { if (vec) LH_CHALL_AS(true, true); else LH_CHALL_AS(true, false); }
  else { if (vec) LH_CHALL_AS(false, true); else LH_CHALL_AS(false, false); }
#undef LH_CHALL_AS
  return hipGetLastError();
}

hipError_t launch_chall_verdict_i64(hipStream_t s, const i64* norm, i64 bound, int32_t* fails, i64* worst, i64 I, i64 L) {
  return launch_verdict<VerdictI64>(s, norm, bound, fails, worst, I, L);
}
hipError_t launch_chall_verdict_f64(hipStream_t s, const double* norm, double bound, int32_t* fails, double* worst, i64 I,
                                    i64 L) {
  return launch_verdict<VerdictF64>(s, norm, bound, fails, worst, I, L);
}
hipError_t launch_chall_verdict_rlwr(hipStream_t s, const int32_t* mismatch, int32_t* fails, i64* worst, i64 I, i64 L) {
  return launch_verdict<VerdictRlwr>(s, mismatch, 0, fails, worst, I, L);
}

}  // namespace lolhip
