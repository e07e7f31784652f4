// lol_amd/csrc/rlwe_dev.h — the per-element device arithmetic the samplers and the RLWE / RLWR passes share
// (encrypt.hip, rlwe.hip, rlwe_ring.hip): the ChaCha20 stream's block of a batch item, Box-Muller on its words, the
// K/(qR) operations of RRq.hs:47-84 and the RLWR rounding.  One definition, so a fused pass gives the bits of the
// passes it replaces.  Included by .hip files only.
#pragma once
#include "rng_dev.h"
#include "zq_dev.h"

namespace lolhip {

// the block of item b: nonce (domain, lo32(ctr + b), hi32(ctr + b)), block counter k
__device__ __forceinline__ void stream_block(const ChaChaKey& key, u64 ctr, int domain, i64 b, u32 k, u32 w[16]) {
  const u64 nb = ctr + (u64)b;
  chacha20_block(key, k, (u32)domain, (u32)nb, (u32)(nb >> 32), w);
}

// basic Box-Muller on words w[0..3]: u1 = ((a >> 11) + 1) 2^-53 in (0, 1], u2 = (c >> 11) 2^-53
__device__ __forceinline__ void box_muller(const u32* w, double sigma, double* g0, double* g1) {
  const u64 a = (u64)w[0] | (u64)w[1] << 32, c = (u64)w[2] | (u64)w[3] << 32;
  const double u1 = (double)((a >> 11) + 1) * 0x1p-53;
  const double u2 = (double)(c >> 11) * 0x1p-53;
  const double r = sigma * sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  *g0 = r * cs;
  *g1 = r * sn;
}

// the 8 Gaussians of block k (coefficients 8k .. 8k+7)
__device__ __forceinline__ void gauss8(const ChaChaKey& key, u64 ctr, int domain, i64 b, u32 k, double sigma,
                                       double g[8]) {
  u32 w[16];
  stream_block(key, ctr, domain, b, k, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) box_muller(w + 4 * i, sigma, &g[2 * i], &g[2 * i + 1]);
}

// ---------------------------------------------------------------------------------------
// RRq (RRq.hs:47-84): reduce' x = x - q floor(x / q); x + y with one conditional subtraction; lift y = y + y < q ? y :
// y - q.  Every IEEE operation rounded on its own (no contraction), whatever the including unit compiles with.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double rrq_reduce(double x, double q) {
#pragma clang fp contract(off)
  return x - q * floor(x / q);
}
__device__ __forceinline__ double rrq_add(double x, double y, double q) {
#pragma clang fp contract(off)
  const double z = x + y;
  return z >= q ? z - q : z;
}
__device__ __forceinline__ double rrq_lift(double y, double q) {
#pragma clang fp contract(off)
  return y + y < q ? y : y - q;
}

// ---------------------------------------------------------------------------------------
// RLWR: l = the centred lift of x (decode', ZqBasic.hs:92-94), r = floor((p l + floor(q/2)) / q) mod p (roundedProd:
// rescaleMod, Prelude.hs:144-153 over divModCent, Numeric.hs:227-234), exact: the 64-bit division where p |l| + q/2
// fits it, else the 128-bit one.  x in [0, q), 2 <= p < q < 2^62.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ i64 rlwr_round(u64 x, u64 q, u64 p) {
  const bool neg = 2 * x >= q;
  const u64 al = neg ? q - x : x;                              // |l| <= q/2
  const u64 h = q >> 1;
  const u128 pl = (u128)p * al;
  i64 quo;                                                     // floor((+-pl + h) / q), |quo| <= p/2 + 1
  if (!neg) {
    const u128 num = pl + h;
    quo = (num >> 64) == 0 ? (i64)((u64)num / q) : (i64)(u64)(num / q);
  } else if (pl <= h) {
    quo = 0;                                                   // 0 <= h - pl < q
  } else {
    const u128 num = pl - h + (q - 1);                         // -ceil((pl - h) / q)
    quo = (num >> 64) == 0 ? -(i64)((u64)num / q) : -(i64)(u64)(num / q);
  }
  i64 r = quo % (i64)p;
  return r < 0 ? r + (i64)p : r;
}

}  // namespace lolhip
