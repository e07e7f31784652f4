// lol_amd/csrc/gadget.hip — the third class of the reference's Gadget module on the device: Correct, the LWE inversion
// of the gadget trapdoor, and Gadget.encode plus noise, which makes its inputs.  gfx950 only; both are element-wise
// passes over the [L][B][n][T] digit-slab layout k_decompose (pipeline.hip) writes, one thread per row (coefficient).
//
//   k_gadget_correct  (u, es) from L noisy gadget multiples, decoding basis   Cyc.hs:615-621, Gadget.hs:84-134,
//                                                                             ZqBasic.hs:234-314
//   k_gadget_encode   g_j s + reduce (e_j)                                    Gadget.hs:47-56, ZqBasic.hs:247-255
//
// The algorithm, its domain and the proof that inside it no value leaves 64 bits: DESIGN.md 3.4j.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "gadget.h"

namespace lolhip {

constexpr int EPT = 2;                       // rows per thread, as pipeline.hip
constexpr i64 TILE = 256 * EPT;

// floor((x1:x0) / c.q) for (x1:x0) < q 2^64: the quotient of the division step whose remainder is rem128 (zq_dev.h)
__device__ __forceinline__ u64 quot128(u64 x1, u64 x0, const ModCtx& c) {
  const u64 u1 = (x1 << c.s) | (x0 >> (64 - c.s));
  const u64 u0 = x0 << c.s;
  const u128 qq = (u128)c.v * u1 + (((u128)u1 << 64) | u0);
  u64 q1 = (u64)(qq >> 64) + 1;
  const u64 q0 = (u64)qq;
  u64 r = u0 - q1 * c.d;
  if (r > q0) { --q1; r += c.d; }
  if (r >= c.d) ++q1;
  return q1;
}

// floor(a / q) of a signed 128-bit numerator, |a| < q 2^64
__device__ __forceinline__ i64 floor_div_q(__int128 a, const ModCtx& c) {
  const bool neg = a < 0;
  const u128 m = neg ? ~(u128)a : (u128)a;                    // -a - 1
  const u64 quo = quot128((u64)(m >> 64), (u64)m, c);
  return neg ? -(i64)quo - 1 : (i64)quo;
}

// x mod q of any int64; a canonical residue, the usual input, costs one compare
__device__ __forceinline__ u64 residue(i64 x, const ModCtx& mc) { return (u64)x < mc.q ? (u64)x : mod_any(x, mc); }

// One thread per row.  Component t corrects its own block of k = p.d.k[t] entries over q = q_t.  With v_i the centred
// lifts, w_i = divModCent (b v_i - v_(i+1), q) and z_i = q sum_{j<i} b^(i-1-j) w_j (z_0 = 0, z_(i+1) = b z_i + q w_i),
// the reference's y_i is b^i x - z_i, so  e_i = (v_i + z_i) - b^i c  with  c = x + s: ONE sweep over the entries yields
// x, every t_i = v_i + z_i and, at its end, s and c.  u' = xs_0 - e_0 = c mod q needs nothing else; the errors are
// stored as t_i during the sweep and get their - b^i c in a second sweep over the thread's own stores (k up to 61
// values cannot stay in registers).  All sums are taken mod 2^64: inside the domain gadget_api.cpp admits, every true
// value fits int64, so the wrapped value is the true one.  In a pair the entry is q_o^-1 (own - lift other) and the
// error xo + q_o e': the same two sweeps, scaled by q_o.
// V2: T = 2 and 16-byte aligned xs and u: a row's pair is one 16-byte access.
template <bool V2>
__global__ void __launch_bounds__(256)
k_gadget_correct(const i64* __restrict__ xs, i64* __restrict__ u, i64* es, i64 rows, CorrectParams p,
                 const ModCtx* __restrict__ mod) {
  const int T = V2 ? 2 : p.d.T;
  const i64 b = p.d.base;
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const i64 r = s0 + (u32)e * 256u + threadIdx.x;
    if (r >= rows) continue;
    i64 j0 = 0;                                               // first entry of the block
    u64x2 uw; uw.x = 0; uw.y = 0;
    for (int t = 0; t < T; ++t) {
      const ModCtx mc = mod[t];
      const ModCtx mo = mod[T == 2 ? 1 - t : t];
      const int k = p.d.k[t];
      const u64 q = mc.q, qo = p.qo[t];
      const i64 h = (i64)(q >> 1);
      // entry i of the block: the centred lift of what is corrected over q, and xo, the part of its error read off
      // the other component (0 for a single modulus)
      auto entry = [&](int i, i64& xo) -> i64 {
        const i64* src = xs + ((j0 + i) * rows + r) * T;
        if (T != 2) { xo = 0; return centred(residue(src[0], mc), q); }
        i64 own, other;
        if constexpr (V2) {
          const u64x2 w = *reinterpret_cast<const u64x2*>(src);
          own = (i64)(t == 0 ? w.x : w.y);
          other = (i64)(t == 0 ? w.y : w.x);
        } else {
          own = src[t];
          other = src[1 - t];
        }
        xo = centred(residue(other, mo), mo.q);
        return centred(mulmod(submod(residue(own, mc), residue(xo, mc), q), p.qo_inv[t], mc), q);
      };
      u64 z = 0, x = 0, qd = q;
      i64 xo, v = entry(0, xo);
      for (int i = 0; i + 1 < k; ++i) {
        i64 xon;
        const i64 vn = entry(i + 1, xon);
        qd = (u64)floor_div_inv((i64)qd, p.d.magic, p.d.sh1, p.d.sh2);         // floor(q / b^(i+1))
        const i64 w = floor_div_q((__int128)b * v - vn + h, mc);               // |numerator| <= (b + 2) h
        if (es) es[(j0 + i) * rows + r] = (i64)((u64)xo + qo * ((u64)v + z));
        x += (u64)w * qd;
        z = (u64)b * z + q * (u64)w;
        v = vn;
        xo = xon;
      }
      const u64 tl = (u64)v + z, g = p.g[t];
      const i64 vl = (i64)(tl - g * x);                                        // v'_(k-1)
      const i64 s = floor_div_inv(vl + (i64)(g >> 1), p.gmagic[t], p.gsh1[t], p.gsh2[t]);
      const u64 c = x + (u64)s;
      if (es) {
        es[(j0 + k - 1) * rows + r] = (i64)((u64)xo + qo * (tl - g * c));
        u64 f = qo * c;                                                        // q_o b^i c
        for (int i = 0; i + 1 < k; ++i) {
          i64* o = es + (j0 + i) * rows + r;
          *o = (i64)((u64)*o - f);
          f *= (u64)b;
        }
      }
      const u64 up = mod_any((i64)c, mc);
      const u64 ut = T == 2 ? mulmod(up, p.qo_mod[t], mc) : up;
      if constexpr (V2) { if (t == 0) uw.x = ut; else uw.y = ut; }
      else u[r * T + t] = (i64)ut;
      j0 += k;
    }
    if constexpr (V2) *reinterpret_cast<u64x2*>(u + r * 2) = uw;
  }
}

hipError_t launch_gadget_correct(hipStream_t s, const i64* xs, i64* u, i64* es, i64 rows, const CorrectParams& p,
                                 const ModCtx* mod) {
  if (rows == 0) return hipSuccess;
  if (p.d.T < 1 || p.d.T > GADGET_MAX_T) return hipErrorInvalidValue;
  unsigned blocks;
  if (!tiles_for(rows, TILE, &blocks)) return hipErrorInvalidValue;
  if (p.d.T == 2 && aligned16(xs, u))
    hipLaunchKernelGGL((k_gadget_correct<true>), dim3(blocks), dim3(256), 0, s, xs, u, es, rows, p, mod);
  else
    hipLaunchKernelGGL((k_gadget_correct<false>), dim3(blocks), dim3(256), 0, s, xs, u, es, rows, p, mod);
  return hipGetLastError();
}

// out_j = g_j s + reduce (e_j): entry j of component t's block is b^i s_t + e_j in component t and e_j alone in the
// others, each row's T words one chunk.  V2 as above, over out.
template <bool V2>
__global__ void __launch_bounds__(256)
k_gadget_encode(const i64* __restrict__ sv, const i64* __restrict__ e, i64* __restrict__ out, i64 rows, DecompParams p,
                const ModCtx* __restrict__ mod) {
  const int T = V2 ? 2 : p.T;
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
#pragma unroll
  for (int ee = 0; ee < EPT; ++ee) {
    const i64 r = s0 + (u32)ee * 256u + threadIdx.x;
    if (r >= rows) continue;
    i64 j = 0;
    for (int t = 0; t < T; ++t) {
      const ModCtx mc = mod[t];
      const u64 bq = mod_any(p.base, mc);
      u64 gs = residue(sv[r * T + t], mc);                    // b^i s mod q_t
      for (int i = 0; i < p.k[t]; ++i, ++j) {
        const i64 ej = e ? e[j * rows + r] : 0;
        i64* o = out + (j * rows + r) * T;
        if constexpr (V2) {
          u64x2 w;
          w.x = mod_any(ej, mod[0]);
          w.y = mod_any(ej, mod[1]);
          if (t == 0) w.x = addmod(w.x, gs, mc.q); else w.y = addmod(w.y, gs, mc.q);
          *reinterpret_cast<u64x2*>(o) = w;
        } else {
          for (int s = 0; s < T; ++s) {
            const u64 red = mod_any(ej, mod[s]);
            o[s] = (i64)(s == t ? addmod(red, gs, mc.q) : red);
          }
        }
        gs = mulmod(gs, bq, mc);
      }
    }
  }
}

hipError_t launch_gadget_encode(hipStream_t s, const i64* sv, const i64* e, i64* out, i64 rows, const DecompParams& p,
                                const ModCtx* mod) {
  if (rows == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(rows, TILE, &blocks)) return hipErrorInvalidValue;
  if (p.T == 2 && aligned16(out))
    hipLaunchKernelGGL((k_gadget_encode<true>), dim3(blocks), dim3(256), 0, s, sv, e, out, rows, p, mod);
  else
    hipLaunchKernelGGL((k_gadget_encode<false>), dim3(blocks), dim3(256), 0, s, sv, e, out, rows, p, mod);
  return hipGetLastError();
}

}  // namespace lolhip
