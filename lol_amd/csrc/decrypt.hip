// lol_amd/csrc/decrypt.hip — the two kernels of SymmSHE errorTerm / decrypt (lol-apps SymmSHE.hs:153-178) that
// no Tensor member provides.  gfx950 only.
//
//   k_sk_eval  sum_i c_i s^i pointwise in the CRT basis (Horner), s broadcast over the batch    SymmSHE.hs:155-157
//   k_lift     the centred lift from Z_q0 x ... x Z_q(T-1) to the integers of every decoding-basis
//              coefficient (Lift' (a,b), Prelude.hs:165-180, nested; decode', ZqBasic.hs:92-94),
//              then either reduce mod p and scale by l' (decrypt) or the int64 value (errorTerm)
//   k_addmod   y += a componentwise (c_0 joins the other components before lInv)
//
// k_lift works in mixed radix (Garner): with P_i = q_0 ... q_(i-1), the lift X in [0, Q) is
// sum_i v_i P_i with digits v_i in [0, q_i), and
//     v_i = (x_i - sum_{j<i} v_j P_j) * P_i^-1   mod q_i
// where the inner sum is a Horner chain over the constants q_j mod q_i: i rem128 steps for digit i, O(T^2) per
// coefficient, no wide integers.  X is negative as a centred value iff X > floor((Q-1)/2), which a most-significant
// first comparison of the digits decides (garner_digits and above_half, elementwise_dev.h).  The constants that do
// not depend on p live in the plan (plan.h lift_consts); the p-dependent ones travel by value in LiftParams.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "pipeline.h"

namespace lolhip {

namespace {
constexpr int EPT = 2;                       // elements per thread (k_sk_eval, k_addmod)
constexpr i64 TILE = 256 * EPT;
}  // namespace

// ---------------------------------------------------------------------------------------
// sk_eval: out = (sum_k comp_k s^k) * (times_s ? s : 1), every slab [B][n][T] in the CRT basis.
// comp_k = comps + k * total.  out may alias comps (each element reads all of its inputs first).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_sk_eval(const i64* comps, int ncomp, int times_s, const i64* __restrict__ s_crt, i64* out, i64 total, u32 per, int T,
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
    const u64 sv = canon_in(s_crt[r], mc.q);
    u64 acc = canon_in(comps[(i64)(ncomp - 1) * total + g], mc.q);
    for (int k = ncomp - 2; k >= 0; --k) {
      const u128 t = (u128)acc * sv + canon_in(comps[(i64)k * total + g], mc.q);     // < q^2 + q < q 2^64
      acc = rem128((u64)(t >> 64), (u64)t, mc);
    }
    if (times_s) acc = mulmod(acc, sv, mc);
    out[g] = (i64)acc;
  }
}

hipError_t launch_sk_eval(hipStream_t s, const i64* comps, int ncomp, bool times_s, const i64* s_crt, i64* out, i64 B,
                          i64 n, int T, const ModCtx* mod) {
  const i64 total = B * n * T;
  if (total == 0) return hipSuccess;
  if (ncomp < 1) return hipErrorInvalidValue;
  unsigned blocks;
  if (!tiles_for(total, TILE, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sk_eval, dim3(blocks), dim3(256), 0, s, comps, ncomp, times_s ? 1 : 0, s_crt, out, total,
                     (u32)(n * T), T, mod);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// addmod: y = y + a, [B][n][T]
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_addmod(i64* y, const i64* a, i64 total, int T, const ModCtx* __restrict__ mod) {
  const i64 s0 = (i64)blockIdx.x * TILE;                      // wave-uniform
  const u32 t_s = (u32)((u64)s0 % (u32)T);
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const u32 l = (u32)e * 256u + threadIdx.x;
    const i64 g = s0 + l;
    if (g >= total) continue;
    const u64 q = mod[(t_s + l) % (u32)T].q;
    y[g] = (i64)addmod(canon_in(y[g], q), canon_in(a[g], q), q);
  }
}

hipError_t launch_addmod(hipStream_t s, i64* y, const i64* a, i64 B, i64 n, int T, const ModCtx* mod) {
  const i64 total = B * n * T;
  if (total == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(total, TILE, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_addmod, dim3(blocks), dim3(256), 0, s, y, a, total, T, mod);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// lift: one thread per coefficient (row of T residues), one int64 out.  NT = T at compile time, so the digit
// array stays in registers for every T up to PIPE_MAX_T.
//   PMODE: out = l' * (X mod p - [X negative] * (Q mod p))  mod p        (reduce . lift, then scalarCyc l)
//   else:  out = the centred lift as int64, INT64_MIN when |lift| >= 2^63
// in (and add, when given) [rows][NT]; the residue lifted is scale_t * (in + add) when p.msd.
// ---------------------------------------------------------------------------------------
constexpr int LIFT_TILE = 256;

template <int NT, bool PMODE>
__global__ void __launch_bounds__(256)
k_lift(const i64* __restrict__ in, const i64* __restrict__ add, i64* __restrict__ out, i64 rows, LiftParams p,
       const u64* __restrict__ lc, const ModCtx* __restrict__ mod) {
  const u64* pinv = lc;                       // plan.h lift_consts
  const u64* qmod = lc + NT;
  const u64* half = lc + NT + NT * NT;
  const i64 r = (i64)blockIdx.x * LIFT_TILE + threadIdx.x;
  if (r >= rows) return;
  u64 v[NT];
  garner_digits<NT>(v, [&](int i) {
    const ModCtx mc = mod[i];
    u64 x = canon_in(in[r * NT + i], mc.q);
    if (add) x = addmod(x, canon_in(add[r * NT + i], mc.q), mc.q);
    if (p.msd) x = mulmod(x, p.scale[i], mc);
    return x;
  }, mod, pinv, qmod, NT);
  const bool neg = above_half<NT>(v, half);
  if constexpr (PMODE) {
    u128 acc = 0;                             // sum v_i (P_i mod p): 16 terms below 2^124 each
#pragma unroll
    for (int i = 0; i < NT; ++i) acc += (u128)v[i] * p.pw[i];
    u64 x = reduce128((u64)(acc >> 64), (u64)acc, p.mp);
    if (neg) x = submod(x, p.qp, p.mp.q);
    out[r] = (i64)mulmod(x, p.lp, p.mp);
  } else {
    // |X| (or Q - X = sum (q_i - 1 - v_i) P_i + 1 for a negative value), folded from the top with overflow detection
    u64 x = 0;
    bool ovf = false;
#pragma unroll
    for (int i = NT - 1; i >= 0; --i) {
      const u64 q = mod[i].q;
      const u64 d = neg ? q - 1 - v[i] : v[i];
      const u128 t = (u128)x * q + d;                          // x < 2^63, q < 2^62
      ovf |= (t >> 63) != 0;
      x = (u64)t & (~0ull >> 1);
    }
    if (neg) {
      x += 1;
      ovf |= (x >> 63) != 0;
    }
    out[r] = ovf ? INT64_MIN : (neg ? -(i64)x : (i64)x);
  }
}

hipError_t launch_lift(hipStream_t s, const i64* in, const i64* add, i64* out, i64 rows, const LiftParams& p, bool pmode,
                       const u64* lift_consts, const ModCtx* mod) {
  if (rows == 0) return hipSuccess;
  unsigned blocks;
  if (!tiles_for(rows, LIFT_TILE, &blocks)) return hipErrorInvalidValue;
  const dim3 grid(blocks), block(256);
#define LOLHIP_LIFT(N)                                                                                          \
  case N:                                                                                                     \
    if (pmode) hipLaunchKernelGGL((k_lift<N, true>), grid, block, 0, s, in, add, out, rows, p, lift_consts, mod); \
    else hipLaunchKernelGGL((k_lift<N, false>), grid, block, 0, s, in, add, out, rows, p, lift_consts, mod);     \
    break;
  switch (p.T) {
    LOLHIP_LIFT(1) LOLHIP_LIFT(2) LOLHIP_LIFT(3) LOLHIP_LIFT(4) LOLHIP_LIFT(5) LOLHIP_LIFT(6) LOLHIP_LIFT(7)
    LOLHIP_LIFT(8) LOLHIP_LIFT(9) LOLHIP_LIFT(10) LOLHIP_LIFT(11) LOLHIP_LIFT(12) LOLHIP_LIFT(13) LOLHIP_LIFT(14)
    LOLHIP_LIFT(15) LOLHIP_LIFT(16)
    default: return hipErrorInvalidValue;
  }
#undef LOLHIP_LIFT
  return hipGetLastError();
}

}  // namespace lolhip
