// lol_amd/csrc/generic_dev.h — one output element of one stage of a stage program (plan.h), out of place: the
// arithmetic of the scalar interpreter k_generic (kernels.hip), shared with the element-wise stages of the dense
// Z_q kernels (zqdense.hip).
#pragma once
#include "plan.h"
#include "zq_dev.h"

namespace lolhip {

__device__ __forceinline__ u64 dot_reduce(unsigned __int128 acc, const ModCtx& mc) {
  return reduce128((u64)(acc >> 64), (u64)acc, mc);
}

// k mod q for a small constant k (almost always k < q: skip the 64-bit division)
__device__ __forceinline__ u64 smallmod(u64 k, u64 q) { return k < q ? k : k % q; }
// x / v for x < 2^20 with M = floor(2^40/v)+1 (integer division is ~40 instructions on this ISA)
template <bool MAGIC> __device__ __forceinline__ int fdiv(int x, u64 M, int v) {
  if constexpr (MAGIC) return (int)(((u64)(u32)x * M) >> 40); else return x / v;
}
// a*b mod q for the generic path; Q32: both operands (and q) are below 2^32, one 32x32 product
template <bool Q32> __device__ __forceinline__ u64 gmul(u64 a, u64 b, const ModCtx& mc) {
  if constexpr (Q32) return rem128(0, (u64)(u32)a * (u32)b, mc);
  else return mulmod(a, b, mc);
}
// out-of-place evaluation of one output element of one stage.
// Q32 (every modulus of the plan < 2^32, the reference's own valid domain and below): the
// dot products multiply 32-bit operands — one v_mad_u64_u32 per term instead of a 64x64->128
// product — still accumulated exactly in 128 bits and reduced once.
// Wd: the word the input buffer holds, u64, or u32 for an LDS tile of a Q32 plan (zqdense.hip).
template <bool MAGIC, bool Q32, typename Wd = u64>
__device__ __forceinline__ u64 stage_eval(const Stage& st, const Wd* __restrict__ in, int x,
                                          const u64* __restrict__ cst, const ModCtx& mc) {
  const u64 q = mc.q;
  u64 out;
  if (st.kind == ST_DIAG) {
    out = in[x];
  } else if (st.kind == ST_SCALE) {
    return gmul<Q32>(in[x], cst[st.tw_off], mc);
  } else {
    const int rts = st.rts, d = st.d, p = st.p;
    const int xb = fdiv<MAGIC>(x, st.m_rts, rts);
    const int i = xb - fdiv<MAGIC>(xb, st.m_d, d) * d;
    const Wd* vin = in + (x - i * rts);
    switch (st.kind) {
      case ST_DFTP:
      case ST_CRTP:
      case ST_CRTPINV: {
        const u64* row = cst + st.mat_off + i * d;      // dense matrix row (plan.cpp)
        unsigned __int128 acc = 0;
        u64 part = 0;
        int cnt = 0;
        for (int c = 0; c < d; ++c) {
          if constexpr (Q32) acc += (unsigned __int128)((u64)(u32)vin[c * rts] * (u32)row[c]);
          else acc += (unsigned __int128)vin[c * rts] * row[c];
          if (++cnt == 8) {   // 8 products of < 2^124 fit in 128 bits
            part = addmod(part, dot_reduce(acc, mc), q); acc = 0;
            cnt = 0;
          }
        }
        out = cnt ? addmod(part, dot_reduce(acc, mc), q) : part;
        break;
      }
      case ST_L: {
        u64 s = 0;
        for (int c = 0; c <= i; ++c) s = addmod(s, vin[c * rts], q);
        out = s;
        break;
      }
      case ST_LINV:
        out = (i == 0) ? vin[0] : submod(vin[i * rts], vin[(i - 1) * rts], q);
        break;
      case ST_GPOW: {
        const u64 last = vin[(d - 1) * rts];
        out = addmod(vin[i * rts], last, q);
        if (i > 0) out = submod(out, vin[(i - 1) * rts], q);
        break;
      }
      case ST_GDEC: {
        if (i > 0) {
          out = submod(vin[i * rts], vin[(i - 1) * rts], q);
        } else {
          u64 s = vin[0];
          for (int c = 0; c < d; ++c) s = addmod(s, vin[c * rts], q);
          out = s;
        }
        break;
      }
      case ST_GINVPOW: {
        u64 le = 0, re = 0;
        for (int c = 0; c < d; ++c) {
          if (c <= i) le = addmod(le, vin[c * rts], q); else re = addmod(re, vin[c * rts], q);
        }
        out = submod(gmul<Q32>(smallmod((u64)(p - 1 - i), q), le, mc), gmul<Q32>(smallmod((u64)(i + 1), q), re, mc), q);
        break;
      }
      case ST_GINVDEC: {
        u64 s = 0, hi = 0;
        for (int c = 0; c < d; ++c) {
          s = addmod(s, gmul<Q32>(smallmod((u64)(c + 1), q), vin[c * rts], mc), q);
          if (c > i) hi = addmod(hi, vin[c * rts], q);
        }
        out = submod(s, gmul<Q32>(smallmod((u64)p, q), hi, mc), q);
        break;
      }
      default:
        out = in[x];
    }
  }
  if (st.tw_off >= 0) {
    const int xd = fdiv<MAGIC>(x, st.m_twdiv, st.tw_div);
    out = gmul<Q32>(out, cst[st.tw_off + xd - fdiv<MAGIC>(xd, st.m_twmod, st.tw_mod) * st.tw_mod], mc);
  }
  return out;
}

}  // namespace lolhip
