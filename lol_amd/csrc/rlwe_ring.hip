// lol_amd/csrc/rlwe_ring.hip — the passes of RLWE / RLWR instances over ONE modulus q without a CRT basis (2^k, p^e,
// odd composites).  a s is the exact ring product against a prepared secret (ringmul.hip, DESIGN.md
// 3.4i): lift, crt on the plan of the K <= 3 NTT primes, pointwise product, crtInv, fold.  These passes fuse what comes
// before the lift and after the fold into them.  gfx950 only.
//
//   k_rr_draw_lift   uniform a from the ChaCha20 stream (the words of rlwe.hip's k_rlwe_uniform over one modulus) written
//                    as a_pow [B][n], and in the same pass the K residues of its centred lift [B][n][K], which are what
//                    k_ring_lift would read a_pow again to produce
//   k_rr_fold        the mixed-radix fold of k_ring_fold (sign test, reduction mod q, no wide integers), then a tail in
//                    registers (rlwe_ring.h): + an addend, b - fold, or at an index where L, L^-1 and the Gaussian map
//                    are identities the whole remainder of a call, with the arithmetic of the passes it stands for
//                    (rlwe_dev.h), so both routes give the same bits
//   k_rr_centre      the T = 1 centred lift: one compare
//
// One thread per coefficient pair (per 8 coefficients = one ChaCha20 block in the Gaussian tails, per 4 = one block in
// the draw), the batch's rows laid end to end over a grid-stride launch (short rows still fill their waves), 16-byte
// accesses where every slab is aligned and n is a multiple of the thread's run, constants by value in the launch struct.
// 8 K bytes of la and 8 or 16 bytes of in / out per coefficient.
#include <hip/hip_runtime.h>

#include "elementwise_dev.h"
#include "ringmul_dev.h"
#include "rlwe_dev.h"
#include "rlwe_ring.h"

// the Cont tails are pure functions of their IEEE double operations in the stated order (include/lolhip.h)
#pragma clang fp contract(off)

namespace lolhip {

namespace {
// the row of flat thread index g when `per` threads cover a row: a 32-bit division wherever the index fits one
__device__ __forceinline__ i64 row_of(i64 g, i64 per) {
  return (u64)g >> 32 ? g / per : (i64)((u32)g / (u32)per);
}

// W words at p, as 16-byte accesses (VEC: p is 16-byte aligned and W is even) or as the first cnt single words
template <int W, bool VEC>
__device__ __forceinline__ void load_words(const u64* __restrict__ p, int cnt, u64* x) {
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < W / 2; ++i) {
      const u64x2 a = reinterpret_cast<const u64x2*>(p)[i];
      x[2 * i] = a.x;
      x[2 * i + 1] = a.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = i < cnt ? p[i] : 0;
  }
}

template <int W, bool VEC>
__device__ __forceinline__ void store_words(u64* __restrict__ p, int cnt, const u64* x) {
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < W / 2; ++i) reinterpret_cast<u64x2*>(p)[i] = u64x2{x[2 * i], x[2 * i + 1]};
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i)
      if (i < cnt) p[i] = x[i];
  }
}

// ---------------------------------------------------------------------------------------
// uniform a, 4 residues per ChaCha20 block: residue j -> (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q, and its lift
// ---------------------------------------------------------------------------------------
template <int K, bool VEC>
__global__ void __launch_bounds__(RING_TPB)
k_rr_draw_lift(i64* __restrict__ a_pow, i64* __restrict__ la, i64 B, i64 n, RingMul c, ChaChaKey key, u64 ctr,
               int domain) {
  const ModCtx mc = c.q[0];
  const i64 nblk = (n + 3) >> 2;
  for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < B * nblk; g += (i64)gridDim.x * blockDim.x) {
    const i64 b = row_of(g, nblk), k = g - b * nblk;
    const i64 j = 4 * k;
    const int cnt = n - j < 4 ? (int)(n - j) : 4;
    u32 w[16];
    stream_block(key, ctr, domain, b, (u32)k, w);
    u64 u[4], y[4 * K];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u64 lo = (u64)w[4 * i] | (u64)w[4 * i + 1] << 32, hi = (u64)w[4 * i + 2] | (u64)w[4 * i + 3] << 32;
      u[i] = reduce128(hi, lo, mc);
      lift_residue<K>(u[i], mc.q, c, y + i * K);
    }
    store_words<4, VEC>(reinterpret_cast<u64*>(a_pow) + b * n + j, cnt, u);
    store_words<4 * K, VEC>(reinterpret_cast<u64*>(la) + (b * n + j) * K, cnt * K, y);
  }
}

// ---------------------------------------------------------------------------------------
// fold and tail
// ---------------------------------------------------------------------------------------
constexpr bool gauss_tail(int tail) { return tail == RR_DISC_SAMPLE || tail == RR_CONT_SAMPLE; }
constexpr bool reads_in(int tail) { return tail == RR_ADD || tail == RR_SUB || tail == RR_DISC_ERROR || tail == RR_CONT_ERROR; }
constexpr int run_of(int tail) { return gauss_tail(tail) ? 8 : 2; }

template <int K, bool POW2, int TAIL, bool VEC>
__global__ void __launch_bounds__(RING_TPB)
k_rr_fold(const i64* __restrict__ la, const u64* __restrict__ in, u64* __restrict__ out, i64 B, i64 n, RingMul c,
          RrTail t) {
  constexpr int W = run_of(TAIL);
  const ModCtx mc = c.q[0];
  const u64 q = mc.q;
  const double qd = (double)q;
  const i64 per = (n + W - 1) / W;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < B * per; i += (i64)gridDim.x * blockDim.x) {
    const i64 b = row_of(i, per), g = i - b * per;
    const i64 j = g * W;
    const int cnt = n - j < W ? (int)(n - j) : W;
    u64 x[W * K], v[W], o[W];
    load_words<W * K, VEC>(reinterpret_cast<const u64*>(la) + (b * n + j) * K, cnt * K, x);
    if constexpr (reads_in(TAIL)) load_words<W, VEC>(in + b * n + j, cnt, v);
    double gs[8];
    if constexpr (gauss_tail(TAIL)) gauss8(t.key, t.ctr, CHACHA_DOM_RLWE_GAUSS, b, (u32)g, t.sigma, gs);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const u64 f = fold_word<K, POW2>(x + w * K, mc, 0, c);
      if constexpr (TAIL == RR_ADD) {
        o[w] = addmod(f, canon_in((i64)v[w], q), q);
      } else if constexpr (TAIL == RR_SUB) {
        o[w] = submod(mod_any((i64)v[w], mc), f, q);
      } else if constexpr (TAIL == RR_DISC_SAMPLE) {
        o[w] = addmod(f, mod_any((i64)rint(gs[w]), mc), q);
      } else if constexpr (TAIL == RR_DISC_ERROR) {
        o[w] = (u64)centred(submod(mod_any((i64)v[w], mc), f, q), q);
      } else if constexpr (TAIL == RR_CONT_SAMPLE) {
        o[w] = (u64)__double_as_longlong(rrq_add((double)(i64)f, rrq_reduce(gs[w], qd), qd));
      } else if constexpr (TAIL == RR_CONT_ERROR) {
        const double xd = (double)(i64)f;
        o[w] = (u64)__double_as_longlong(
            rrq_lift(rrq_add(__longlong_as_double((i64)v[w]), rrq_reduce(-xd, qd), qd), qd));
      } else {
        o[w] = (u64)rlwr_round(f, q, t.p);
      }
    }
    store_words<W, VEC>(out + b * n + j, cnt, o);
  }
}

__global__ void __launch_bounds__(256)
k_rr_centre(const i64* x, i64* e, i64 total, u64 q) {
  for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g < total; g += (i64)gridDim.x * 256)
    e[g] = centred(canon_in(x[g], q), q);
}

// one thread per run of a row, the rows laid end to end: short rows (n = 128 is 16 runs of 8) still fill their waves
RingShape flat_shape(i64 threads) {
  return RingShape{dim3(grid_stride_blocks(threads, RING_TPB, RING_MAX_BLOCKS)), dim3(RING_TPB)};
}

bool params_ok(i64 B, i64 n, const RingMul& c) {
  return B > 0 && n > 0 && c.T == 1 && c.K >= 1 && c.K <= RING_MAX_K && B <= 0x7fffffff;
}

template <int TAIL>
hipError_t launch_tail(hipStream_t s, const i64* la, const void* in, void* out, i64 B, i64 n, const RingMul& c,
                       const RrTail& t) {
  constexpr int W = run_of(TAIL);
  if (reads_in(TAIL) != (in != nullptr)) return hipErrorInvalidValue;
  const bool vec = aligned16(la, in, out) && n % W == 0;
  const RingShape sh = flat_shape(B * ((n + W - 1) / W));
  const u64* i = static_cast<const u64*>(in);
  u64* o = static_cast<u64*>(out);
#define LOLHIP_RR_FOLD(KK, P2, V) \
  hipLaunchKernelGGL((k_rr_fold<KK, P2, TAIL, V>), sh.grid, sh.block, 0, s, la, i, o, B, n, c, t)
  switch (c.K * 4 + (c.pow2 ? 2 : 0) + (vec ? 1 : 0)) {
    case 4:  LOLHIP_RR_FOLD(1, false, false); break;
    case 5:  LOLHIP_RR_FOLD(1, false, true); break;
    case 6:  LOLHIP_RR_FOLD(1, true, false); break;
    case 7:  LOLHIP_RR_FOLD(1, true, true); break;
    case 8:  LOLHIP_RR_FOLD(2, false, false); break;
    case 9:  LOLHIP_RR_FOLD(2, false, true); break;
    case 10: LOLHIP_RR_FOLD(2, true, false); break;
    case 11: LOLHIP_RR_FOLD(2, true, true); break;
    case 12: LOLHIP_RR_FOLD(3, false, false); break;
    case 13: LOLHIP_RR_FOLD(3, false, true); break;
    case 14: LOLHIP_RR_FOLD(3, true, false); break;
    default: LOLHIP_RR_FOLD(3, true, true); break;
  }
#undef LOLHIP_RR_FOLD
  return hipGetLastError();
}
}  // namespace

hipError_t launch_rr_draw_lift(hipStream_t s, i64* a_pow, i64* la, i64 B, i64 n, const RingMul& c, const ChaChaKey& key,
                               u64 ctr, int domain) {
  if (B == 0 || n == 0) return hipSuccess;
  if (!a_pow || !la || !params_ok(B, n, c)) return hipErrorInvalidValue;
  const bool vec = aligned16(a_pow, la) && n % 4 == 0;
  const RingShape sh = flat_shape(B * ((n + 3) >> 2));
#define LOLHIP_RR_DRAW(KK)                                                                                        \
  do {                                                                                                            \
    if (vec) hipLaunchKernelGGL((k_rr_draw_lift<KK, true>), sh.grid, sh.block, 0, s, a_pow, la, B, n, c, key, ctr, domain); \
    else hipLaunchKernelGGL((k_rr_draw_lift<KK, false>), sh.grid, sh.block, 0, s, a_pow, la, B, n, c, key, ctr, domain);   \
  } while (0)
  if (c.K == 1) LOLHIP_RR_DRAW(1);
  else if (c.K == 2) LOLHIP_RR_DRAW(2);
  else LOLHIP_RR_DRAW(3);
#undef LOLHIP_RR_DRAW
  return hipGetLastError();
}

hipError_t launch_rr_fold(hipStream_t s, int tail, const i64* la, const void* in, void* out, i64 B, i64 n,
                          const RingMul& c, const RrTail& t) {
  if (B == 0 || n == 0) return hipSuccess;
  if (!la || !out || !params_ok(B, n, c)) return hipErrorInvalidValue;
  switch (tail) {
    case RR_ADD:         return launch_tail<RR_ADD>(s, la, in, out, B, n, c, t);
    case RR_SUB:         return launch_tail<RR_SUB>(s, la, in, out, B, n, c, t);
    case RR_DISC_SAMPLE: return launch_tail<RR_DISC_SAMPLE>(s, la, in, out, B, n, c, t);
    case RR_DISC_ERROR:  return launch_tail<RR_DISC_ERROR>(s, la, in, out, B, n, c, t);
    case RR_CONT_SAMPLE: return launch_tail<RR_CONT_SAMPLE>(s, la, in, out, B, n, c, t);
    case RR_CONT_ERROR:  return launch_tail<RR_CONT_ERROR>(s, la, in, out, B, n, c, t);
    case RR_RLWR:        return launch_tail<RR_RLWR>(s, la, in, out, B, n, c, t);
    default:             return hipErrorInvalidValue;
  }
}

hipError_t launch_rr_centre(hipStream_t s, const i64* x, i64* e, i64 total, u64 q) {
  if (total == 0) return hipSuccess;
  if (!x || !e || total < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rr_centre, dim3(grid_stride_blocks(total, 256, 8192)), dim3(256), 0, s, x, e, total, q);
  return hipGetLastError();
}

}  // namespace lolhip
