// lol_amd/csrc/eltops.hip — L, L^-1, mulG and divG of both bases over int64 slabs (arithmetic mod 2^64) and over slabs of
// doubles, and mulC.  The prime-index maps are the reference's recurrences (l.cpp:28-57, 67-98;
// g.cpp:16-35, 37-58, 60-90, 92-123) in the reference's order of operations: one thread runs one (p-1)-vector
// sequentially, and nothing in this file is contracted into a fused multiply-add, so that doubles come out as the
// reference compiled for a host without FMA gives them.  A complex slab is a slab of doubles with 2 T words per
// coefficient (every map here is real-linear and componentwise).
//
// Layout: y [B][n][W] words.  The batch is one more left tensor factor: item b, block blk, residue lo of the prime with
// (d = p - 1, rts) owns the words  b n W + blk st d + lo + i st,  st = rts W, i < d  —  so a chunk of whole items is
// transformed as one array of (words / d) vectors.
//
//   on-chip route   k_elt_lds: a workgroup loads a chunk of whole items into LDS, applies every odd prime there and
//                   writes it back: each word is read once and written once, one launch, grid-stride over chunks.  The
//                   LDS copy carries one pad word after every 32.  The vectors of the innermost prime sit d words apart
//                   (d even): unpadded, the 32 lanes of a ds_read_b64 group, reading element i of 32 neighbouring
//                   vectors, share 32 / gcd(d, 32) of the 32 eight-byte bank pairs; the pad word shifts every run of
//                   32 words by one pair (d = 2, 4: conflict-free).
//   global route    k_elt_global once per odd prime straight from HBM, then (divG) the division passes.  For items
//                   beyond the LDS, and forced by the ELT_GLOBAL switch.  Same vec_op, same bits.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "elementwise_dev.h"
#include "eltops.h"
#include "kernel_dev.h"

#pragma clang fp contract(off)

namespace lolhip {
namespace {

constexpr int TPB = 256;
constexpr i64 MAX_BLOCKS = 4096;
constexpr int ELT_GROUP = 32;          // most items of one chunk
constexpr int ELT_CHUNK_WORDS = 4096;  // small items are chunked up to this many words

__host__ __device__ constexpr i64 padded(i64 a) { return a + (a >> 5); }

template <class E>
struct Padded {                        // the LDS copy
  E* b;
  __device__ __forceinline__ E& operator()(int a) const { return b[a + (a >> 5)]; }
};
template <class E>
struct Flat {                          // the slab itself
  E* b;
  __device__ __forceinline__ E& operator()(i64 a) const { return b[a]; }
};

// one (p-1)-vector y(a0 + i st), i < p - 1, in place.  E = u64: sums and products wrap; E = double: one rounding each.
template <int OP, class E, class A, class I>
__device__ __forceinline__ void vec_op(const A& y, I a0, I st, int p) {
  const int d = p - 1;
  if constexpr (OP == ELT_L) {                       // y_i += y_(i-1), i ascending
    E prev = y(a0);
    for (int i = 1; i < d; ++i) {
      E& r = y(a0 + i * st);
      prev = r + prev;
      r = prev;
    }
  } else if constexpr (OP == ELT_LINV) {             // y_i -= y_(i-1), i descending
    E cur = y(a0 + (d - 1) * st);
    for (int i = d - 1; i >= 1; --i) {
      const E below = y(a0 + (i - 1) * st);
      y(a0 + i * st) = cur - below;
      cur = below;
    }
  } else if constexpr (OP == ELT_MULGPOW) {          // y_i += last - y_(i-1), i descending; y_0 += last
    const E last = y(a0 + (d - 1) * st);
    E cur = last;
    for (int i = d - 1; i >= 1; --i) {
      const E below = y(a0 + (i - 1) * st);
      y(a0 + i * st) = cur + (last - below);
      cur = below;
    }
    y(a0) = cur + last;
  } else if constexpr (OP == ELT_MULGDEC) {          // acc += y_i, y_i -= y_(i-1), i descending; y_0 += acc
    const E y0 = y(a0);
    E acc = y0, cur = y(a0 + (d - 1) * st);
    for (int i = d - 1; i >= 1; --i) {
      const E below = y(a0 + (i - 1) * st);
      acc = acc + cur;
      y(a0 + i * st) = cur - below;
      cur = below;
    }
    y(a0) = y0 + acc;
  } else if constexpr (OP == ELT_DIVGPOW) {          // y_i = (p-1-i) lelts - (i+1) relts, i descending
    E lelts = 0;
    for (int i = 0; i < d; ++i) lelts = lelts + y(a0 + i * st);
    E relts = 0;
    for (int i = d - 1; i >= 0; --i) {
      E& r = y(a0 + i * st);
      const E z = r;
      const E lm = (E)(p - 1 - i) * lelts, rm = (E)(i + 1) * relts;
      r = lm - rm;
      lelts = lelts - z;
      relts = relts + z;
    }
  } else {                                           // ELT_DIVGDEC: lastOut = sum i y_(i-1); acc -= p y_i, i descending
    E acc = 0;
    for (int i = 1; i < p; ++i) {
      const E term = (E)i * y(a0 + (i - 1) * st);
      acc = acc + term;
    }
    const E rp = (E)p;
    for (int i = d - 1; i >= 1; --i) {
      E& r = y(a0 + i * st);
      const E tmp = acc, prod = r * rp;
      acc = acc - prod;
      r = tmp;
    }
    y(a0) = acc;
  }
}

// v is divisible by the odd d iff q = v d^-1 mod 2^64, read as int64, has |q| <= qmax = floor((2^63 - 1) / d): then q d
// does not overflow and is congruent to v, so it is v, and q is the exact quotient; a divisible v has |v / d| <= qmax.
__device__ __forceinline__ bool exact_quot(u64 v, u64 dinv, i64 qmax, u64* q) {
  *q = v * dinv;
  const i64 s = (i64)*q;
  return s >= -qmax && s <= qmax;
}

// ---------------------------------------------------------------------------------------
// on-chip route: chunks of G whole items (nW words each) through LDS, every odd prime applied there
// ---------------------------------------------------------------------------------------
template <int OP, class E>
__global__ void __launch_bounds__(1024)
k_elt_lds(E* y, int32_t* ok, i64 B, int G, int nW, int W, NormDims nd, double dr, u64 dinv, i64 qmax, int v2) {
  constexpr bool DIV = OP == ELT_DIVGPOW || OP == ELT_DIVGDEC;
  constexpr bool DIVI = DIV && std::is_same_v<E, u64>;
  typedef E E2 __attribute__((ext_vector_type(2)));
  extern __shared__ unsigned char elt_lds[];
  __shared__ int bad[ELT_GROUP];
  const Padded<E> l{reinterpret_cast<E*>(elt_lds)};
  const int t = threadIdx.x, nt = blockDim.x;
  const i64 chunks = (B + G - 1) / G;
  for (i64 c = blockIdx.x; c < chunks; c += gridDim.x) {
    const i64 b0 = c * G;
    const int g = B - b0 < G ? (int)(B - b0) : G;
    const int words = g * nW;
    E* src = y + b0 * nW;
    if (v2) {                                        // nW even and y 16-byte aligned: a pair never straddles a pad word
      const E2* s2 = reinterpret_cast<const E2*>(src);
      for (int a = t; a < (words >> 1); a += nt) {
        const E2 v = s2[a];
        l(2 * a) = v.x;
        l(2 * a + 1) = v.y;
      }
    } else {
      for (int a = t; a < words; a += nt) l(a) = src[a];
    }
    if constexpr (DIVI) {
      if (t < ELT_GROUP) bad[t] = 0;
    }
    __syncthreads();
    for (int k = 0; k < nd.k; ++k) {
      const int d = nd.d[k], st = nd.rts[k] * W;
      const int nvec = words / d;
      for (int v = t; v < nvec; v += nt) {
        const int blk = v / st, lo = v - blk * st;
        vec_op<OP, E>(l, blk * st * d + lo, st, d + 1);
      }
      __syncthreads();
    }
    const auto item = [&](int a) { return G == 1 ? 0 : a / nW; };   // large items come one to a chunk: no division
    if constexpr (DIVI) {                            // the items' flags first: an indivisible item keeps its numerators
      for (int a = t; a < words; a += nt) {
        u64 q;
        if (!exact_quot((u64)l(a), dinv, qmax, &q)) bad[item(a)] = 1;
      }
      __syncthreads();
      if (t < g) ok[b0 + t] = bad[t] ? 0 : 1;
    }
    auto result = [&](int a) -> E {
      const E v = l(a);
      if constexpr (DIVI) return bad[item(a)] ? v : (E)((u64)v * dinv);
      else if constexpr (DIV) return v / (E)dr;
      else return v;
    };
    if (v2) {
      E2* d2 = reinterpret_cast<E2*>(src);
      for (int a = t; a < (words >> 1); a += nt) {
        E2 v;
        v.x = result(2 * a);
        v.y = result(2 * a + 1);
        d2[a] = v;
      }
    } else {
      for (int a = t; a < words; a += nt) src[a] = result(a);
    }
    __syncthreads();                                 // the LDS copy and bad[] are free again
  }
}

// ---------------------------------------------------------------------------------------
// global route: one odd prime per launch, one vector per thread, then the division passes
// ---------------------------------------------------------------------------------------
template <int OP, class E>
__global__ void __launch_bounds__(TPB)
k_elt_global(E* y, i64 nvec, i64 st, int p) {
  const Flat<E> f{y};
  for (i64 v = (i64)blockIdx.x * TPB + threadIdx.x; v < nvec; v += (i64)gridDim.x * TPB) {
    const i64 blk = v / st, lo = v - blk * st;
    vec_op<OP, E>(f, blk * st * (p - 1) + lo, st, p);
  }
}

__global__ void __launch_bounds__(TPB)
k_elt_div_f64(double* y, i64 total, double dr) {
  for (i64 a = (i64)blockIdx.x * TPB + threadIdx.x; a < total; a += (i64)gridDim.x * TPB) y[a] = y[a] / dr;
}

__global__ void __launch_bounds__(TPB)
k_elt_ok(int32_t* ok, i64 B) {
  for (i64 b = (i64)blockIdx.x * TPB + threadIdx.x; b < B; b += (i64)gridDim.x * TPB) ok[b] = 1;
}

// ok[b] (1 on entry) = 0 where item b holds a coefficient oddrad does not divide: plain stores of one value
__global__ void __launch_bounds__(TPB)
k_elt_flag(const u64* __restrict__ y, int32_t* ok, i64 total, i64 nW, u64 dinv, i64 qmax) {
  for (i64 a = (i64)blockIdx.x * TPB + threadIdx.x; a < total; a += (i64)gridDim.x * TPB) {
    u64 q;
    if (!exact_quot(y[a], dinv, qmax, &q)) ok[a / nW] = 0;
  }
}

__global__ void __launch_bounds__(TPB)
k_elt_div_i64(u64* y, const int32_t* __restrict__ ok, i64 total, i64 nW, u64 dinv) {
  for (i64 a = (i64)blockIdx.x * TPB + threadIdx.x; a < total; a += (i64)gridDim.x * TPB)
    if (ok[a / nW]) y[a] = y[a] * dinv;
}

// ---------------------------------------------------------------------------------------
// mulC (types.h:146-152): two rounded products and one rounded sum per part
// ---------------------------------------------------------------------------------------
template <bool V2>
__global__ void __launch_bounds__(TPB)
k_mulc(double* a, const double* b, i64 count) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  for (i64 i = (i64)blockIdx.x * TPB + threadIdx.x; i < count; i += (i64)gridDim.x * TPB) {
    double ar, ai, br, bi;
    if constexpr (V2) {
      const d2 x = reinterpret_cast<const d2*>(a)[i], w = reinterpret_cast<const d2*>(b)[i];
      ar = x.x; ai = x.y; br = w.x; bi = w.y;
    } else {
      ar = a[2 * i]; ai = a[2 * i + 1]; br = b[2 * i]; bi = b[2 * i + 1];
    }
    const double rr = ar * br, ii = ai * bi, ri = ar * bi, ir = ai * br;
    const double re = rr - ii, im = ri + ir;
    if constexpr (V2) {
      d2 o;
      o.x = re; o.y = im;
      reinterpret_cast<d2*>(a)[i] = o;
    } else {
      a[2 * i] = re; a[2 * i + 1] = im;
    }
  }
}

unsigned grid_for(i64 total) { return grid_stride_blocks(total, TPB, MAX_BLOCKS); }

// d^-1 mod 2^64 of an odd d (Newton: each step doubles the correct low bits, 3 to start with)
u64 inv64(u64 d) {
  u64 x = d;
  for (int i = 0; i < 6; ++i) x *= 2 - d * x;
  return x;
}

// the on-chip kernel of (OP, E): raises its LDS limit once per device, as every kernel beyond 64 KiB must
template <int OP, class E>
hipError_t launch_lds(const EltLaunch& a, double dr, u64 dinv, i64 qmax) {
  const i64 nW = a.n * a.W;
  i64 G = ELT_CHUNK_WORDS / nW;
  G = G < 1 ? 1 : (G > ELT_GROUP ? ELT_GROUP : G);
  if (G > a.B) G = a.B;
  const size_t lds = (size_t)padded(G * nW) * sizeof(E);
  if (lds + ELT_GROUP * sizeof(int) > ELT_LDS_BYTES) return hipErrorInvalidValue;   // bad[] is static LDS
  if (lds > 64 * 1024) {
    hipError_t er = allow_big_lds<&k_elt_lds<OP, E>>((int)(ELT_LDS_BYTES - ELT_GROUP * sizeof(int)));
    if (er != hipSuccess) return er;
  }
  const unsigned threads = lds <= 40 * 1024 ? 256 : lds <= 80 * 1024 ? 512 : 1024;
  const i64 chunks = (a.B + G - 1) / G;
  const unsigned grid = (unsigned)(chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS);
  const int v2 = aligned16(a.y) && nW % 2 == 0;
  hipLaunchKernelGGL((k_elt_lds<OP, E>), dim3(grid), dim3(threads), lds, a.stream, static_cast<E*>(a.y), a.ok, a.B, (int)G,
                     (int)nW, a.W, a.nd, dr, dinv, qmax, v2);
  return hipGetLastError();
}

template <int OP, class E>
hipError_t launch_global(const EltLaunch& a, double dr, u64 dinv, i64 qmax) {
  constexpr bool DIV = OP == ELT_DIVGPOW || OP == ELT_DIVGDEC;
  const i64 nW = a.n * a.W, total = a.B * nW;
  for (int k = 0; k < a.nd.k; ++k) {
    const i64 nvec = total / a.nd.d[k];
    hipLaunchKernelGGL((k_elt_global<OP, E>), dim3(grid_for(nvec)), dim3(TPB), 0, a.stream, static_cast<E*>(a.y), nvec,
                       (i64)a.nd.rts[k] * a.W, a.nd.d[k] + 1);
  }
  if constexpr (DIV && std::is_same_v<E, double>) {
    hipLaunchKernelGGL(k_elt_div_f64, dim3(grid_for(total)), dim3(TPB), 0, a.stream, static_cast<double*>(a.y), total, dr);
  } else if constexpr (DIV) {                        // ok itself is the flag word of the division pass
    hipLaunchKernelGGL(k_elt_ok, dim3(grid_for(a.B)), dim3(TPB), 0, a.stream, a.ok, a.B);
    hipLaunchKernelGGL(k_elt_flag, dim3(grid_for(total)), dim3(TPB), 0, a.stream, static_cast<const u64*>(a.y), a.ok, total, nW,
                       dinv, qmax);
    hipLaunchKernelGGL(k_elt_div_i64, dim3(grid_for(total)), dim3(TPB), 0, a.stream, static_cast<u64*>(a.y), a.ok, total, nW,
                       dinv);
  }
  return hipGetLastError();
}

template <int OP>
hipError_t launch_op(const EltLaunch& a, double dr, u64 dinv, i64 qmax) {
  if (a.global) return a.f64 ? launch_global<OP, double>(a, dr, dinv, qmax) : launch_global<OP, u64>(a, dr, dinv, qmax);
  return a.f64 ? launch_lds<OP, double>(a, dr, dinv, qmax) : launch_lds<OP, u64>(a, dr, dinv, qmax);
}

}  // namespace

size_t elt_lds_bytes(i64 n, int W) { return (size_t)padded(n * W) * 8 + ELT_GROUP * sizeof(int); }

hipError_t launch_elt(const EltLaunch& a) {
  if (a.B == 0) return hipSuccess;
  if (a.n < 1 || a.n > ELT_MAX_N || a.W < 1 || a.W > 2 * ELT_MAX_T || a.nd.k < 1 || a.nd.k > NORM_MAX_PRIMES)
    return hipErrorInvalidValue;
  if (a.oddrad < 3 || !(a.oddrad & 1) || a.B > INT64_MAX / (a.n * a.W)) return hipErrorInvalidValue;
  for (int k = 0; k < a.nd.k; ++k)
    if (a.nd.d[k] < 2 || a.nd.rts[k] < 1 || a.n % ((i64)a.nd.d[k] * a.nd.rts[k])) return hipErrorInvalidValue;
  if (!a.global && !elt_fits_lds(a.n, a.W)) return hipErrorInvalidValue;
  if (getenv("LOLHIP_ELT_INFO"))
    fprintf(stderr, "k_elt: route %s, op %d, word %s, n %lld, W %d, lds %zu B\n", a.global ? "global" : "lds", a.op,
            a.f64 ? "f64" : "u64", (long long)a.n, a.W, a.global ? (size_t)0 : elt_lds_bytes(a.n, a.W));
  const double dr = (double)a.oddrad;
  const u64 dinv = inv64((u64)a.oddrad);
  const i64 qmax = INT64_MAX / a.oddrad;
  switch (a.op) {
    case ELT_L: return launch_op<ELT_L>(a, dr, dinv, qmax);
    case ELT_LINV: return launch_op<ELT_LINV>(a, dr, dinv, qmax);
    case ELT_MULGPOW: return launch_op<ELT_MULGPOW>(a, dr, dinv, qmax);
    case ELT_MULGDEC: return launch_op<ELT_MULGDEC>(a, dr, dinv, qmax);
    case ELT_DIVGPOW: return launch_op<ELT_DIVGPOW>(a, dr, dinv, qmax);
    case ELT_DIVGDEC: return launch_op<ELT_DIVGDEC>(a, dr, dinv, qmax);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_elt_ok(hipStream_t s, int32_t* ok, i64 B) {
  if (B == 0) return hipSuccess;
  hipLaunchKernelGGL(k_elt_ok, dim3(grid_for(B)), dim3(TPB), 0, s, ok, B);
  return hipGetLastError();
}

hipError_t launch_mulc(hipStream_t s, double* a, const double* b, i64 count) {
  if (count == 0) return hipSuccess;
  if (aligned16(a, b)) hipLaunchKernelGGL(k_mulc<true>, dim3(grid_for(count)), dim3(TPB), 0, s, a, b, count);
  else hipLaunchKernelGGL(k_mulc<false>, dim3(grid_for(count)), dim3(TPB), 0, s, a, b, count);
  return hipGetLastError();
}

}  // namespace lolhip
