// lol_amd/csrc/floatpath.hip — the floating-point members of the Tensor class that sit beside the
// Z_q hot path, float64, separate tolerance contract (rel 1e-12 against lol-cpp):
//
//   tensorCRTC / tensorCRTInvC   crt.cpp:583-598: ppcrt / ppcrtinv instantiated at Complex — the CRT
//                                over C that UCyc falls back to when a modulus has no CRT basis
//                                (CRTExt, UCyc.hs:422-444).  The plan's Z_q stage lists are
//                                reused with a second constant pool over C (plan.cpp).
//   tensorGaussianDec            random.cpp:19-64: the linear map that turns iid real Gaussians
//                                into a sample in the decoding basis (CPP.hs:376-389): per odd
//                                prime p a real (p-1) x (p-1) matrix on every (p-1)-vector.
//
// One polynomial per workgroup, resident in LDS (n <= 8192: 128 KiB of complex doubles); one
// thread owns one d-vector of a stage (d <= 13), reads it once, applies the dense map in
// registers in the reference's summation order, writes it back in place.
//
// tensorGaussianDec at a prime above 13 (plans created with LOLHIP_PLAN_DENSE_GAUSS): k_gauss_dense.  A (p-1)-vector
// no longer fits one thread, so the stage is a batched dense product out of LDS: a workgroup holds a tile of items
// (polynomials), and every (p-1)-vector of the tile (item, block, r) is a column.  Same accumulator, same order of
// summation and the same fused multiply-add as the register stage, so both routes give the same bits.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "kernels.h"

namespace lolhip {

namespace {

__device__ __forceinline__ int fdiv40(int x, u64 M) { return (int)(((u64)(u32)x * M) >> 40); }   // x / v, M = floor(2^40/v)+1

struct cd { double re, im; };
__device__ __forceinline__ cd cmul(cd a, cd b) { return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cd cadd(cd a, cd b) { return cd{a.re + b.re, a.im + b.im}; }

template <int D>
__device__ __forceinline__ void cplx_stage_vec(const Stage& st, cd* __restrict__ buf, int vec, const cd* __restrict__ cst) {
  const int rts = st.rts;
  const int blk = fdiv40(vec, st.m_rts), r = vec - blk * rts;
  const int x0 = blk * D * rts + r;
  cd* base = buf + x0;
  cd v[D], o[D];
#pragma unroll
  for (int i = 0; i < D; ++i) v[i] = base[i * rts];
  const cd* M = cst + st.mat_off;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    cd acc = cmul(v[0], M[i * D]);
#pragma unroll
    for (int c = 1; c < D; ++c) acc = cadd(acc, cmul(v[c], M[i * D + c]));
    o[i] = acc;
  }
  if (st.tw_off >= 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int xd = fdiv40(x0 + i * rts, st.m_twdiv);
      o[i] = cmul(o[i], cst[st.tw_off + xd - fdiv40(xd, st.m_twmod) * st.tw_mod]);
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i) base[i * rts] = o[i];
}

__global__ void __launch_bounds__(256)
k_cplx(cd* __restrict__ y, i64 B, int n, const Stage* __restrict__ stages, int nstages, const cd* __restrict__ cst) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cd* buf = reinterpret_cast<cd*>(smem);
  for (i64 b = blockIdx.x; b < B; b += gridDim.x) {
    cd* yb = y + (size_t)b * n;
    for (int x = threadIdx.x; x < n; x += blockDim.x) buf[x] = yb[x];
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
      const Stage st = stages[s];
      if (st.kind == ST_DIAG || st.kind == ST_SCALE) {
        for (int x = threadIdx.x; x < n; x += blockDim.x) {
          const int xd = fdiv40(x, st.m_twdiv);
          buf[x] = cmul(buf[x], cst[st.tw_off + xd - fdiv40(xd, st.m_twmod) * st.tw_mod]);
        }
      } else {
        const int nvec = n / st.d;
        for (int vec = threadIdx.x; vec < nvec; vec += blockDim.x) {
          switch (st.d) {
            case 2: cplx_stage_vec<2>(st, buf, vec, cst); break;
            case 3: cplx_stage_vec<3>(st, buf, vec, cst); break;
            case 4: cplx_stage_vec<4>(st, buf, vec, cst); break;
            case 5: cplx_stage_vec<5>(st, buf, vec, cst); break;
            case 6: cplx_stage_vec<6>(st, buf, vec, cst); break;
            case 7: cplx_stage_vec<7>(st, buf, vec, cst); break;
            case 10: cplx_stage_vec<10>(st, buf, vec, cst); break;
            case 11: cplx_stage_vec<11>(st, buf, vec, cst); break;
            case 12: cplx_stage_vec<12>(st, buf, vec, cst); break;
            case 13: cplx_stage_vec<13>(st, buf, vec, cst); break;
            default: break;   // excluded on the host (Plan::cplx_ok)
          }
        }
      }
      __syncthreads();
    }
    for (int x = threadIdx.x; x < n; x += blockDim.x) yb[x] = buf[x];
    __syncthreads();
  }
}

template <int D>
__device__ __forceinline__ void gauss_stage_vec(const Stage& st, double* __restrict__ buf, int vec, const double* __restrict__ cst) {
  const int rts = st.rts;
  const int blk = fdiv40(vec, st.m_rts), r = vec - blk * rts;
  double* base = buf + blk * D * rts + r;
  double v[D], o[D];
#pragma unroll
  for (int i = 0; i < D; ++i) v[i] = base[i * rts];
  const double* M = cst + st.mat_off;         // entries 2 c(row * col mod p)
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) acc += M[i * D + c] * v[c];      // the reference's order of summation (random.cpp:35-41)
    o[i] = acc / 1.4142135623730951;                             // acc / sqrt(2) (random.cpp:42)
  }
#pragma unroll
  for (int i = 0; i < D; ++i) base[i * rts] = o[i];
}

__global__ void __launch_bounds__(256)
k_gauss(double* __restrict__ y, i64 B, int n, const Stage* __restrict__ stages, int nstages, const double* __restrict__ cst) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* buf = reinterpret_cast<double*>(smem);
  for (i64 b = blockIdx.x; b < B; b += gridDim.x) {
    double* yb = y + (size_t)b * n;
    for (int x = threadIdx.x; x < n; x += blockDim.x) buf[x] = yb[x];
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
      const Stage st = stages[s];
      const int nvec = n / st.d;
      for (int vec = threadIdx.x; vec < nvec; vec += blockDim.x) {
        switch (st.d) {
          case 2: gauss_stage_vec<2>(st, buf, vec, cst); break;
          case 4: gauss_stage_vec<4>(st, buf, vec, cst); break;
          case 6: gauss_stage_vec<6>(st, buf, vec, cst); break;
          case 10: gauss_stage_vec<10>(st, buf, vec, cst); break;
          case 12: gauss_stage_vec<12>(st, buf, vec, cst); break;
          default: break;
        }
      }
      __syncthreads();
    }
    for (int x = threadIdx.x; x < n; x += blockDim.x) yb[x] = buf[x];
    __syncthreads();
  }
}

// ---- dense stages of tensorGaussianDec ---------------------------------------------------------
// out[col, row] = (sum_c M[row d + c] v[col, c]) / sqrt 2 over the columns col = (item, blk, r) of the tile, element c of
// a column at item n + blk d rts + c rts + r.  src is the LDS tile; dst is the other LDS buffer or, for the last stage
// of the program, the slab itself (same layout), so a stage never runs in place.
constexpr int GD_J = 8;          // register tile: columns (rows layout) or rows (cols layout) per thread

__device__ __forceinline__ u64 magic40_dev(int v) { return ((u64)1 << 40) / (u64)(v > 0 ? v : 1) + 1; }

// base address of column col: nq = n / d columns per item
__device__ __forceinline__ int gauss_col_base(const Stage& st, int col, int n, int nq, u64 m_nq) {
  const int item = fdiv40(col, m_nq), q = col - item * nq;
  const int blk = fdiv40(q, st.m_rts), r = q - blk * st.rts;
  return item * n + blk * st.d * st.rts + r;
}

// Lanes along the rows (stride below a wave): a thread owns one output row across GD_J columns.  The matrix element
// comes from the transposed copy (consecutive lanes, consecutive words) and feeds GD_J multiply-adds; the GD_J inputs
// are LDS reads at an address the lanes of one column group share (a broadcast).
__device__ __forceinline__ void gauss_dense_rows(const Stage& st, const double* __restrict__ src, double* __restrict__ dst,
                                                 int n, int items, const double* __restrict__ cst) {
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq, ngroups = (ncols + GD_J - 1) / GD_J;
  const u64 m_nq = magic40_dev(nq);
  const double* __restrict__ Mt = cst + st.wp_off;
  for (int w = threadIdx.x; w < d * ngroups; w += blockDim.x) {
    const int cg = fdiv40(w, st.m_d), row = w - cg * d;
    int base[GD_J];
    double acc[GD_J];
#pragma unroll
    for (int j = 0; j < GD_J; ++j) {
      const int col = cg * GD_J + j;
      base[j] = gauss_col_base(st, col < ncols ? col : ncols - 1, n, nq, m_nq);      // a dead column re-reads the last live one
      acc[j] = 0.0;
    }
    for (int c = 0; c < d; ++c) {
      const double m = Mt[c * d + row];
#pragma unroll
      for (int j = 0; j < GD_J; ++j) acc[j] = fma(m, src[base[j] + c * rts], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < GD_J; ++j)
      if (cg * GD_J + j < ncols) dst[base[j] + row * rts] = acc[j] / 1.4142135623730951;
  }
}

// Lanes along r (stride of at least a wave): a wave owns GD_J rows of 64 consecutive columns.  The input is one
// conflict-free LDS read per thread and feeds GD_J multiply-adds; the GD_J matrix elements are wave-uniform.
__device__ __forceinline__ void gauss_dense_cols(const Stage& st, const double* __restrict__ src, double* __restrict__ dst,
                                                 int n, int items, const double* __restrict__ cst) {
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq;
  const int nrg = (d + GD_J - 1) / GD_J, nchunks = (ncols + 63) >> 6;
  const u64 m_nq = magic40_dev(nq);
  const double* __restrict__ M = cst + st.mat_off;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int nwaves = (int)(blockDim.x >> 6);
  for (int wi = wave; wi < nrg * nchunks; wi += nwaves) {
    const int rg = wi / nchunks, chunk = wi - rg * nchunks, row0 = rg * GD_J;
    const int col = chunk * 64 + lane;
    const int base = gauss_col_base(st, col < ncols ? col : ncols - 1, n, nq, m_nq);
    int moff[GD_J];
    double acc[GD_J];
#pragma unroll
    for (int j = 0; j < GD_J; ++j) {
      moff[j] = (row0 + j < d ? row0 + j : d - 1) * d;                                // a dead row re-reads the last live one
      acc[j] = 0.0;
    }
    for (int c = 0; c < d; ++c) {
      const double v = src[base + c * rts];
#pragma unroll
      for (int j = 0; j < GD_J; ++j) acc[j] = fma(M[moff[j] + c], v, acc[j]);
    }
    if (col < ncols) {
#pragma unroll
      for (int j = 0; j < GD_J; ++j)
        if (row0 + j < d) dst[base + (row0 + j) * rts] = acc[j] / 1.4142135623730951;
    }
  }
}

// One tile of `items` polynomials per workgroup pass.  routes: the route word of launch_gauss (kernels.h).  nbuf = 2 when
// a dense stage is followed by another stage (LDS ping-pong); the last stage, when dense, writes the slab directly.
__global__ void __launch_bounds__(256)
k_gauss_dense(double* __restrict__ y, i64 B, int n, const Stage* __restrict__ stages, int routes, const double* __restrict__ cst,
              int items) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nstages = routes & 255;
  const i64 ntiles = (B + items - 1) / items;
  for (i64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const i64 b0 = t * items;
    const int live = (int)(B - b0 < items ? B - b0 : items);
    double* yt = y + (size_t)b0 * n;
    double* cur = reinterpret_cast<double*>(smem);
    double* oth = cur + (size_t)items * n;
    for (int x = threadIdx.x; x < live * n; x += blockDim.x) cur[x] = yt[x];
    __syncthreads();
    bool in_lds = true;
    for (int s = 0; s < nstages; ++s) {
      const Stage st = stages[s];
      const int route = (routes >> (8 + 2 * s)) & 3;            // gauss_stage_route (kernels.h)
      if (route == GAUSS_REG) {
        const int nvec = n / st.d;
        const u64 m_nvec = magic40_dev(nvec);
        for (int w = threadIdx.x; w < live * nvec; w += blockDim.x) {
          const int item = fdiv40(w, m_nvec), vec = w - item * nvec;
          double* buf = cur + item * n;
          switch (st.d) {
            case 2: gauss_stage_vec<2>(st, buf, vec, cst); break;
            case 4: gauss_stage_vec<4>(st, buf, vec, cst); break;
            case 6: gauss_stage_vec<6>(st, buf, vec, cst); break;
            case 10: gauss_stage_vec<10>(st, buf, vec, cst); break;
            case 12: gauss_stage_vec<12>(st, buf, vec, cst); break;
            default: break;
          }
        }
      } else {
        const bool last = s == nstages - 1;
        double* dst = last ? yt : oth;
        if (route == GAUSS_ROWS) gauss_dense_rows(st, cur, dst, n, live, cst);
        else gauss_dense_cols(st, cur, dst, n, live, cst);
        if (last) in_lds = false;
        else { double* t2 = cur; cur = oth; oth = t2; }
      }
      __syncthreads();
    }
    if (in_lds)
      for (int x = threadIdx.x; x < live * n; x += blockDim.x) yt[x] = cur[x];
    __syncthreads();
  }
}

}  // namespace

// k_cplx / k_gauss_dense with more than 64 KiB of dynamic LDS: the attribute, once per device
template <typename K>
static hipError_t allow_big_lds(K kernel, std::atomic<unsigned long long>& done) {
  int dev = -1;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!(done.load(std::memory_order_acquire) >> dev & 1)) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (e != hipSuccess) return e;
    done.fetch_or(1ull << dev, std::memory_order_release);
  }
  return hipSuccess;
}

hipError_t launch_cplx(hipStream_t s, double* y, i64 B, i64 n, const Stage* stages, int nstages, const double* cconsts) {
  if (B == 0 || nstages == 0) return hipSuccess;
  const size_t lds = (size_t)n * sizeof(cd);
  if (lds > 64 * 1024) {
    static std::atomic<unsigned long long> done{0};
    hipError_t e = allow_big_lds(&k_cplx, done);
    if (e != hipSuccess) return e;
  }
  i64 grid = B < 4096 ? B : 4096;
  hipLaunchKernelGGL(k_cplx, dim3((unsigned)grid), dim3(256), lds, s, reinterpret_cast<cd*>(y), B, (int)n, stages, nstages,
                     reinterpret_cast<const cd*>(cconsts));
  return hipGetLastError();
}

hipError_t launch_gauss(hipStream_t s, double* y, i64 B, i64 n, const Stage* stages, int nstages, const double* rconsts) {
  const int ns = nstages & 255;
  if (B == 0 || ns == 0) return hipSuccess;
  const bool info = getenv("LOLHIP_GAUSS_INFO") != nullptr;
  if ((nstages >> 8) == 0) {                                // register stages only
    const size_t lds = (size_t)n * sizeof(double);          // <= 64 KiB
    i64 grid = B < 4096 ? B : 4096;
    if (info) fprintf(stderr, "k_gauss: n %lld, B %lld, stages reg\n", (long long)n, (long long)B);
    hipLaunchKernelGGL(k_gauss, dim3((unsigned)grid), dim3(256), lds, s, y, B, (int)n, stages, ns, rconsts);
    return hipGetLastError();
  }
  // The tile: as many items as 64 KiB of LDS hold (two workgroups per CU), but no more than leave about 512 tiles to
  // the batch, in whole register tiles; one item where a polynomial (or its ping-pong pair) is larger than that.  With
  // lanes along r a column group never spans items, so more items buy nothing there: 32 KiB, for the occupancy.
  int nbuf = 1;
  bool rows = false;
  for (int i = 0; i < ns; ++i) {
    if (i + 1 < ns && gauss_stage_route(nstages, i) != GAUSS_REG) nbuf = 2;
    if (gauss_stage_route(nstages, i) == GAUSS_ROWS) rows = true;
  }
  const size_t per = (size_t)nbuf * (size_t)n * sizeof(double);          // <= 128 KiB (n <= 8192)
  i64 cap = (i64)((rows ? 64 : 32) * 1024 / per);
  i64 want = (B + 511) / 512;
  want = (want + GD_J - 1) / GD_J * GD_J;
  i64 items = want < cap ? want : cap;
  if (items > GD_J) items = items / GD_J * GD_J;
  if (items > B) items = B;
  if (items < 1) items = 1;
  const size_t lds = per * (size_t)items;
  if (lds > 64 * 1024) {
    static std::atomic<unsigned long long> done{0};
    hipError_t e = allow_big_lds(&k_gauss_dense, done);
    if (e != hipSuccess) return e;
  }
  const i64 ntiles = (B + items - 1) / items;
  const i64 grid = ntiles < 4096 ? ntiles : 4096;
  if (info) {
    char line[256];
    int at = snprintf(line, sizeof(line), "k_gauss_dense: n %lld, B %lld, items %lld, bufs %d, lds %zu B, grid %lld, stages",
                      (long long)n, (long long)B, (long long)items, nbuf, lds, (long long)grid);
    static const char* const names[4] = {"reg", "dense-rows", "dense-cols", "?"};
    for (int i = 0; i < ns && at > 0 && at < (int)sizeof(line); ++i)
      at += snprintf(line + at, sizeof(line) - (size_t)at, " %s", names[gauss_stage_route(nstages, i)]);
    fprintf(stderr, "%s\n", line);
  }
  hipLaunchKernelGGL(k_gauss_dense, dim3((unsigned)grid), dim3(256), lds, s, y, B, (int)n, stages, nstages, rconsts, (int)items);
  return hipGetLastError();
}

}  // namespace lolhip
