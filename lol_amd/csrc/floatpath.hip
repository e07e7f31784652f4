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
//
// tensorCRTC / tensorCRTInvC at a prime above 13 (plans created with LOLHIP_PLAN_DENSE_CPLX): k_cplx_dense.  The same tile
// of items, over C: the DFT_p, CRT_p and CRT_p^-1 stages of such a prime are batched dense complex products, on the FP64
// matrix cores or on the vector ALU (the route of every stage rides in the stage word: kernels.h), between the register
// stages of the small primes, in one launch.  Tolerance contract, so each route sums in its own order.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "kernel_dev.h"
#include "kernels.h"
#include "tile_dev.h"

namespace lolhip {

namespace {

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
            default: break;   // excluded on the host (Plan::cplx_route)
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
// out[col, row] = (sum_c M[row d + c] v[col, c]) / sqrt 2 over the columns of the tile (tile_dev.h), in either layout:
// the matrix is the transposed copy for the rows layout, src the LDS tile, dst the other LDS buffer or the slab.
constexpr int GD_J = 8;          // register tile: columns (rows layout) or rows (cols layout) per thread

__device__ __forceinline__ void gauss_dense(const Stage& st, bool cols, const double* __restrict__ src, double* __restrict__ dst,
                                            int n, int items, const double* __restrict__ cst) {
  const int d = st.d;
  auto dots = [&](const double* __restrict__ M) {
    return [&, M](auto mat, auto in, double (&acc)[GD_J]) {
#pragma unroll
      for (int j = 0; j < GD_J; ++j) acc[j] = 0.0;
      for (int c = 0; c < d; ++c) {
#pragma unroll
        for (int j = 0; j < GD_J; ++j) acc[j] = fma(M[mat(c, j)], src[in(c, j)], acc[j]);
      }
    };
  };
  auto put = [&](int x, int, double v) { dst[x] = v / 1.4142135623730951; };
  if (!cols) tile_dense_rows<GD_J, double>(st, n, items, dots(cst + st.wp_off), put);
  else tile_dense_cols<GD_J, double>(st, n, items, dots(cst + st.mat_off), put);
}

// One tile of `items` polynomials per workgroup pass.  word: the stage word of launch_gauss (kernels.h).  nbuf = 2 when
// a dense stage is followed by another stage (LDS ping-pong); the last stage, when dense, writes the slab directly.
__global__ void __launch_bounds__(256)
k_gauss_dense(double* __restrict__ y, i64 B, int n, const Stage* __restrict__ stages, int word, const double* __restrict__ cst,
              int items) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nstages = word & 255;
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
      const int route = stage_route(word, s);
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
        gauss_dense(st, route != GAUSS_ROWS, cur, dst, n, live, cst);
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

// ---- dense stages of tensorCRTC / tensorCRTInvC -------------------------------------------------
// out[col, row] = tw(row) * sum_c M[row][c] v[col, c] over the columns col = (item, blk, r) of the tile, as for the
// Gaussian map above, over C: a DFT_p (d = p), CRT_p or CRT_p^-1 (d = p - 1) of a prime no register vector holds.  src
// is the LDS tile; dst is the other LDS buffer or, for the last stage of the program, the slab.  The contract of this
// path is a tolerance, not a bit pattern (include/lolhip.h), so the order of summation is each route's own.
constexpr int CD_J = 4;          // register tile of the vector-ALU routes: 4 complex accumulators per thread

// entry of the stage's folded diagonal at position x of the polynomial (as cplx_stage_vec applies it)
__device__ __forceinline__ cd cplx_tw(const Stage& st, const cd* __restrict__ cst, int x) {
  const int xd = fdiv40(x, st.m_twdiv);
  return cst[st.tw_off + xd - fdiv40(xd, st.m_twmod) * st.tw_mod];
}
__device__ __forceinline__ void cplx_fma(cd& acc, cd m, cd v) {
  acc.re = fma(m.re, v.re, fma(-m.im, v.im, acc.re));
  acc.im = fma(m.re, v.im, fma(m.im, v.re, acc.im));
}

// Vector ALU, either layout (tile_dev.h): the matrix is the transposed copy for the rows layout
__device__ __forceinline__ void cplx_dense_valu(const Stage& st, bool cols, const cd* __restrict__ src, cd* __restrict__ dst, int n,
                                                int items, const cd* __restrict__ cst) {
  const int d = st.d;
  auto dots = [&](const cd* __restrict__ M) {
    return [&, M](auto mat, auto in, cd (&acc)[CD_J]) {
#pragma unroll
      for (int j = 0; j < CD_J; ++j) acc[j] = cd{0.0, 0.0};
      for (int c = 0; c < d; ++c) {
#pragma unroll
        for (int j = 0; j < CD_J; ++j) cplx_fma(acc[j], M[mat(c, j)], src[in(c, j)]);
      }
    };
  };
  auto put = [&](int x, int loc, cd o) {
    if (st.tw_off >= 0) o = cmul(o, cplx_tw(st, cst, loc));
    dst[x] = o;
  };
  if (cols) tile_dense_cols<CD_J, cd>(st, n, items, dots(cst + st.mat_off), put);
  else tile_dense_rows<CD_J, cd>(st, n, items, dots(cst + st.wp_off), put);
}

// Matrix cores: v_mfma_f64_16x16x4_f64, D (16 x 16) += A (16 x 4) B (4 x 16).  Lane l holds A[l & 15][l >> 4],
// B[l >> 4][l & 15] and D[(l >> 4) + 4 reg][l & 15], reg < 4.  One complex product is four real ones:
//   out_re = M_re v_re + (-M_im) v_im,   out_im = M_im v_re + M_re v_im,
// from the planes M_re, M_im, -M_im (rows padded to 16, depth to 4 with zeros; tile by tile in lane order, plan.cpp
// plan_upload), so the inner loop is three plane loads, one 16-byte LDS read per column tile and four MFMAs per column
// tile.  A wave owns 16 rows of CM_CT tiles of 16 columns.  Lane l feeds matrix entry [row l & 15][depth l >> 4] and the
// element of depth l >> 4 of column l & 15 either way round:
//   stride >= 16  A = M, B = V: lane l gets rows (l >> 4) + 4 reg of column l & 15 - consecutive lanes, consecutive r;
//   stride < 16   A = V^T, B = M^T: lane l gets row l & 15 of columns (l >> 4) + 4 reg - consecutive lanes, consecutive
//                 rows, which at stride 1 are consecutive words.
// A depth past d re-reads element d - 1 against a zero of the plane; a column past the tile re-reads the last live one
// and is not stored.
typedef double cplx_d4 __attribute__((ext_vector_type(4)));
constexpr int CM_CT = 2;

__device__ __forceinline__ void cplx_dense_mfma(const Stage& st, const cd* __restrict__ src, cd* __restrict__ dst, int n, int items,
                                                const cd* __restrict__ cst) {
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq;
  const int nrt = (d + 15) >> 4, nks = (d + 3) >> 2;
  const int nct = (ncols + 15) >> 4, ncg = (nct + CM_CT - 1) / CM_CT;
  const u64 m_nq = magic40_dev(nq);
  const size_t plane = (size_t)nrt * nks * 64;
  const double* __restrict__ pl = reinterpret_cast<const double*>(cst) + st.pad[0];
  const bool tr = rts < 16;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int nwaves = (int)(blockDim.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  for (int wi = wave; wi < nrt * ncg; wi += nwaves) {
    const int rt = wi / ncg, cg = wi - rt * ncg;
    int base[CM_CT];
    cplx_d4 are[CM_CT], aim[CM_CT];
#pragma unroll
    for (int t = 0; t < CM_CT; ++t) {
      const int col = (cg * CM_CT + t) * 16 + li;
      base[t] = tile_col(st, col < ncols ? col : ncols - 1, n, nq, m_nq).base;
      are[t] = cplx_d4{0.0, 0.0, 0.0, 0.0};
      aim[t] = cplx_d4{0.0, 0.0, 0.0, 0.0};
    }
    const double* __restrict__ pr = pl + (size_t)rt * nks * 64 + lane;
    for (int ks = 0; ks < nks; ++ks) {
      const double mre = pr[(size_t)ks * 64], mim = pr[plane + (size_t)ks * 64], mni = pr[2 * plane + (size_t)ks * 64];
      int c = ks * 4 + lk;
      if (c > d - 1) c = d - 1;
#pragma unroll
      for (int t = 0; t < CM_CT; ++t) {
        const cd v = src[base[t] + c * rts];
        if (!tr) {
          are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(mre, v.re, are[t], 0, 0, 0);
          are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(mni, v.im, are[t], 0, 0, 0);
          aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(mim, v.re, aim[t], 0, 0, 0);
          aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(mre, v.im, aim[t], 0, 0, 0);
        } else {
          are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, mre, are[t], 0, 0, 0);
          are[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, mni, are[t], 0, 0, 0);
          aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, mim, aim[t], 0, 0, 0);
          aim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, mre, aim[t], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < CM_CT; ++t) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = rt * 16 + (tr ? li : lk + 4 * reg);
        const int col = (cg * CM_CT + t) * 16 + (tr ? lk + 4 * reg : li);
        if (row < d && col < ncols) {
          const TileCol tc = tile_col(st, col, n, nq, m_nq);
          cd o = cd{are[t][reg], aim[t][reg]};
          if (st.tw_off >= 0) o = cmul(o, cplx_tw(st, cst, tc.loc + row * rts));
          dst[tc.base + row * rts] = o;
        }
      }
    }
  }
}

// One tile of `items` polynomials per workgroup pass.  word: the stage word of launch_cplx (kernels.h).  The launcher
// gives two LDS buffers when a dense stage is followed by another stage; the last stage, when dense, writes the slab.
__global__ void __launch_bounds__(256)
k_cplx_dense(cd* __restrict__ y, i64 B, int n, const Stage* __restrict__ stages, int word, const cd* __restrict__ cst, int items) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nstages = word & 255;
  const i64 ntiles = (B + items - 1) / items;
  const u64 m_n = magic40_dev(n);
  for (i64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const i64 b0 = t * items;
    const int live = (int)(B - b0 < items ? B - b0 : items);
    cd* yt = y + (size_t)b0 * n;
    cd* cur = reinterpret_cast<cd*>(smem);
    cd* oth = cur + (size_t)items * n;
    for (int x = threadIdx.x; x < live * n; x += blockDim.x) cur[x] = yt[x];
    __syncthreads();
    bool in_lds = true;
    for (int s = 0; s < nstages; ++s) {
      const Stage st = stages[s];
      const int route = stage_route(word, s);
      if (st.kind == ST_DIAG || st.kind == ST_SCALE) {
        for (int x = threadIdx.x; x < live * n; x += blockDim.x)
          cur[x] = cmul(cur[x], cplx_tw(st, cst, x - fdiv40(x, m_n) * n));
      } else if (route == CPLX_REG) {
        const int nvec = n / st.d;
        const u64 m_nvec = magic40_dev(nvec);
        for (int w = threadIdx.x; w < live * nvec; w += blockDim.x) {
          const int item = fdiv40(w, m_nvec), vec = w - item * nvec;
          cd* buf = cur + item * n;
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
            default: break;   // excluded on the host (plan.cpp: such a stage is dense or the plan is refused)
          }
        }
      } else {
        const bool last = s == nstages - 1;
        cd* dst = last ? yt : oth;
        if (route == CPLX_MFMA) cplx_dense_mfma(st, cur, dst, n, live, cst);
        else cplx_dense_valu(st, route == CPLX_VALU_COLS, cur, dst, n, live, cst);
        if (last) in_lds = false;
        else { cd* t2 = cur; cur = oth; oth = t2; }
      }
      __syncthreads();
    }
    if (in_lds)
      for (int x = threadIdx.x; x < live * n; x += blockDim.x) yt[x] = cur[x];
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_cplx(hipStream_t s, double* y, i64 B, i64 n, const Stage* stages, int word, const double* cconsts) {
  const int ns = word & 255;
  if (B == 0 || ns == 0) return hipSuccess;
  const bool info = getenv("LOLHIP_CPLX_INFO") != nullptr;
  if ((word >> 8) == 0) {                                   // register stages only
    const size_t lds = (size_t)n * sizeof(cd);
    if (lds > 64 * 1024) {
      hipError_t e = allow_big_lds<&k_cplx>(128 * 1024);
      if (e != hipSuccess) return e;
    }
    i64 grid = B < 4096 ? B : 4096;
    if (info)
      fprintf(stderr, "k_cplx: n %lld, B %lld, items 1, bufs 1, lds %zu B, grid %lld, stages reg\n", (long long)n, (long long)B, lds,
              (long long)grid);
    hipLaunchKernelGGL(k_cplx, dim3((unsigned)grid), dim3(256), lds, s, reinterpret_cast<cd*>(y), B, (int)n, stages, ns,
                       reinterpret_cast<const cd*>(cconsts));
    return hipGetLastError();
  }
  // The tile: as many items as 64 KiB of LDS hold (two workgroups per CU) but no more than leave about 512 tiles to the
  // batch; one item where a polynomial (or its ping-pong pair) is larger than that (up to CPLX_LDS_BUDGET: plan.cpp).
  int nbuf = 1;
  for (int i = 0; i + 1 < ns; ++i)
    if (stage_route(word, i) != CPLX_REG) nbuf = 2;
  const size_t per = (size_t)nbuf * (size_t)n * sizeof(cd);
  const i64 items = tile_items(B, (i64)(64 * 1024 / per), 1);
  const size_t lds = per * (size_t)items;
  if (lds > CPLX_LDS_BUDGET) return hipErrorInvalidValue;   // excluded on the host (Plan::cplx_route)
  if (lds > 64 * 1024) {
    hipError_t e = allow_big_lds<&k_cplx_dense>((int)CPLX_LDS_BUDGET);
    if (e != hipSuccess) return e;
  }
  const i64 ntiles = (B + items - 1) / items;
  const i64 grid = ntiles < 4096 ? ntiles : 4096;
  if (info) {
    char line[320];
    const int at = snprintf(line, sizeof(line), "k_cplx_dense: n %lld, B %lld, items %lld, bufs %d, lds %zu B, grid %lld, stages",
                            (long long)n, (long long)B, (long long)items, nbuf, lds, (long long)grid);
    static const char* const names[4] = {"reg", "dense-valu", "dense-mfma", "dense-valu"};
    tile_info(line, at, ns, [&](char* p, size_t room, int i) { return snprintf(p, room, " %s", names[stage_route(word, i)]); });
  }
  hipLaunchKernelGGL(k_cplx_dense, dim3((unsigned)grid), dim3(256), lds, s, reinterpret_cast<cd*>(y), B, (int)n, stages, word,
                     reinterpret_cast<const cd*>(cconsts), (int)items);
  return hipGetLastError();
}

hipError_t launch_gauss(hipStream_t s, double* y, i64 B, i64 n, const Stage* stages, int word, const double* rconsts) {
  const int ns = word & 255;
  if (B == 0 || ns == 0) return hipSuccess;
  const bool info = getenv("LOLHIP_GAUSS_INFO") != nullptr;
  if ((word >> 8) == 0) {                                   // register stages only
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
    if (i + 1 < ns && stage_route(word, i) != GAUSS_REG) nbuf = 2;
    if (stage_route(word, i) == GAUSS_ROWS) rows = true;
  }
  const size_t per = (size_t)nbuf * (size_t)n * sizeof(double);          // <= 128 KiB (n <= 8192)
  const i64 items = tile_items(B, (i64)((rows ? 64 : 32) * 1024 / per), GD_J);
  const size_t lds = per * (size_t)items;
  if (lds > 64 * 1024) {
    hipError_t e = allow_big_lds<&k_gauss_dense>(128 * 1024);
    if (e != hipSuccess) return e;
  }
  const i64 ntiles = (B + items - 1) / items;
  const i64 grid = ntiles < 4096 ? ntiles : 4096;
  if (info) {
    char line[256];
    const int at = snprintf(line, sizeof(line), "k_gauss_dense: n %lld, B %lld, items %lld, bufs %d, lds %zu B, grid %lld, stages",
                            (long long)n, (long long)B, (long long)items, nbuf, lds, (long long)grid);
    static const char* const names[4] = {"reg", "dense-rows", "dense-cols", "?"};
    tile_info(line, at, ns, [&](char* p, size_t room, int i) { return snprintf(p, room, " %s", names[stage_route(word, i)]); });
  }
  hipLaunchKernelGGL(k_gauss_dense, dim3((unsigned)grid), dim3(256), lds, s, y, B, (int)n, stages, word, rconsts, (int)items);
  return hipGetLastError();
}

}  // namespace lolhip
