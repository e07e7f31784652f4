// lol_amd/csrc/tile_dev.h — the device side the LDS-tile stage kernels share (k_gauss_dense, k_cplx_dense:
// floatpath.hip; k_zq_dense: zqdense.hip; k_zq_scan: zqscan.hip).  A workgroup holds a tile of `items` whole
// polynomials of n elements in LDS, and every d-vector of the tile (item, block, r) is a column of a stage: element c
// of it sits at item n + blk d rts + c rts + r.  A dense stage is one matrix product over all the columns, out of
// place, in one of two layouts (lanes_along_r, tile_host.h):
//   rows  (stride below a wave)   a thread owns one output row across J columns.  The matrix element comes from the
//         transposed copy (consecutive lanes, consecutive words) and feeds J multiply-adds; the J inputs are LDS reads
//         at an address the lanes of one column group share (a broadcast).
//   cols  (stride of at least a wave)   a wave owns J rows of 64 consecutive columns: one conflict-free LDS read per
//         thread feeds J multiply-adds, the J matrix elements are wave-uniform.
// The ring (R, C, Z_q) is the caller's: dots(mat, in, acc) computes the J products acc[j] = sum_c M[mat(c, j)] *
// src[in(c, j)], c ascending, where mat and in give the index of the two factors of term c of product j in the matrix
// copy of the layout and in the tile; put(x, loc, v) finishes product v and stores it at element x of the tile, which
// is element loc of its polynomial.  Also here: the index helpers and zq_put, the write-back of the Z_q kernels.
#pragma once
#include "generic_dev.h"

namespace lolhip {

__device__ __forceinline__ int fdiv40(int x, u64 M) { return (int)(((u64)(u32)x * M) >> 40); }   // x / v, M = floor(2^40/v)+1
__device__ __forceinline__ u64 magic40_dev(int v) { return ((u64)1 << 40) / (u64)(v > 0 ? v : 1) + 1; }

// Column col of the tile, nq = n / d columns per item: the tile-relative position (base) of its element 0, and with it
// the polynomial-relative one (loc), which a stage with a folded diagonal over C needs.  Callers that need base alone
// take tile_col_base: written as one expression it is what the compiler keeps out of the products' inner loops.
__device__ __forceinline__ int tile_col_base(const Stage& st, int col, int n, int nq, u64 m_nq) {
  const int item = fdiv40(col, m_nq), q = col - item * nq;
  const int blk = fdiv40(q, st.m_rts), r = q - blk * st.rts;
  return item * n + blk * st.d * st.rts + r;
}
struct TileCol { int base, loc; };
__device__ __forceinline__ TileCol tile_col(const Stage& st, int col, int n, int nq, u64 m_nq) {
  const int item = fdiv40(col, m_nq), q = col - item * nq;
  const int blk = fdiv40(q, st.m_rts), r = q - blk * st.rts;
  return TileCol{item * n + blk * st.d * st.rts + r, blk * st.d * st.rts + r};
}

template <int J, typename Acc, typename Dots, typename Put>
__device__ __forceinline__ void tile_dense_rows(const Stage& st, int n, int items, Dots dots, Put put) {
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq, ngroups = (ncols + J - 1) / J;
  const u64 m_nq = magic40_dev(nq);
  for (int w = threadIdx.x; w < d * ngroups; w += blockDim.x) {
    const int cg = fdiv40(w, st.m_d), row = w - cg * d;
    int base[J], loc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int col = cg * J + j;
      const TileCol tc = tile_col(st, col < ncols ? col : ncols - 1, n, nq, m_nq);      // a dead column re-reads the last live one
      base[j] = tc.base; loc[j] = tc.loc;
    }
    Acc acc[J];
    dots([&](int c, int) { return c * d + row; }, [&](int c, int j) { return base[j] + c * rts; }, acc);
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (cg * J + j < ncols) put(base[j] + row * rts, loc[j] + row * rts, acc[j]);
  }
}

template <int J, typename Acc, typename Dots, typename Put>
__device__ __forceinline__ void tile_dense_cols(const Stage& st, int n, int items, Dots dots, Put put) {
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq;
  const int nrg = (d + J - 1) / J, nchunks = (ncols + 63) >> 6;
  const u64 m_nq = magic40_dev(nq);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int nwaves = (int)(blockDim.x >> 6);
  for (int wi = wave; wi < nrg * nchunks; wi += nwaves) {
    const int rg = wi / nchunks, chunk = wi - rg * nchunks, row0 = rg * J;
    const int col = chunk * 64 + lane;
    const TileCol tc = tile_col(st, col < ncols ? col : ncols - 1, n, nq, m_nq);
    const int base = tc.base, loc = tc.loc;
    int moff[J];
#pragma unroll
    for (int j = 0; j < J; ++j) moff[j] = (row0 + j < d ? row0 + j : d - 1) * d;   // a dead row re-reads the last live one
    Acc acc[J];
    dots([&](int c, int j) { return moff[j] + c; }, [&](int c, int) { return base + c * rts; }, acc);
    if (col < ncols) {
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (row0 + j < d) put(base + (row0 + j) * rts, loc + (row0 + j) * rts, acc[j]);
    }
  }
}

// the stage's diagonal on output element x of the tile (x = item * n + index in the polynomial), then the store
template <typename Wd>
__device__ __forceinline__ void zq_put(const Stage& st, Wd* __restrict__ dst, int x, u64 v, int n, u64 m_n,
                                       const u64* __restrict__ cst, const ModCtx& mc) {
  if (st.tw_off >= 0) {
    const int xi = x - fdiv40(x, m_n) * n;
    const int xd = fdiv40(xi, st.m_twdiv);
    v = gmul<sizeof(Wd) == 4>(v, cst[st.tw_off + xd - fdiv40(xd, st.m_twmod) * st.tw_mod], mc);
  }
  dst[x] = (Wd)v;
}

}  // namespace lolhip
