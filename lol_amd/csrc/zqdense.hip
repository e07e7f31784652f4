// lol_amd/csrc/zqdense.hip — Z_q stage programs with a prime above 13, for plans created with LOLHIP_ROUTE_DENSE_ZQ.
//
// CRT_p at a prime index is a dense (p-1) x (p-1) matrix applied to a batch of vectors.  The scalar interpreter
// (k_generic, kernels.hip) computes each output element as its own dot product: a matrix word from global memory and
// a strided LDS read per term.  Here a workgroup holds a TILE of polynomials of one RNS component in LDS, and every
// d-vector of the tile (item, block, r) is a column of one matrix product:
//
//   rows  (stride below a wave)   a thread owns one output row across ZD_J columns.  The matrix word comes from the
//         plan's transposed copy (consecutive lanes, consecutive words) and feeds ZD_J multiply-adds; the ZD_J inputs
//         are LDS reads at an address the lanes of one column group share (a broadcast).
//   cols  (stride of at least a wave)   a wave owns ZD_J rows of 64 consecutive columns: one conflict-free LDS read
//         per thread feeds ZD_J multiply-adds, the ZD_J matrix words are wave-uniform.
//
// Words in LDS are 4 bytes when every modulus is below 2^32, else 8.  The accumulation is lazy: 32 x 32 products go into
// a 64-bit accumulator that is folded every `fold` terms (the host states the period: (q-1) + fold (q-1)^2 < 2^64);
// wider moduli take 128-bit accumulators folded every 8 terms, as stage_eval does.  The stage's diagonal is applied in
// the write-back.  Every other stage of the program (diagonals, the scale, DFT_2, dense stages of primes up to 13,
// merged vectors) runs element-wise on the tile through stage_eval (generic_dev.h), the scalar interpreter's own
// arithmetic.  Residues are canonical everywhere, so the result is the scalar interpreter's, bit for bit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "kernel_dev.h"
#include "kernels.h"
#include "tile_dev.h"

namespace lolhip {

namespace {

constexpr int ZD_TPB = 256;
constexpr size_t ZD_LDS_BUDGET = ZQ_LDS_BUDGET;

template <typename Wd> constexpr int zd_j() { return sizeof(Wd) == 4 ? 8 : 4; }

// J dot products sharing their matrix words or their inputs, whichever the layout makes uniform.  mat(c, j) and
// in(c, j) give the two factors of term c of product j; both are canonical residues.
template <typename Wd, int J, typename Mat, typename In>
__device__ __forceinline__ void zq_dots(int d, int fold, const ModCtx& mc, Mat mat, In in, u64 (&out)[J]) {
  if constexpr (sizeof(Wd) == 4) {
    u64 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0;
    int c = 0;
    while (c < d) {
      const int ce = d - c < fold ? d : c + fold;
      for (; c < ce; ++c) {
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] += (u64)(u32)mat(c, j) * (u32)in(c, j);
      }
      if (c < d) {
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = rem128(0, acc[j], mc);
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) out[j] = rem128(0, acc[j], mc);
  } else {
    unsigned __int128 acc[J];
    u64 part[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { acc[j] = 0; part[j] = 0; }
    int cnt = 0;
    for (int c = 0; c < d; ++c) {
#pragma unroll
      for (int j = 0; j < J; ++j) acc[j] += (unsigned __int128)mat(c, j) * in(c, j);
      if (++cnt == 8) {                     // 8 products of < 2^124 fit in 128 bits
#pragma unroll
        for (int j = 0; j < J; ++j) { part[j] = addmod(part[j], dot_reduce(acc[j], mc), mc.q); acc[j] = 0; }
        cnt = 0;
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) out[j] = cnt ? addmod(part[j], dot_reduce(acc[j], mc), mc.q) : part[j];
  }
}

// The two layouts of tile_dense_rows / tile_dense_cols (tile_dev.h), written out over Z_q with tile_col_base: in this form
// the products' inner loop keeps one of its J column addresses in a register; through the skeleton every one of them is
// recomputed per term.
template <typename Wd>
__device__ __forceinline__ void zq_dense_rows(const Stage& st, const Wd* __restrict__ src, Wd* __restrict__ dst, int n,
                                              int items, const u64* __restrict__ Mt, const u64* __restrict__ cst,
                                              const ModCtx& mc, int fold) {
  constexpr int J = zd_j<Wd>();
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq, ngroups = (ncols + J - 1) / J;
  const u64 m_nq = magic40_dev(nq), m_n = magic40_dev(n);
  for (int w = threadIdx.x; w < d * ngroups; w += blockDim.x) {
    const int cg = fdiv40(w, st.m_d), row = w - cg * d;
    int base[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int col = cg * J + j;
      base[j] = tile_col_base(st, col < ncols ? col : ncols - 1, n, nq, m_nq);      // a dead column re-reads the last live one
    }
    u64 out[J];
    zq_dots<Wd, J>(d, fold, mc, [&](int c, int) { return Mt[c * d + row]; },
                   [&](int c, int j) { return src[base[j] + c * rts]; }, out);
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (cg * J + j < ncols) zq_put(st, dst, base[j] + row * rts, out[j], n, m_n, cst, mc);
  }
}

template <typename Wd>
__device__ __forceinline__ void zq_dense_cols(const Stage& st, const Wd* __restrict__ src, Wd* __restrict__ dst, int n,
                                              int items, const u64* __restrict__ cst, const ModCtx& mc, int fold) {
  constexpr int J = zd_j<Wd>();
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq;
  const int nrg = (d + J - 1) / J, nchunks = (ncols + 63) >> 6;
  const u64 m_nq = magic40_dev(nq), m_n = magic40_dev(n);
  const u64* __restrict__ M = cst + st.mat_off;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int nwaves = (int)(blockDim.x >> 6);
  for (int wi = wave; wi < nrg * nchunks; wi += nwaves) {
    const int rg = wi / nchunks, chunk = wi - rg * nchunks, row0 = rg * J;
    const int col = chunk * 64 + lane;
    const int base = tile_col_base(st, col < ncols ? col : ncols - 1, n, nq, m_nq);
    int moff[J];
#pragma unroll
    for (int j = 0; j < J; ++j) moff[j] = (row0 + j < d ? row0 + j : d - 1) * d;   // a dead row re-reads the last live one
    u64 out[J];
    zq_dots<Wd, J>(d, fold, mc, [&](int c, int j) { return M[moff[j] + c]; },
                   [&](int c, int) { return src[base + c * rts]; }, out);
    if (col < ncols) {
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (row0 + j < d) zq_put(st, dst, base + (row0 + j) * rts, out[j], n, m_n, cst, mc);
    }
  }
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Matrix-core form (route 2; every modulus fits W <= 4 balanced base-256 limbs after centring, so words are 4 bytes).
// A wave owns a 32-row x 32-column tile of the product and walks the depth in steps of 32.  Per step the lane
// (column, half) reads its 16 inputs out of the LDS tile, centres them and peels the W limbs with y = (v + C) ^ C,
// C = 0x80 in each of the W low bytes (byte w of y is limb w, two's complement); the lane (row, half) loads 16 bytes
// of each of the plan's W limb planes (rows and depth zero padded to multiples of 32).  W^2 v_mfma_i32_32x32x32_i8,
// pair (i, j) into accumulator i + j: |acc_s| <= W * 8192 * 2^14 = 2^29.  Write-back: Horner from the top diagonal,
// z <- (256 z + acc_s) mod q, then the stage's diagonal and the store.  Dead columns contribute zeros and store nothing.
template <int W>
__device__ __forceinline__ void zq_dense_mfma(const Stage& st, const u32* __restrict__ src, u32* __restrict__ dst, int n,
                                              int items, const int8_t* __restrict__ planes, int dp,
                                              const u64* __restrict__ cst, const ModCtx& mc) {
  constexpr int NA = 2 * W - 1;
  constexpr u32 C = 0x80808080u >> (32 - 8 * W);
  const int d = st.d, rts = st.rts, nq = n / d, ncols = items * nq;
  const int nrt = dp >> 5, nct = (ncols + 31) >> 5;
  const u64 m_nq = magic40_dev(nq), m_n = magic40_dev(n);
  const int lane = (int)(threadIdx.x & 63), r32 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nwaves = (int)(blockDim.x >> 6);
  const u32 q = (u32)mc.q, half = q >> 1;
  const u64 off = (((u64)1 << 29) / mc.q + 1) * mc.q;       // a multiple of q above every |acc_s|
  const size_t plane = (size_t)dp * dp;
  for (int wi = wave; wi < nrt * nct; wi += nwaves) {
    const int ct = wi / nrt, rt = wi - ct * nrt;
    const int col = ct * 32 + r32;
    const bool cok = col < ncols;
    const int base = tile_col_base(st, cok ? col : ncols - 1, n, nq, m_nq);
    v16i acc[NA];
#pragma unroll
    for (int s = 0; s < NA; ++s)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[s][e] = 0;
    const int8_t* __restrict__ arow = planes + (size_t)(rt * 32 + r32) * dp + h * 16;
    for (int k0 = 0; k0 < dp; k0 += 32) {
      u32 y[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int c = k0 + h * 16 + j;
        const u32 x = (cok && c < d) ? src[base + c * rts] : 0u;
        const u32 v = x - (x > half ? q : 0u);               // centred, two's complement: |v| <= floor(q / 2) < 2^31
        y[j] = (v + C) ^ C;
      }
      v4i bf[W];
#pragma unroll
      for (int w = 0; w < W; ++w)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          bf[w][t] = (int)(((y[4 * t] >> (8 * w)) & 255u) | ((y[4 * t + 1] >> (8 * w)) & 255u) << 8 |
                           ((y[4 * t + 2] >> (8 * w)) & 255u) << 16 | ((y[4 * t + 3] >> (8 * w)) & 255u) << 24);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint4 a = *reinterpret_cast<const uint4*>(arow + (size_t)i * plane + k0);
        v4i af;
        af[0] = (int)a.x; af[1] = (int)a.y; af[2] = (int)a.z; af[3] = (int)a.w;
#pragma unroll
        for (int j = 0; j < W; ++j) acc[i + j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf[j], acc[i + j], 0, 0, 0);
      }
    }
    // C/D map of the 32 x 32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    if (cok) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = rt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row >= d) continue;
        u64 z = rem128(0, (u64)((i64)acc[NA - 1][e] + (i64)off), mc);
#pragma unroll
        for (int s = NA - 2; s >= 0; --s) z = rem128(0, (z << 8) + (u64)((i64)acc[s][e] + (i64)off), mc);
        zq_put(st, dst, base + row * rts, z, n, m_n, cst, mc);
      }
    }
  }
}

struct ZqArgs {
  i64* y;
  const i64* src;                // never null: y for an in-place launch
  const i64* b;                  // the poly-mul's second operand, else null
  const Stage* stages_inv;       // the poly-mul's inverse program
  int nstages_inv;
  i64 B, ntiles;
  int T, n, nstages, cpc, fold, items;
  const Stage* stages;
  const u64* consts;
  const ModCtx* mod;
  const u64* mt;
  i64 mtpc;
  const int8_t* planes;
  i64 plpc;
  uint8_t kind[ZQ_MAX_STAGES];
  int32_t mt_off[ZQ_MAX_STAGES];
  int32_t dp[ZQ_MAX_STAGES];
  i64 pl_off[ZQ_MAX_STAGES];
};

// One work item = (tile of `items` polynomials, component t), grid-strided.  Two LDS buffers of items * n words: no
// stage runs in place.  A partial tile loads, computes and stores its live items only.  MW: 0, the dense stages on the
// vector ALU; 2..4, on the matrix cores with MW limbs.
// Poly-mul (a.b set): the tile holds the live items of the first operand and, right behind them, those of the second,
// so the forward program runs once over twice the columns; the pointwise product lands on the first half, the inverse
// program runs on that half and it alone is stored.  Everything of a tile is loaded before anything is stored and tiles
// are disjoint, so y may alias either operand and the operands each other.
template <typename Wd, int MW>
__global__ void __launch_bounds__(ZD_TPB)
k_zq_dense(const ZqArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool Q32 = sizeof(Wd) == 4;
  const int n = a.n, T = a.T;
  const i64 nwork = a.ntiles * T;
  const u64 m_n = magic40_dev(n);
  for (i64 wk = blockIdx.x; wk < nwork; wk += gridDim.x) {
    const i64 tile = wk / T;
    const int t = (int)(wk - tile * T);
    const i64 b0 = tile * a.items;
    const int live = (int)(a.B - b0 < a.items ? a.B - b0 : a.items);
    const int tot = live * n;
    const ModCtx mc = a.mod[t];
    const u64* __restrict__ cst = a.consts + (size_t)t * a.cpc;
    const u64* __restrict__ mt = a.mt + (size_t)t * a.mtpc;
    const bool pm = a.b != nullptr;
    Wd* cur = reinterpret_cast<Wd*>(smem);
    Wd* oth = cur + (size_t)a.items * n * (pm ? 2 : 1);
    const i64* in = a.src + (size_t)b0 * n * T + t;
    for (int x = threadIdx.x; x < tot; x += blockDim.x) cur[x] = (Wd)canon_in(in[(size_t)x * T], mc.q);
    if (pm) {
      const i64* inb = a.b + (size_t)b0 * n * T + t;
      for (int x = threadIdx.x; x < tot; x += blockDim.x) cur[tot + x] = (Wd)canon_in(inb[(size_t)x * T], mc.q);
    }
    __syncthreads();
    int live_s = pm ? 2 * live : live;                   // items the current stage runs over
    const int nst = a.nstages + (pm ? a.nstages_inv : 0);
    for (int s = 0; s < nst; ++s) {
      if (pm && s == a.nstages) {                        // the pointwise product, onto the first operand's half
        for (int x = threadIdx.x; x < tot; x += blockDim.x) cur[x] = (Wd)gmul<Q32>(cur[x], cur[tot + x], mc);
        __syncthreads();
        live_s = live;
      }
      const Stage st = s < a.nstages ? a.stages[s] : a.stages_inv[s - a.nstages];
      const int tot_s = live_s * n;
      int kind = ZQ_ELT, mt_off = 0, dp = 0;
      i64 pl_off = 0;
#pragma unroll
      for (int k = 0; k < ZQ_MAX_STAGES; ++k)      // constant indices: the arrays stay in the kernel's argument segment
        if (k == s) { kind = a.kind[k]; mt_off = a.mt_off[k]; dp = a.dp[k]; pl_off = a.pl_off[k]; }
      if (kind == ZQ_ELT) {
        for (int x = threadIdx.x; x < tot_s; x += blockDim.x) {
          const int pi = fdiv40(x, m_n), xi = x - pi * n;
          oth[x] = (Wd)stage_eval<true, Q32, Wd>(st, cur + pi * n, xi, cst, mc);
        }
      } else if constexpr (MW > 0) {
        zq_dense_mfma<MW>(st, cur, oth, n, live_s, a.planes + (size_t)t * a.plpc + pl_off, dp, cst, mc);
      } else if (kind == ZQ_ROWS) {
        zq_dense_rows<Wd>(st, cur, oth, n, live_s, mt + mt_off, cst, mc, a.fold);
      } else {
        zq_dense_cols<Wd>(st, cur, oth, n, live_s, cst, mc, a.fold);
      }
      __syncthreads();
      Wd* tmp = cur; cur = oth; oth = tmp;
    }
    i64* out = a.y + (size_t)b0 * n * T + t;
    for (int x = threadIdx.x; x < tot; x += blockDim.x) out[(size_t)x * T] = (i64)(u64)cur[x];
    __syncthreads();
  }
}

template <typename Wd, int MW>
hipError_t launch_zq_kernel(const ZqArgs& a, i64 grid, size_t lds, hipStream_t stream) {
  if (lds > 64 * 1024) {
    const hipError_t e = allow_big_lds<&k_zq_dense<Wd, MW>>((int)ZD_LDS_BUDGET);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_zq_dense<Wd, MW>), dim3((unsigned)grid), dim3(ZD_TPB), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_zq_dense(const GenericLaunch& g) {
  const ZqDenseLaunch& z = g.zq;
  if (g.B == 0 || g.nstages == 0) return hipSuccess;
  const bool mfma = z.route == 2, pm = z.b != nullptr;
  const int nst = g.nstages + (pm ? z.nstages_inv : 0);
  if (pm && (!z.stages_inv || z.nstages_inv < 1)) return hipErrorInvalidValue;
  if ((z.route != 1 && !mfma) || nst > ZQ_MAX_STAGES || g.n > 8192 || !z.mt || (g.q32 && z.fold < 1))
    return hipErrorInvalidValue;
  if (mfma && (!g.q32 || z.W < 2 || z.W > 4 || !z.planes || z.dmax < 1 || z.dmax > g.n)) return hipErrorInvalidValue;
  const size_t word = g.q32 ? 4 : 8;
  // The tile: as many items as 64 KiB of LDS hold (two workgroups per CU), but no more than leave about 512 tiles to the
  // batch, in whole register tiles of columns (route 2: whole 32-column tiles where the items allow it); one item where a
  // polynomial's ping-pong pair is larger than that (n = 8192 at 8-byte words takes 128 KiB).  With lanes along r a
  // column group never spans items: 32 KiB there, for the occupancy.
  bool rows = false;
  for (int i = 0; i < nst; ++i) if (z.kind[i] == ZQ_ROWS) rows = true;
  const int J = mfma ? 32 : g.q32 ? 8 : 4;
  const size_t per = (pm ? 4 : 2) * (size_t)g.n * word;       // the poly-mul: both operands, twice the columns
  if (per > ZD_LDS_BUDGET) return hipErrorInvalidValue;
  i64 cap = (i64)((size_t)((rows || mfma) ? 64 : 32) * 1024 / per);
  // route 2 computes whole 32-column tiles: where 64 KiB hold fewer columns than one (a large prime index, one column per
  // item), the tile grows towards 32 items within the budget
  if (mfma && cap * (pm ? 2 : 1) * (g.n / z.dmax) < 32) {
    const i64 big = (i64)(ZD_LDS_BUDGET / per), full = (32 + (pm ? 2 : 1) * (g.n / z.dmax) - 1) / ((pm ? 2 : 1) * (g.n / z.dmax));
    cap = big < full ? big : full;
  }
  const i64 items = tile_items(g.B, cap, J);
  const size_t lds = per * (size_t)items;
  const i64 ntiles = (g.B + items - 1) / items;
  i64 grid = ntiles * g.T;
  if (grid > 65536) grid = 65536;                 // as launch_generic caps
  if (const char* e = getenv("LOLHIP_ZQ_DENSE_GRID")) {
    const long v = atol(e);
    grid = v < 1 ? 1 : (v > 65536 ? 65536 : v);
  }
  if (getenv("LOLHIP_ZQ_DENSE_INFO")) {
    char line[512];
    const int at = snprintf(line, sizeof(line), "k_zq_dense: route %d, W %d, n %lld, B %lld, T %d, word %zu, items %lld, lds %zu B, grid %lld, polymul %d, stages",
                            z.route, mfma ? z.W : 0, (long long)g.n, (long long)g.B, g.T, word, (long long)items, lds, (long long)grid, pm ? 1 : 0);
    static const char* const names[3] = {"elt", "dense-rows", "dense-cols"};
    tile_info(line, at, nst, [&](char* p, size_t room, int i) {              // the poly-mul: "*" before the inverse program
      return snprintf(p, room, "%s %s", pm && i == g.nstages ? " *" : "", names[z.kind[i] < 3 ? z.kind[i] : 0]);
    });
  }
  ZqArgs a;
  a.y = g.y; a.src = z.src ? z.src : g.y; a.B = g.B; a.ntiles = ntiles;
  a.b = z.b; a.stages_inv = pm ? z.stages_inv : nullptr; a.nstages_inv = pm ? z.nstages_inv : 0;
  a.T = g.T; a.n = (int)g.n; a.nstages = g.nstages; a.cpc = g.cpc; a.fold = z.fold; a.items = (int)items;
  a.stages = g.stages; a.consts = g.consts; a.mod = g.mod; a.mt = z.mt; a.mtpc = z.mtpc;
  a.planes = z.planes; a.plpc = z.plpc;
  for (int i = 0; i < ZQ_MAX_STAGES; ++i) {
    const bool dense = i < nst && z.kind[i] != ZQ_ELT;
    if (dense && (z.mt_off[i] < 0 || (mfma && (z.pl_off[i] < 0 || z.dp[i] < 32 || z.dp[i] % 32)))) return hipErrorInvalidValue;
    a.kind[i] = dense ? z.kind[i] : (uint8_t)ZQ_ELT;
    a.mt_off[i] = dense ? z.mt_off[i] : 0;
    a.dp[i] = dense ? z.dp[i] : 0;
    a.pl_off[i] = dense && mfma ? z.pl_off[i] : 0;
  }
  if (!mfma) return g.q32 ? launch_zq_kernel<u32, 0>(a, grid, lds, g.stream) : launch_zq_kernel<u64, 0>(a, grid, lds, g.stream);
  switch (z.W) {
    case 2: return launch_zq_kernel<u32, 2>(a, grid, lds, g.stream);
    case 3: return launch_zq_kernel<u32, 3>(a, grid, lds, g.stream);
    default: return launch_zq_kernel<u32, 4>(a, grid, lds, g.stream);
  }
}

}  // namespace lolhip
