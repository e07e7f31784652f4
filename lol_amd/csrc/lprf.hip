// lol_amd/csrc/lprf.hip — the kernels of the key-homomorphic lattice PRF of [BP14] (lol-apps KeyHomomorphicPRF.hs
// latticePRF', eq. 2.3; include/lolhip.h lolhip_lprf_*).  gfx950 only.  One modulus; slabs are row-major
// int64 residues in [0, q).
//
//   k_lprf_node_valu  A_v = A_l * G^-1(A_r) for every slot of node v over an input window, int64 lazy sums on the
//                     vector ALU: out[k][i][c] = sum_{i2, j} L[slot_l(k)][i][i2 ell + j] digit_j(R[slot_r(k)][i2][c])
//   k_lprf_node_mfma  the same residues on the matrix cores: L in W balanced base-256 limbs, the digits as int8,
//                     v_mfma_i32_32x32x32_i8 into one i32 tile per limb, sum_w 256^w acc_w mod q in the write-back
//   k_lprf_keymul     s_key * A per slot (nkeys x n by n x K)
//
// G^-1(A_r) is never stored: a thread that owns column c of the right operand lifts R[i2][c] and peels its ell centred
// digits (k_decompose's order and centring, pipeline.hip) as the sum reaches them.  The slots are those of khprf.hip:
// slot k of v stands for w_v = k (full) or (x0 >> s_v) + k, the children's slots come from child_slot, and slots k,
// k + R, k + 2R, ... share one right slot.  Their left rows are stacked into ONE row dimension per right slot (rows =
// slots per right slot x M), so a row tile is filled even when one matrix has n = 3 rows.  With p != 0 the write-back
// rounds to Z_p (rescaleMod) and o_slot / o_row place the rows of the keyed root as [key][x][K].
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "elementwise_dev.h"
#include "lprf.h"

namespace lolhip {

namespace {
constexpr int TPB = 256;
constexpr i64 MAX_BLOCKS = 1 << 20;

constexpr int V_TM = 16;       // VALU route: rows per block (4 per wave)
constexpr int V_TN = 64;       //             columns per block (one per lane)
constexpr int V_KT = 128;      //             depth of the staged left tile

constexpr int X_TM = 32;       // matrix route: rows per block (one MFMA tile)
constexpr int X_TN = 128;      //               columns per block (32 per wave)
constexpr int X_ST = 4;        //               k-steps (32 deep each) per staged left tile

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ i64 child_slot(i64 w_v, const KhprfChild& ch) {
  const i64 w = w_v >> ch.shift;
  return ch.full ? (w & ch.mask) : w - ch.lo;
}

// one centred base-b digit off v (not the last one: that is v itself), as k_decompose peels it
__device__ __forceinline__ i64 peel(i64& v, const LprfMod& md) {
  const i64 h = md.dp.base >> 1;
  const i64 a = v + h;
  const i64 qd = md.lg >= 0 ? (a >> md.lg) : floor_div_inv(a, md.dp.magic, md.dp.sh1, md.dp.sh2);
  v = qd;
  return a - qd * md.dp.base - h;
}

// rescaleMod of z in [0, q): fst (divModCent (p lift z) q) mod p.  Shifted by p q to stay unsigned: a = p (lift z + q) +
// q div 2 < 1.5 p q + q / 2 < 2^64 (p q < 2^63, q < 2^62), floor(a / q) = y + p with y in [-p/2, p/2]
__device__ __forceinline__ u64 round_p(u64 z, u64 q, u64 p) {
  const u64 vq = 2 * z < q ? z + q : z;
  const u64 quot = (p * vq + (q >> 1)) / q;
  return quot >= p ? quot - p : quot;
}

// rows m0 .. m0 + TM of right-slot group g: the left row and the output row of each (null where there is none)
template <int TM>
__device__ __forceinline__ void row_table(const i64* Lv, i64* out, const LprfNode& nd, i64 g, i64 m0,
                                          const i64** lrow, i64** orow) {
  if (threadIdx.x < TM) {
    const i64 m = m0 + threadIdx.x;
    const i64 t = m / nd.M;
    i64 i = m - t * nd.M;
    i64 k = g + t * nd.R;
    const bool ok = k < nd.U;
    if (!ok) { k = g; i = 0; }                                  // a row past the last slot reads the first one (not stored)
    const i64 ls = child_slot((nd.full ? 0 : nd.lo) + k, nd.l);
    lrow[threadIdx.x] = Lv + (ls * nd.M + i) * (i64)nd.K;
    orow[threadIdx.x] = ok ? out + k * nd.o_slot + i * nd.o_row : nullptr;
  }
}
}  // namespace

// ---------------------------------------------------------------------------------------
// VALU route.  Block = (right-slot group, 16 rows, 64 columns); lane = column, wave = 4 rows.  The left tile [16][128]
// is staged in LDS and read as a broadcast; the lane walks its column of the right operand entry by entry and peels the
// digits.  !WIDE: signed 64-bit sums of a * digit, reduced every md.fold terms ((q-1) + fold (q-1) max|digit| < 2^63,
// asserted where fold is derived); WIDE: 128-bit sums of a * (digit mod q), reduced every 8 terms (8 q^2 + q < 2^127).
// ---------------------------------------------------------------------------------------
template <bool WIDE>
__global__ void __launch_bounds__(TPB)
k_lprf_node_valu(const i64* __restrict__ Lv, const i64* __restrict__ Rv, i64* __restrict__ out, LprfNode nd, LprfMod md,
                 i64 mtiles) {
  __shared__ i64 a_s[V_TM][V_KT];
  __shared__ const i64* lrow[V_TM];
  __shared__ i64* orow[V_TM];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const i64 g = blockIdx.x / mtiles, mt = blockIdx.x - g * mtiles;
  row_table<V_TM>(Lv, out, nd, g, mt * V_TM, lrow, orow);
  const i64 rs = child_slot((nd.full ? 0 : nd.lo) + g, nd.r);
  const int c = (int)blockIdx.y * V_TN + tx;
  const bool cok = c < nd.K;
  const i64* rp = Rv + rs * (i64)nd.n * nd.K + (cok ? c : nd.K - 1);
  const u64 q = md.mc.q;
  using Acc = std::conditional_t<WIDE, u128, i64>;
  Acc acc[4] = {0, 0, 0, 0};
  auto red = [&](Acc a) -> u64 {
    if constexpr (WIDE) return reduce128((u64)(a >> 64), (u64)a, md.mc);
    else return mod_any(a, md.mc);
  };
  const int fold = WIDE ? 8 : md.fold;
  int cnt = 0, i2 = 0, jd = 0;
  i64 v = 0;
  __syncthreads();
  for (int k0 = 0; k0 < nd.K; k0 += V_KT) {
    for (int e = threadIdx.x; e < V_TM * V_KT; e += TPB) {
      const int row = e / V_KT, kk = e - row * V_KT;
      a_s[row][kk] = k0 + kk < nd.K ? lrow[row][k0 + kk] : 0;
    }
    __syncthreads();
    const int kend = nd.K - k0 < V_KT ? nd.K - k0 : V_KT;
    for (int kk = 0; kk < kend; ++kk) {
      if (jd == 0) { v = centred((u64)rp[(i64)i2 * nd.K], q); ++i2; }
      i64 d;
      if (jd == nd.ell - 1) { d = v; jd = 0; } else { d = peel(v, md); ++jd; }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u64 a = (u64)a_s[ty * 4 + r][kk];
        if constexpr (WIDE) acc[r] += (u128)a * (u64)(d < 0 ? d + (i64)q : d);
        else acc[r] += (i64)a * d;
      }
      if (++cnt == fold) {
        cnt = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = (Acc)red(acc[r]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    i64* o = orow[ty * 4 + r];
    if (!o || !cok) continue;
    const u64 z = red(acc[r]);
    o[c] = (i64)(nd.p ? round_p(z, q, nd.p) : z);
  }
}

// ---------------------------------------------------------------------------------------
// Matrix route.  Block = (right-slot group, 32 rows, 128 columns), one 32 x 32 tile of W i32 accumulators per wave.
// The depth K = n ell is walked in UNITS of 16 elements, two per v_mfma_i32_32x32x32_i8 (one per lane half): for
// ell < 16 a unit holds the digits of E = 16 / ell whole entries (elements past E ell are zero), for ell >= 16 an
// entry takes ceil(ell / 16) units.  Both operands follow this one order, so the sum pairs L[i][i2 ell + j] with digit
// j of entry i2 whatever order the instruction walks a half's 16 elements in.  Unit u covers the `cnt` consecutive
// depth indices from `start`:
//   left   the block stages 32 rows x 8 units: a thread loads its 16 words, y = (x + C) ^ C with C = 0x80 in each of the
//          W low bytes has limb w of x (balanced, [-128, 127]) as byte w; it writes one 16-byte row of limb w per w
//   right  the lane (column, half) peels the 16 digits of its unit into 4 VGPRs of int8
// Out-of-range rows, columns and depth indices contribute zeros or clamped loads; nothing out of range is stored.
// ---------------------------------------------------------------------------------------
struct Unit { int start, cnt, jd; };
__device__ __forceinline__ Unit unit_of(int u, int ell, int nch, int E, int n) {
  Unit r;
  if (nch > 1) {
    const int i2 = u / nch, ch = u - i2 * nch;
    r.jd = ch * 16;
    r.start = i2 * ell + r.jd;
    r.cnt = i2 < n ? (ell - r.jd < 16 ? ell - r.jd : 16) : 0;
  } else {
    const int K = n * ell, span = E * ell;
    r.jd = 0;
    r.start = u * span;
    r.cnt = r.start >= K ? 0 : (K - r.start < span ? K - r.start : span);
  }
  return r;
}

template <int W>
__global__ void __launch_bounds__(TPB)
k_lprf_node_mfma(const i64* __restrict__ Lv, const i64* __restrict__ Rv, i64* __restrict__ out, LprfNode nd, LprfMod md,
                 i64 mtiles) {
  __shared__ uint4 a_s[W][X_ST][X_TM][2];
  __shared__ const i64* lrow[X_TM];
  __shared__ i64* orow[X_TM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  const i64 g = blockIdx.x / mtiles, mt = blockIdx.x - g * mtiles;
  row_table<X_TM>(Lv, out, nd, g, mt * X_TM, lrow, orow);
  const i64 rs = child_slot((nd.full ? 0 : nd.lo) + g, nd.r);
  const int c = (int)blockIdx.y * X_TN + wave * 32 + r32;
  const bool cok = c < nd.K;
  const i64* rp = Rv + rs * (i64)nd.n * nd.K + (cok ? c : nd.K - 1);
  const u64 q = md.mc.q;
  const int ell = nd.ell;
  const int nch = ell > 16 ? (ell + 15) >> 4 : 1;
  const int E = ell > 16 ? 1 : 16 / ell;
  const int nunits = nch > 1 ? nd.n * nch : (nd.n + E - 1) / E;
  const int nsteps = (nunits + 1) >> 1;
  const u64 C = 0x8080808080808080ull >> (64 - 8 * W);
  v16i acc[W];
#pragma unroll
  for (int w = 0; w < W; ++w)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[w][e] = 0;
  const int srow = threadIdx.x >> 3, sstep = (threadIdx.x & 7) >> 1, shalf = threadIdx.x & 1;
  __syncthreads();
  for (int s0 = 0; s0 < nsteps; s0 += X_ST) {
    {                                                           // the left tile: row srow, unit (s0 + sstep, shalf)
      const Unit un = unit_of(2 * (s0 + sstep) + shalf, ell, nch, E, nd.n);
      const i64* src = lrow[srow] + un.start;
      u64 y[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) y[j] = j < un.cnt ? ((u64)src[j] + C) ^ C : 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        u32 pk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          pk[t] = (u32)((y[4 * t] >> (8 * w)) & 255) | (u32)((y[4 * t + 1] >> (8 * w)) & 255) << 8 |
                  (u32)((y[4 * t + 2] >> (8 * w)) & 255) << 16 | (u32)((y[4 * t + 3] >> (8 * w)) & 255) << 24;
        a_s[w][sstep][srow][shalf] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int st = 0; st < X_ST; ++st) {
      if (s0 + st >= nsteps) break;                             // block-uniform
      const Unit un = unit_of(2 * (s0 + st) + h, ell, nch, E, nd.n);
      u32 b[4] = {0, 0, 0, 0};
      int i2 = un.start / ell, jd = un.jd;
      i64 v = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (j < un.cnt) {
          if (jd == 0 || j == 0) {
            v = centred((u64)rp[(i64)i2 * nd.K], q);
            if (j == 0) for (int t = 0; t < jd; ++t) (void)peel(v, md);    // an entry's later unit: past its first digits
          }
          const i64 d = jd == ell - 1 ? v : peel(v, md);
          b[j >> 2] |= ((u32)d & 255u) << (8 * (j & 3));
          if (++jd == ell) { jd = 0; ++i2; }
        }
      }
      v4i bf;
      bf[0] = (int)b[0]; bf[1] = (int)b[1]; bf[2] = (int)b[2]; bf[3] = (int)b[3];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const uint4 a = a_s[w][st][r32][h];
        v4i af;
        af[0] = (int)a.x; af[1] = (int)a.y; af[2] = (int)a.z; af[3] = (int)a.w;
        acc[w] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf, acc[w], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // C/D map of the 32 x 32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    i64* o = orow[(e & 3) + 8 * (e >> 2) + 4 * h];
    if (!o || !cok) continue;
    u64 z = mod_any((i64)acc[W - 1][e], md.mc);
#pragma unroll
    for (int w = W - 2; w >= 0; --w) {
      const u128 t = ((u128)z << 8) + (u64)((i64)acc[w][e] + (i64)md.off);
      z = reduce128((u64)(t >> 64), (u64)t, md.mc);
    }
    o[c] = (i64)(nd.p ? round_p(z, q, nd.p) : z);
  }
}

hipError_t launch_lprf_node(hipStream_t s, const i64* L, const i64* R, i64* out, const LprfNode& nd, const LprfMod& md,
                            bool mfma, bool info) {
  if (nd.U <= 0) return hipSuccess;
  if (nd.R < 1 || nd.M < 1 || nd.n < 1 || nd.ell < 1 || nd.K != nd.n * nd.ell || (mfma && (md.W < 1 || md.W > 8)) ||
      (!mfma && md.fold < 0))
    return hipErrorInvalidValue;
  const i64 groups = nd.R < nd.U ? nd.R : nd.U;
  const i64 per = (nd.U + nd.R - 1) / nd.R;                     // slots per right slot
  const i64 rows = per * nd.M;
  const i64 mtiles = (rows + (mfma ? X_TM : V_TM) - 1) / (mfma ? X_TM : V_TM);
  const i64 gy = (nd.K + (mfma ? X_TN : V_TN) - 1) / (mfma ? X_TN : V_TN);
  if (groups > 0x7fffffff / mtiles || gy > 65535) return hipErrorInvalidValue;
  if (info)
    fprintf(stderr, "k_lprf: route %s, M %lld, N %d, K %d, W %d, slots %lld\n", mfma ? "mfma" : "valu", (long long)rows,
            nd.K, nd.K, mfma ? md.W : 0, (long long)nd.U);
  const dim3 grid((unsigned)(groups * mtiles), (unsigned)gy);
#define LOLHIP_X(WW) case WW: hipLaunchKernelGGL(k_lprf_node_mfma<WW>, grid, dim3(TPB), 0, s, L, R, out, nd, md, mtiles); break;
  if (mfma) {
    switch (md.W) { LOLHIP_X(1) LOLHIP_X(2) LOLHIP_X(3) LOLHIP_X(4) LOLHIP_X(5) LOLHIP_X(6) LOLHIP_X(7) LOLHIP_X(8) }
  } else if (md.fold == 0) {
    hipLaunchKernelGGL(k_lprf_node_valu<true>, grid, dim3(TPB), 0, s, L, R, out, nd, md, mtiles);
  } else {
    hipLaunchKernelGGL(k_lprf_node_valu<false>, grid, dim3(TPB), 0, s, L, R, out, nd, md, mtiles);
  }
#undef LOLHIP_X
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// out[slot][key][c] = sum_i s[key][i] A[slot][i][c] mod q: one thread per output word, c fastest
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB)
k_lprf_keymul(const i64* __restrict__ A, const i64* __restrict__ keys, i64* __restrict__ out, i64 total, int nkeys, int n,
              int K, i64 o_slot, i64 o_row, u64 p, ModCtx mc) {
  for (i64 g = (i64)blockIdx.x * TPB + threadIdx.x; g < total; g += (i64)gridDim.x * TPB) {
    const i64 sk = g / K;
    const int c = (int)(g - sk * K);
    const i64 slot = sk / nkeys;
    const int key = (int)(sk - slot * nkeys);
    const i64* a = A + slot * (i64)n * K + c;
    u64 z = 0;
    for (int i = 0; i < n; ++i) z = addmod(z, mulmod(mod_any(keys[(i64)key * n + i], mc), (u64)a[(i64)i * K], mc), mc.q);
    out[slot * o_slot + key * o_row + c] = (i64)(p ? round_p(z, mc.q, p) : z);
  }
}

hipError_t launch_lprf_keymul(hipStream_t s, const i64* A, const i64* keys, i64* out, i64 slots, int nkeys, int n, int K,
                              i64 o_slot, i64 o_row, u64 p, const ModCtx& mc) {
  const i64 total = slots * nkeys * K;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_lprf_keymul, dim3(grid_stride_blocks(total, TPB, MAX_BLOCKS)), dim3(TPB), 0, s, A, keys, out,
                     total, nkeys, n, K, o_slot, o_row, p, mc);
  return hipGetLastError();
}

}  // namespace lolhip
