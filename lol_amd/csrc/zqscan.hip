// lol_amd/csrc/zqscan.hip — the prime ops' stage programs (L, L^-1, mulG, divG over Z_q) at a prime above 13, for plans
// created with LOLHIP_ROUTE_SCAN_ZQ.
//
// Every stage of these programs is a prefix sum, a total or a neighbour difference along vectors of d = p - 1 elements
// at stride rts.  The scalar interpreter (k_generic, kernels.hip) computes each output element on its own, which costs
// up to d modular additions and strided LDS reads per output for L, divGPow and divGDec.  Here a workgroup holds a TILE
// of polynomials of one RNS component in LDS (the tile contract of zqdense.hip) and every stage runs IN PLACE on it.
// For a stage the tile is an array of blocks of d * rts words, element (i, r) of a block at word i * rts + r:
//
//   lanes (stride below a wave)   a wave reads 64 consecutive words of a block: SP = min(d, 64 / rts) steps of the
//         recurrence times rts columns (lanes past SP * rts idle).  It scans across lanes with shifts of rts, 2 rts,
//         4 rts, ... and carries the last step's row into the next round.  A block of at most 32 words shares the wave
//         with its neighbours: the scan's condition is on the step index, so it never crosses a block.
//   cols  (stride of at least a wave)   a lane owns one column and walks its d steps; consecutive lanes read
//         consecutive words.
//
// Per vector a stage needs the inclusive prefix sums P_i, for mulGDec / divG the total S and for divGDec the weighted
// total W = sum (c + 1) v_c; S and W take a reduction pass before the scan pass.  What is stored at element i is
// stage_eval's own expression of (v_i, v_(i-1), P_i, S, W, v_(d-1)) (generic_dev.h), then the stage's diagonal.
// Residues are canonical everywhere and modular addition is associative and exact, so the result is the scalar
// interpreter's, bit for bit.  Ranges: sums of two residues stay below 2^63 (q < 2^62); with 4-byte words W accumulates
// lazily, at most 8190 terms of less than 8191 * 2^32, below 2^58, and is reduced once; with 8-byte words every term is a
// modular product.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "kernels.h"
#include "tile_dev.h"

namespace lolhip {

namespace {

constexpr int ZS_MAX_TPB = 512;          // two workgroups of a 64 KiB tile per CU, at the kernel's 4 waves per SIMD
constexpr size_t ZS_TILE_BYTES = 64 * 1024;       // two workgroups per CU; within ZQ_LDS_BUDGET
static_assert(ZS_TILE_BYTES <= ZQ_LDS_BUDGET, "the tile must fit the dynamic LDS of a workgroup");

// what the stage stores at element i of a vector: v the input there, prev the input one step below (unused at i = 0),
// P the inclusive prefix sum, S the total, W the weighted total, last the input at d - 1: stage_eval's expressions
template <bool Q32>
__device__ __forceinline__ u64 zs_out(int kind, int p, int i, u64 v, u64 prev, u64 P, u64 S, u64 W, u64 last, const ModCtx& mc) {
  const u64 q = mc.q;
  switch (kind) {
    case ST_L: return P;
    case ST_LINV: return i == 0 ? v : submod(v, prev, q);
    case ST_GPOW: {
      const u64 o = addmod(v, last, q);
      return i > 0 ? submod(o, prev, q) : o;
    }
    case ST_GDEC: return i > 0 ? submod(v, prev, q) : addmod(S, v, q);
    case ST_GINVPOW:
      return submod(gmul<Q32>(smallmod((u64)(p - 1 - i), q), P, mc), gmul<Q32>(smallmod((u64)(i + 1), q), submod(S, P, q), mc), q);
    default:      // ST_GINVDEC
      return submod(W, gmul<Q32>(smallmod((u64)p, q), submod(S, P, q), mc), q);
  }
}

// one term (c + 1) v_c of the weighted total.  Q32: lazy, c + 1 <= 8190 and v < 2^32, at most 8190 terms: below 2^58
template <bool Q32> __device__ __forceinline__ void zs_wadd(u64& acc, int c1, u64 v, const ModCtx& mc) {
  if constexpr (Q32) acc += (u64)(u32)c1 * (u32)v;
  else acc = addmod(acc, mulmod(smallmod((u64)c1, mc.q), v, mc), mc.q);
}
template <bool Q32> __device__ __forceinline__ u64 zs_wfin(u64 acc, const ModCtx& mc) {
  if constexpr (Q32) return rem128(0, acc, mc); else return acc;
}

template <typename Wd>
__device__ __forceinline__ void zs_cols(const Stage& st, Wd* __restrict__ buf, int n, int items, const u64* __restrict__ cst,
                                        const ModCtx& mc) {
  constexpr bool Q32 = sizeof(Wd) == 4;
  const int d = st.d, rts = st.rts, kind = st.kind, p = st.p;
  const int ncols = items * (n / d);                     // block b of the tile, column r of it: col = b * rts + r
  const u64 m_n = magic40_dev(n), q = mc.q;
  const bool totals = kind == ST_GDEC || kind == ST_GINVPOW || kind == ST_GINVDEC;
  for (int col = threadIdx.x; col < ncols; col += blockDim.x) {
    const int b = fdiv40(col, st.m_rts), r = col - b * rts;
    const int base = b * d * rts + r;
    u64 S = 0, W = 0, last = 0;
    if (totals) {
      u64 wacc = 0;
      for (int c = 0; c < d; ++c) {
        const u64 v = buf[base + c * rts];
        S = addmod(S, v, q);
        if (kind == ST_GINVDEC) zs_wadd<Q32>(wacc, c + 1, v, mc);
      }
      W = zs_wfin<Q32>(wacc, mc);
    }
    if (kind == ST_GPOW) last = buf[base + (d - 1) * rts];      // before anything of the vector is overwritten
    u64 P = 0, prev = 0;
    for (int i = 0; i < d; ++i) {
      const u64 v = buf[base + i * rts];
      P = addmod(P, v, q);
      zq_put(st, buf, base + i * rts, zs_out<Q32>(kind, p, i, v, prev, P, S, W, last, mc), n, m_n, cst, mc);
      prev = v;
    }
  }
}

// cross-lane moves in the width of the tile's word: residues (and 4-byte sums reduced below q) fit it
template <typename Wd> __device__ __forceinline__ u64 zs_up(u64 x, int delta) { return (u64)__shfl_up((Wd)x, (unsigned)delta, 64); }
template <typename Wd> __device__ __forceinline__ u64 zs_from(u64 x, int lane) { return (u64)__shfl((Wd)x, lane, 64); }
// inclusive sums over the steps j = 0 .. SP - 1 of a round, every column of every block of the wave at once: the lane
// delta below holds the same column one step down, and a lane with j >= s has s steps of its own block below it.
// U independent values go through the steps together: a step is a cross-lane move and a dependent addition, and a wave
// that follows one chain waits out the latency of each
template <typename Wd, int U> __device__ __forceinline__ void zs_scan(u64 (&x)[U], int j, int SP, int rts, u64 q) {
  for (int s = 1; s < SP; s <<= 1) {
    u64 y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) y[u] = zs_up<Wd>(x[u], s * rts);
    if (j >= s) {
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = addmod(x[u], y[u], q);
    }
  }
}

constexpr int ZS_U = 4;        // blocks (groups of short blocks) a wave takes through a stage together

template <typename Wd>
__device__ __forceinline__ void zs_lanes(const Stage& st, Wd* __restrict__ buf, int n, int items, const u64* __restrict__ cst,
                                         const ModCtx& mc) {
  constexpr bool Q32 = sizeof(Wd) == 4;
  constexpr int U = ZS_U;
  const int d = st.d, rts = st.rts, kind = st.kind, p = st.p;
  const int R = 64 / rts;                        // steps of the recurrence a wave holds (rts < 64)
  const int SP = d < R ? d : R;                  // steps per round
  const int seg = SP * rts;                      // lanes of one block in a round
  const int G = d <= R ? 64 / seg : 1;           // whole blocks side by side when one round takes a block
  const int rounds = (d + SP - 1) / SP;          // 1 when G > 1
  const int blkw = d * rts, nblocks = items * (n / blkw), ngroups = (nblocks + G - 1) / G;
  const int lane = (int)(threadIdx.x & 63);
  const int g = lane / seg, w = lane - g * seg, j = w / rts, r = w - j * rts;
  const bool live = g < G;
  const int top = live ? g * seg + (SP - 1) * rts + r : lane;      // the lane of the round's last step in this lane's column
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nwaves = (int)(blockDim.x >> 6);
  const u64 m_n = magic40_dev(n), q = mc.q;
  const bool totals = kind == ST_GDEC || kind == ST_GINVPOW || kind == ST_GINVDEC;
  // as many together as leave every wave of the workgroup something to do
  const int per = ngroups >= nwaves * U ? U : ngroups > nwaves ? (ngroups + nwaves - 1) / nwaves : 1;
  for (int w0 = wave * per; w0 < ngroups; w0 += nwaves * per) {  // wave-uniform: every lane takes part in every shuffle
    bool ok[U];
    int base[U];                                                 // round k: + k * seg
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int b = (w0 + u) * G + g;
      ok[u] = live && u < per && w0 + u < ngroups && b < nblocks;
      base[u] = b * blkw + w;
    }
    u64 S[U], W[U], last[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { S[u] = 0; W[u] = 0; last[u] = 0; }
    if (totals) {
      u64 wacc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) wacc[u] = 0;
      for (int k = 0; k < rounds; ++k) {
        const int i = k * SP + j;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (ok[u] && i < d) {
            const u64 v = buf[base[u] + k * seg];
            S[u] = addmod(S[u], v, q);
            if (kind == ST_GINVDEC) zs_wadd<Q32>(wacc[u], i + 1, v, mc);
          }
      }
      zs_scan<Wd, U>(S, j, SP, rts, q);
#pragma unroll
      for (int u = 0; u < U; ++u) S[u] = zs_from<Wd>(S[u], top);
      if (kind == ST_GINVDEC) {
#pragma unroll
        for (int u = 0; u < U; ++u) W[u] = zs_wfin<Q32>(wacc[u], mc);
        zs_scan<Wd, U>(W, j, SP, rts, q);
#pragma unroll
        for (int u = 0; u < U; ++u) W[u] = zs_from<Wd>(W[u], top);
      }
    }
    if (kind == ST_GPOW) {                                       // before anything of the vector is overwritten
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u]) last[u] = buf[base[u] - w + (d - 1) * rts + r];
    }
    u64 carry[U], pv[U];                                         // the prefix sum and the input at the last step of the round before
#pragma unroll
    for (int u = 0; u < U; ++u) { carry[u] = 0; pv[u] = 0; }
    for (int k = 0; k < rounds; ++k) {
      const int i = k * SP + j;
      u64 v[U], P[U], prev[U];
#pragma unroll
      for (int u = 0; u < U; ++u) P[u] = v[u] = (ok[u] && i < d) ? (u64)buf[base[u] + k * seg] : 0;
      zs_scan<Wd, U>(P, j, SP, rts, q);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        P[u] = addmod(P[u], carry[u], q);
        prev[u] = zs_up<Wd>(v[u], rts);
        if (j == 0) prev[u] = pv[u];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u] && i < d)
          zq_put(st, buf, base[u] + k * seg, zs_out<Q32>(kind, p, i, v[u], prev[u], P[u], S[u], W[u], last[u], mc), n, m_n, cst, mc);
      if (k + 1 < rounds) {
#pragma unroll
        for (int u = 0; u < U; ++u) { carry[u] = zs_from<Wd>(P[u], top); pv[u] = zs_from<Wd>(v[u], top); }
      }
    }
  }
}

struct ZsArgs {
  i64* y;
  const i64* src;                // never null: y for an in-place launch
  i64 B, ntiles;
  int T, n, nstages, cpc, items;
  const Stage* stages;
  const u64* consts;
  const ModCtx* mod;
  uint8_t kind[ZQ_MAX_STAGES];
};

// One work item = (tile of `items` polynomials, component t), grid-strided.  One LDS buffer of items * n words: every
// stage runs in place.  A partial tile loads, computes and stores its live items only.  Everything of a tile is loaded
// before anything is stored and tiles are disjoint, so y may alias src.
template <typename Wd>
__global__ void __launch_bounds__(ZS_MAX_TPB)
k_zq_scan(const ZsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool Q32 = sizeof(Wd) == 4;
  const int n = a.n, T = a.T;
  const i64 nwork = a.ntiles * T;
  const u64 m_n = magic40_dev(n);
  Wd* buf = reinterpret_cast<Wd*>(smem);
  for (i64 wk = blockIdx.x; wk < nwork; wk += gridDim.x) {
    const i64 tile = wk / T;
    const int t = (int)(wk - tile * T);
    const i64 b0 = tile * a.items;
    const int live = (int)(a.B - b0 < a.items ? a.B - b0 : a.items);
    const int tot = live * n;
    const ModCtx mc = a.mod[t];
    const u64* __restrict__ cst = a.consts + (size_t)t * a.cpc;
    const i64* in = a.src + (size_t)b0 * n * T + t;
    for (int x = threadIdx.x; x < tot; x += blockDim.x) buf[x] = (Wd)canon_in(in[(size_t)x * T], mc.q);
    __syncthreads();
    for (int s = 0; s < a.nstages; ++s) {
      const Stage st = a.stages[s];
      int kind = ZS_ELT;
#pragma unroll
      for (int k = 0; k < ZQ_MAX_STAGES; ++k)      // constant indices: the array stays in the kernel's argument segment
        if (k == s) kind = a.kind[k];
      if (kind == ZS_ELT) {                          // a diagonal: element x depends on element x alone
        for (int x = threadIdx.x; x < tot; x += blockDim.x) {
          const int pi = fdiv40(x, m_n), xi = x - pi * n;
          buf[x] = (Wd)stage_eval<true, Q32, Wd>(st, buf + pi * n, xi, cst, mc);
        }
      } else if (kind == ZS_LANES) {
        zs_lanes<Wd>(st, buf, n, live, cst, mc);
      } else {
        zs_cols<Wd>(st, buf, n, live, cst, mc);
      }
      __syncthreads();
    }
    i64* out = a.y + (size_t)b0 * n * T + t;
    for (int x = threadIdx.x; x < tot; x += blockDim.x) out[(size_t)x * T] = (i64)(u64)buf[x];
    __syncthreads();
  }
}

const char* zs_kind_name(int kind) {
  switch (kind) {
    case ST_L: return "l";
    case ST_LINV: return "linv";
    case ST_GPOW: return "gpow";
    case ST_GDEC: return "gdec";
    case ST_GINVPOW: return "ginvpow";
    case ST_GINVDEC: return "ginvdec";
    default: return "diag";
  }
}

}  // namespace

hipError_t launch_zq_scan(const GenericLaunch& g) {
  const ZqScanLaunch& z = g.scan;
  if (g.B == 0 || g.nstages == 0) return hipSuccess;
  if (z.route != 1 || g.nstages > ZQ_MAX_STAGES || g.n < 1 || g.n > 8192 || !z.host_stages) return hipErrorInvalidValue;
  for (int i = 0; i < g.nstages; ++i) {            // what the kernel's index arithmetic relies on
    const Stage& st = z.host_stages[i];
    if (z.kind[i] == ZS_ELT) {
      if (st.kind != ST_DIAG && st.kind != ST_SCALE) return hipErrorInvalidValue;
      continue;
    }
    if (!zq_scan_stage(st) || st.d < 1 || st.rts < 1 || g.n % ((i64)st.d * st.rts) != 0) return hipErrorInvalidValue;
    if ((z.kind[i] == ZS_COLS) != lanes_along_r(st) || z.kind[i] > ZS_COLS) return hipErrorInvalidValue;
  }
  const size_t word = g.q32 ? 4 : 8;
  // The tile: as many items as 64 KiB of LDS hold (two workgroups per CU), but no more than leave about 512 tiles to the
  // batch, and no fewer than make 1024 words (four for each of a workgroup's 256 threads); n = 8192 at 8-byte words is
  // one item of exactly 64 KiB.
  const size_t per = (size_t)g.n * word;
  const i64 items = tile_items(g.B, (i64)(ZS_TILE_BYTES / per), 1, (1024 + g.n - 1) / g.n);
  const size_t lds = per * (size_t)items;
  // a workgroup whose tile fills its share of a CU's LDS should also fill its share of the SIMDs
  const int threads = items * g.n >= 4096 ? ZS_MAX_TPB : 256;
  const i64 ntiles = (g.B + items - 1) / items;
  i64 grid = ntiles * g.T;
  if (grid > 65536) grid = 65536;                 // as launch_generic caps
  if (const char* e = getenv("LOLHIP_ZQ_SCAN_GRID")) {
    const long v = atol(e);
    grid = v < 1 ? 1 : (v > 65536 ? 65536 : v);
  }
  if (getenv("LOLHIP_ZQ_SCAN_INFO")) {
    char line[1024];
    const int at = snprintf(line, sizeof(line), "k_zq_scan: n %lld, B %lld, T %d, word %zu, items %lld, lds %zu B, grid %lld, threads %d, stages",
                            (long long)g.n, (long long)g.B, g.T, word, (long long)items, lds, (long long)grid, threads);
    static const char* const layouts[3] = {"elt", "lanes", "cols"};
    tile_info(line, at, g.nstages, [&](char* p, size_t room, int i) {
      const Stage& st = z.host_stages[i];
      return snprintf(p, room, " %s:%d:%d:%d:%s", zs_kind_name(st.kind), st.p, st.d, st.rts, layouts[z.kind[i]]);
    });
  }
  ZsArgs a;
  a.y = g.y; a.src = z.src ? z.src : g.y; a.B = g.B; a.ntiles = ntiles;
  a.T = g.T; a.n = (int)g.n; a.nstages = g.nstages; a.cpc = g.cpc; a.items = (int)items;
  a.stages = g.stages; a.consts = g.consts; a.mod = g.mod;
  for (int i = 0; i < ZQ_MAX_STAGES; ++i) a.kind[i] = i < g.nstages ? z.kind[i] : (uint8_t)ZS_ELT;
  if (g.q32) hipLaunchKernelGGL((k_zq_scan<u32>), dim3((unsigned)grid), dim3((unsigned)threads), lds, g.stream, a);
  else hipLaunchKernelGGL((k_zq_scan<u64>), dim3((unsigned)grid), dim3((unsigned)threads), lds, g.stream, a);
  return hipGetLastError();
}

}  // namespace lolhip
