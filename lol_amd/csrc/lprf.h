// lol_amd/csrc/lprf.h — host interface of lprf.hip, the kernels of the key-homomorphic lattice PRF (lol-apps
// KeyHomomorphicPRF.hs latticePRF'; include/lolhip.h lolhip_lprf_*).  One modulus; every matrix is a
// row-major int64 slab of residues in [0, q).
#pragma once
#include <hip/hip_runtime_api.h>

#include "pipeline.h"

namespace lolhip {

// what every launch of a family shares
struct LprfMod {
  ModCtx mc;
  DecompParams dp;             // T = 1, k[0] = ell
  int lg;                      // log2 base when base is a power of two (the digits come from shifts), else -1
  int fold;                    // VALU route: terms per signed 64-bit lazy sum, 0 = 128-bit sums of residues (folded every 8)
  int W;                       // matrix route: balanced base-256 limbs of a residue, 0 = not admitted
  u64 off;                     // matrix route: the multiple of q in [2^31, 2^31 + q) that makes an i32 sum non-negative
};

// One node product over a window, slots as in khprf.hip (KhprfChild, the slot scheme of lolhip_khprf_eval_batch):
//   out[slot k][row i][c] = sum_{i2 < n, j < ell} L[slot_l(k)][i][i2 ell + j] * digit_j(R[slot_r(k)][i2][c]) mod q
// L [U_l][M][K], R [U_r][n][K] (a leaf child: the family's [2][n][K]); out row i of slot k at k o_slot + i o_row.
struct LprfNode {
  i64 U;                       // slots of v (the root: B, slot k = input x0 + k)
  i64 lo;                      // x0 >> s_v
  int full;                    // U = 2^c_v: slot k stands for w_v = k, else for lo + k
  int n, ell, M, K;            // M rows per left slot: n, or nkeys at a keyed root; K = n ell
  i64 R;                       // slots k, k + R, ... share one right slot (2^c_r for a full right child, else U)
  i64 o_slot, o_row;
  u64 p;                       // 0: residues mod q; else y = fst (divModCent (p lift z) q) mod p in the write-back
  KhprfChild l, r;
};
// mfma: the matrix route (needs md.W > 0); info: print the launch's line to stderr
hipError_t launch_lprf_node(hipStream_t s, const i64* L, const i64* R, i64* out, const LprfNode& nd, const LprfMod& md,
                            bool mfma, bool info);

// out[slot][key][c] = sum_i s[key][i] A[slot][i][c] mod q (s any int64), rounded to Z_p for p != 0;
// A [slots][n][K], out row `key` of slot at slot o_slot + key o_row
hipError_t launch_lprf_keymul(hipStream_t s, const i64* A, const i64* keys, i64* out, i64 slots, int nkeys, int n, int K,
                              i64 o_slot, i64 o_row, u64 p, const ModCtx& mc);

}  // namespace lolhip
