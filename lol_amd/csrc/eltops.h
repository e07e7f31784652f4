// lol_amd/csrc/eltops.h — launcher interface of eltops.hip: L, L^-1, mulG and divG in both bases over slabs of int64
// (arithmetic mod 2^64) and of doubles (every IEEE operation rounded on its own), and mulC (l.cpp, g.cpp,
// types.h:146-152 of the reference).  Used by eltops_api.cpp only.
#pragma once
#include <hip/hip_runtime_api.h>

#include "rlwe.h"

namespace lolhip {

constexpr i64 ELT_MAX_N = 16384;
constexpr int ELT_MAX_T = 16;
constexpr size_t ELT_LDS_BYTES = 160 * 1024;   // LDS of one CU: the on-chip route holds whole items there

enum EltOp { ELT_L = 0, ELT_LINV = 1, ELT_MULGPOW = 2, ELT_MULGDEC = 3, ELT_DIVGPOW = 4, ELT_DIVGDEC = 5, ELT_NOPS = 6 };

// y [B][n][W] words in place, W words per coefficient (T, or 2 T for complex).  f64: the words are doubles, else uint64
// that wrap.  nd: the odd primes of the index (she_host.h norm_dims), nd.k >= 1.  oddrad: their product.  ok [B]: the
// divisibility flags of divG over uint64 (read as int64), unused otherwise.  global: one pass per odd prime straight
// from HBM instead of the one launch over LDS-resident items (required when !elt_fits_lds).
struct EltLaunch {
  hipStream_t stream;
  void* y;
  int32_t* ok;
  i64 B, n;
  int W;
  bool f64;
  int op;
  NormDims nd;
  i64 oddrad;
  bool global;
};
// bytes of LDS one item of n W words takes on the on-chip route (one pad word after every 32, and 128 bytes of item
// flags), and whether they fit
size_t elt_lds_bytes(i64 n, int W);
inline bool elt_fits_lds(i64 n, int W) { return elt_lds_bytes(n, W) <= ELT_LDS_BYTES; }
hipError_t launch_elt(const EltLaunch& a);
// ok[b] = 1, b < B (divG over int64 at m = 2^k)
hipError_t launch_elt_ok(hipStream_t s, int32_t* ok, i64 B);

// a[i] *= b[i] over count complex doubles (re, im); b may equal a
hipError_t launch_mulc(hipStream_t s, double* a, const double* b, i64 count);

}  // namespace lolhip
