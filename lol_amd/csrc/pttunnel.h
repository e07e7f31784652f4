// lol_amd/csrc/pttunnel.h — the kernels of the clear-text tunnel and of crtSet's powering (pttunnel.hip), as
// pttunnel_api.cpp launches them.
#pragma once
#include <hip/hip_runtime_api.h>

#include "zq_dev.h"

namespace lolhip {

// k_relift: the pass between two exact integer computations mod NTT primes on values that live mod pe = p^e.
//   Qin != 0: x in (-Qin, Qin) -> v = its centred lift mod Qin -> r = v mod pe;   Qin == 0: r = x mod pe, any int64 x
//   res  (may be null): r in [0, pe)
//   lift (may be null): the centred lift of r mod pe ([-pe/2, pe/2) for even pe), reduced into [0, Qout)
// Either output may alias src: every word is read and written by one thread.
struct Relift {
  u64 Qin, Qout;
  ModCtx pe;      // the modulus p^e
  int pebits;     // k when pe = 2^k, else 0
};
hipError_t launch_relift(hipStream_t s, const i64* src, i64* res, i64* lift, i64 total, const Relift& c);

// out[r][i] = idx[i] < 0 ? 0 : in[r][idx[i]]  for r < rows: embedPow of `rows` one-modulus polynomials
hipError_t launch_embed_rows(hipStream_t s, const i64* in, i64* out, const int32_t* idx, i64 rows, i64 n_in, i64 n_out);

}  // namespace lolhip
