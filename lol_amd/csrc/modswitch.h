// lol_amd/csrc/modswitch.h — launcher interface of modswitch.hip: the coefficient-wise part of a ciphertext's
// modSwitch (lol-apps SymmSHE.hs:236-246; lol Prelude.hs:227-232, 274-308).  Slabs are [.][n][T] int64, component t
// innermost.
#pragma once
#include <hip/hip_runtime_api.h>

#include "pipeline.h"

namespace lolhip {

constexpr int MODSW_MAX_D = 5;   // moduli one call drops or adds (the reference's RescaleCyc instances, Cyc.hs:546-582)

// Every constant of the pass, by value.  Shoup pairs (w, floor(w 2^64 / q_t)), w < q_t.
struct ModSwitchParams {
  int T;                                   // input components
  int d;                                   // leading components dropped (0..5); To = T - d + u
  int u;                                   // leading zero components added (0..5; d == 0 then)
  int scaled;                              // 1: every input residue is multiplied by s[t] first
  u64 q[PIPE_MAX_T];                       // input moduli
  u64 s[PIPE_MAX_T], sp[PIPE_MAX_T];       // the input scale: toMSD's p^-1 mod q_t, times the product of the added moduli
  u64 inv[MODSW_MAX_D][PIPE_MAX_T];        // q_i^-1 mod q_t, i < d, t > i
  u64 invp[MODSW_MAX_D][PIPE_MAX_T];
};

// rows coefficient rows: row r of the input is in0 + r T for r < rows0, in + r T after (component 0 of a ciphertext
// may live in another buffer); out + r To.  Inputs in (-q_t, q_t), outputs canonical.  out overlaps no input.
hipError_t launch_modswitch(hipStream_t s, const i64* in0, i64 rows0, const i64* in, i64* out, i64 rows,
                            const ModSwitchParams& p);

}  // namespace lolhip
