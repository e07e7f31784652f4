// lol_amd/csrc/gadget.h — launcher interface of gadget.hip: gadget error correction (class Correct) and Gadget.encode
// plus noise, as gadget_api.cpp launches them.
#pragma once
#include <hip/hip_runtime_api.h>

#include "pipeline.h"

namespace lolhip {

constexpr int GADGET_MAX_T = 2;    // Correct is an instance of fields and of pairs of fields (Gadget.hs:104-134)

// Everything k_gadget_correct needs beside the plan's ModCtx, by value in the launch.  Component t corrects its own
// block of d.k[t] entries over q_t; `o` is the other component of a pair.
struct CorrectParams {
  DecompParams d;                  // T, L, base, the digit counts and the invariant-divisor constants of base
  u64 g[GADGET_MAX_T];             // b^(k_t - 1), the last gadget entry over the integers (1 for TrivGad and k_t = 1)
  u64 gmagic[GADGET_MAX_T];        // the invariant-divisor constants of g[t], as DecompParams states them for base
  int gsh1[GADGET_MAX_T], gsh2[GADGET_MAX_T];
  u64 qo[GADGET_MAX_T];            // q_o, the factor of the block's errors (1 for a single modulus)
  u64 qo_mod[GADGET_MAX_T];        // q_o mod q_t
  u64 qo_inv[GADGET_MAX_T];        // q_o^-1 mod q_t
};

// k_gadget_correct: xs [L][rows][T] (any int64, taken mod q_t), decoding basis -> u [rows][T] in [0, q_t) and, when es
// is not null, es [L][rows] int64.  One thread per row.  u and es must not overlap xs.
hipError_t launch_gadget_correct(hipStream_t s, const i64* xs, i64* u, i64* es, i64 rows, const CorrectParams& p,
                                 const ModCtx* mod);
// k_gadget_encode: sv [rows][T], e [L][rows] int64 or null -> out [L][rows][T] = g_j s + reduce (e_j) in [0, q_t)
hipError_t launch_gadget_encode(hipStream_t s, const i64* sv, const i64* e, i64* out, i64 rows, const DecompParams& p,
                                const ModCtx* mod);

}  // namespace lolhip
