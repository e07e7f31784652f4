// lol_amd/csrc/rlwe_ring.h — launcher interface of rlwe_ring.hip: the passes of RLWE / RLWR instances over moduli
// without a CRT basis that ringmul.hip, rlwe.hip and encrypt.hip do not already provide.  Used by
// rlwe_ring_api.cpp only.  One modulus: the RingMul constants have T = 1.
#pragma once
#include <hip/hip_runtime_api.h>

#include "ringmul.h"
#include "rng_dev.h"

namespace lolhip {

// k_rr_draw_lift: a_pow [B][n] = the uniform residues of `domain` at items ctr + b (4 per ChaCha20 block: the words
// launch_rlwe_uniform writes over one modulus q), and la [B][n][K] = the K residues of their centred lifts, which are
// what launch_ring_lift makes of a_pow.  One pass.
hipError_t launch_rr_draw_lift(hipStream_t s, i64* a_pow, i64* la, i64 B, i64 n, const RingMul& c, const ChaChaKey& key,
                               u64 ctr, int domain);

// The tails of k_rr_fold.  f = the fold of k_ring_fold: la [B][n][K] -> the residue in [0, q).
//   ADD          out i64 = (f + in) mod q              in: residues in [0, q)
//   SUB          out i64 = (in - f) mod q              in: any int64, taken mod q
// and, for an index where the powerful and decoding bases coincide (a 2-power), the rest of a whole call:
//   DISC_SAMPLE  out i64 = (f + round g) mod q         g: the Gaussian of domain 6 drawn in the pass (k_enc_error's)
//   DISC_ERROR   out i64 = the centred lift of (in - f) mod q
//   CONT_SAMPLE  out f64 = f + reduce' g in RRq        (k_rlwe_cont<false> on (f, g), g as k_enc_gauss draws it)
//   CONT_ERROR   out f64 = lift (in + reduce' (-f))    in: doubles (k_rlwe_cont<true>)
//   RLWR         out i64 = the rounding of f to [0, p) (k_rlwr_round)
enum { RR_ADD = 0, RR_SUB, RR_DISC_SAMPLE, RR_DISC_ERROR, RR_CONT_SAMPLE, RR_CONT_ERROR, RR_RLWR, RR_TAILS };

// what the tails read beside la, by value in the launch
struct RrTail {
  ChaChaKey key;      // the Gaussian tails
  u64 ctr;
  double sigma;
  u64 p;              // RR_RLWR
};

// in and out [B][n] words (int64 or double as the tail says); in is null for the tails without an input.  la, in and
// out must not overlap.
hipError_t launch_rr_fold(hipStream_t s, int tail, const i64* la, const void* in, void* out, i64 B, i64 n,
                          const RingMul& c, const RrTail& t);

// e = the centred lift mod q of residues x in (-q, q), [total]; e may be x
hipError_t launch_rr_centre(hipStream_t s, const i64* x, i64* e, i64 total, u64 q);

}  // namespace lolhip
