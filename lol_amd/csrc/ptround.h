// lol_amd/csrc/ptround.h — launcher interface of ptround.hip: the ciphertext product of HomomPRF's ptRound with both
// affine pre-steps folded in (lol-apps HomomPRF.hs:232-270, SymmSHE.hs:381-390, 444-449).  Slabs are [.][B][n'][T]
// int64, component t innermost, CRT basis.
#pragma once
#include <hip/hip_runtime_api.h>

#include "public.h"

namespace lolhip {

// For every pair j < npairs, with a = a + j a_pair and b = b + j b_pair two linear ciphertexts [2][B][n'][T]
// (slab = B n' T words per component) and va_j = va + j n' T, vb_j = vb + j n' T polynomials [n'][T] shared by the batch
// (va / vb null: zero):
//   A0 = alpha_t a_0 + va_j,  A1 = alpha_t a_1;   B0 = beta_t b_0 + vb_j,  B1 = beta_t b_1
//   out_j = (g A0 B0, g (A0 B1 + A1 B0), g A1 B1),  out [npairs][3][B][n'][T], g = gcrt [n'][T]
// alpha_t / beta_t: the Shoup pairs sc.a / sc.b.  a_pair = b_pair = 0 fans one ciphertext out over the pairs; a and b
// may be the same pointer.  Inputs in (-q_t, q_t), outputs canonical.  out may alias a or b when npairs = 1.
hipError_t launch_ct_affine_mul(hipStream_t s, const i64* a, i64 a_pair, const i64* va, const i64* b, i64 b_pair,
                                const i64* vb, int npairs, i64* out, i64 B, i64 n, const PubScales& sc, const i64* gcrt,
                                const ModCtx* mod);

}  // namespace lolhip
