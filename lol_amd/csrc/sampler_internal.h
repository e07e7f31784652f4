// lol_amd/csrc/sampler_internal.h — what the host translation units of the SymmSHE samplers share (encrypt_api.cpp,
// kshint_api.cpp): the sampler's limits, the deviation of tGaussianDec, the key words and the launch plan of one
// batch of rounded Gaussians.  Not part of the public interface.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "kernels.h"
#include "rng_dev.h"
#include "she_host.h"

namespace lolhip {

constexpr int64_t SAMPLER_POW2_MAX_N = 16384;   // 2-powers: no map, one fused pass (k_enc_error from the stream)

// every prime of the index is 2 (m' = 2^k, or 1): L and the Gaussian map are identities
inline bool two_power(const Plan& P) {
  for (const PP& pe : P.pps) if (pe.p != 2) return false;
  return true;
}

// LOLHIP_OK when the sampler takes this index: a 2-power up to n' = 16384, else the limits of the Gaussian map
inline int sampler_ok(const Plan& P) {
  if (two_power(P)) return P.n <= SAMPLER_POW2_MAX_N ? LOLHIP_OK : LOLHIP_ERR_INVALID;
  return P.gauss_route ? LOLHIP_OK : LOLHIP_ERR_INVALID;
}

// The limit is a property of the plan's prime powers and flags alone, so the sampler entries that ask for the device
// first (encrypt, errorRounded, ksHint) answer it before that: a host-only plan tells an index it will never take
// (LOLHIP_ERR_INVALID) from one that only lacks a device.  A null plan is left to the caller's own check.
inline int index_status(const lolhip_plan* p) { return p ? sampler_ok(p->P) : LOLHIP_OK; }

// sigma = sqrt(v (m'/rad m') / 2 pi): the deviation of tGaussianDec v (scaled variance = 2 pi x variance,
// GaussRandom.hs:27-44; CPP.hs:376-389)
inline double deviation(const Plan& P, double v) {
  double mrad = 1.0;
  for (const PP& pe : P.pps)
    for (int i = 1; i < pe.e; ++i) mrad *= pe.p;
  return std::sqrt(v * mrad / 6.283185307179586);
}

inline ChaChaKey make_key(const uint8_t key[32]) {
  ChaChaKey k;
  for (int i = 0; i < 8; ++i)
    k.k[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 |
             (uint32_t)key[4 * i + 3] << 24;
  return k;
}

inline bool svar_ok(double svar) { return std::isfinite(svar) && svar > 0; }

// the double slab of the map and the sampled coefficients into [B][n] int64 / residues: one pass from the stream for a
// 2-power, else Gaussians -> k_gauss (the decoding-basis map of tGaussianDec) -> the rounding pass
inline int sample_error(const Plan& P, hipStream_t s, double* d, const int64_t* rep, int64_t p, int64_t* out, int mode,
                        const ChaChaKey& key, uint64_t ctr, int domain, double sigma, int64_t B) {
  if (two_power(P))
    return hip_status(launch_enc_error(s, nullptr, rep, p, out, B, P.n, P.T, P.d_mod, mode, key, ctr, domain, sigma));
  if (launch_enc_gauss(s, d, B, P.n, key, ctr, domain, sigma) != hipSuccess) return LOLHIP_ERR_HIP;
  if (launch_gauss(s, d, B, P.n, P.prog_gauss.d_stages, P.gauss_word, P.d_rconsts) != hipSuccess)
    return LOLHIP_ERR_HIP;
  return hip_status(launch_enc_error(s, d, rep, p, out, B, P.n, P.T, P.d_mod, mode, key, ctr, domain, sigma));
}

}  // namespace lolhip
