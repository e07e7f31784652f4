// lol_amd/csrc/rng_dev.h — the ChaCha20 block function (RFC 8439 §2.3) and the stream layout of the SymmSHE
// samplers (encrypt.hip, kshint.hip), one source for the kernels and the host inspection entry lolhip_chacha20_block.
//
// The reference draws its encryption randomness from a cryptographic generator (lol-apps SymmSHE.hs:138-146 under
// CryptoRand).  Here every output word is a pure function of (key, nonce, block counter): the samples do not depend
// on launch shape, stream or how a batch is split.  Stream layout (include/lolhip.h states it for callers):
//   batch item b of a call with stream offset ctr: nonce = (domain, lo32(ctr + b), hi32(ctr + b)), block counter
//   from 0 for each (domain, item); domains CHACHA_DOM_* below.
//   Gaussian coefficient j: pair i = j >> 1 from block i >> 2, words 4(i&3) .. 4(i&3)+3 (Box-Muller, below).
//   Uniform residue r = j*T + t: block r >> 2, words 4(r&3) .. 4(r&3)+3, as one 128-bit integer reduced mod q_t.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LH_RNG_HD __host__ __device__ __forceinline__
#else
#define LH_RNG_HD inline
#endif

namespace lolhip {

// 3 / 4: the Gaussians and c1 of key-switch hint rows (kshint.hip; item = LWE sample ctr + b L + j)
// 5 / 6 / 7: the uniform a, the Gaussians and the uniform secret of RLWE / RLWR instances (rlwe.hip; item = ctr + b)
enum { CHACHA_DOM_ENC_GAUSS = 0, CHACHA_DOM_UNIFORM = 1, CHACHA_DOM_ERR_ROUNDED = 2, CHACHA_DOM_HINT_GAUSS = 3,
       CHACHA_DOM_HINT_UNIFORM = 4, CHACHA_DOM_RLWE_UNIFORM = 5, CHACHA_DOM_RLWE_GAUSS = 6, CHACHA_DOM_RLWE_SECRET = 7 };

// the 256-bit key as eight little-endian words (passed to kernels by value)
struct ChaChaKey { uint32_t k[8]; };

LH_RNG_HD uint32_t chacha_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define LH_CHACHA_QR(a, b, c, d)                  \
  a += b; d ^= a; d = chacha_rotl(d, 16);        \
  c += d; b ^= c; b = chacha_rotl(b, 12);        \
  a += b; d ^= a; d = chacha_rotl(d, 8);         \
  c += d; b ^= c; b = chacha_rotl(b, 7);

// RFC 8439 §2.3: state = constants, key, counter, nonce; 20 rounds (10 column + diagonal double rounds); the input
// state added back in.  out[i] is word i of the serialized block (little-endian bytes 4i .. 4i+3).
LH_RNG_HD void chacha20_block(const ChaChaKey& key, uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2,
                              uint32_t out[16]) {
  uint32_t x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                    key.k[0], key.k[1], key.k[2], key.k[3], key.k[4], key.k[5], key.k[6], key.k[7],
                    counter, n0, n1, n2};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    LH_CHACHA_QR(x[0], x[4], x[8], x[12]) LH_CHACHA_QR(x[1], x[5], x[9], x[13])
    LH_CHACHA_QR(x[2], x[6], x[10], x[14]) LH_CHACHA_QR(x[3], x[7], x[11], x[15])
    LH_CHACHA_QR(x[0], x[5], x[10], x[15]) LH_CHACHA_QR(x[1], x[6], x[11], x[12])
    LH_CHACHA_QR(x[2], x[7], x[8], x[13]) LH_CHACHA_QR(x[3], x[4], x[9], x[14])
  }
  out[0] = x[0] + 0x61707865u; out[1] = x[1] + 0x3320646eu; out[2] = x[2] + 0x79622d32u; out[3] = x[3] + 0x6b206574u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) out[4 + i] = x[4 + i] + key.k[i];
  out[12] = x[12] + counter; out[13] = x[13] + n0; out[14] = x[14] + n1; out[15] = x[15] + n2;
}
#undef LH_CHACHA_QR

}  // namespace lolhip
