// lol_amd/csrc/pipeline.h — launcher interface of pipeline.hip (SURVEY.md §8f N1 kernels).
#pragma once
#include <hip/hip_runtime_api.h>

#include "zq_dev.h"

namespace lolhip {

constexpr int PIPE_MAX_T = 16;   // RNS components a pipeline call accepts (parameter structs travel by value)

struct DecompParams {
  int T;                 // components
  int L;                 // total digits = sum k[t]
  i64 base;              // 0: TrivGad (ZqBasic.hs:227-232); >= 2: BaseBGad b (ZqBasic.hs:258-264)
  u64 magic;             // floor(2^64 (2^l - base) / base) + 1,  l = ceil(log2 base)
  int sh1, sh2;          // min(l,1), max(l-1,0)
  int k[PIPE_MAX_T];     // digits of component t: gadlen(base, q_t) (1 for TrivGad)
};

struct RescaleParams {
  int T;                       // components of the input; component 0 is dropped
  u64 qa_inv[PIPE_MAX_T];      // q_0^-1 mod q_s, s >= 1
};

// p-dependent constants of decrypt.hip k_lift (the p-independent ones are the plan's lift_consts)
struct LiftParams {
  int T;                       // components
  int msd;                     // 1: scale every residue by scale[t] first (toLSD of an MSD ciphertext)
  u64 scale[PIPE_MAX_T];       // p mod q_t
  ModCtx mp;                   // p mode: the plaintext modulus (any p >= 2: generic division, no Montgomery form)
  u64 pw[PIPE_MAX_T];          // (q_0 ... q_(i-1)) mod p
  u64 qp;                      // Q mod p
  u64 lp;                      // l' mod p
};

hipError_t launch_ctmul(hipStream_t s, const i64* c0, const i64* c1, const i64* d0, const i64* d1, i64* e0, i64* e1,
                        i64* e2, const i64* gcrt, i64 B, i64 n, int T, const ModCtx* mod);
hipError_t launch_decompose(hipStream_t s, const i64* c, i64* digits, i64 B, i64 n, const DecompParams& p,
                            const ModCtx* mod, bool q32 = false);   // q32: every modulus below 2^31
hipError_t launch_knapsack(hipStream_t s, const i64* xs, int L, const i64* hint, int K, const i64* addend, i64* out,
                           i64 B, i64 n, int T, const ModCtx* mod, bool q32 = false);   // q32: every modulus below 2^29 (64-bit accumulators)
hipError_t launch_rescale(hipStream_t s, const i64* c, i64* out, i64 B, i64 n, const RescaleParams& p,
                          const ModCtx* mod);

// coeffs (Extension.hs:90-93): out[i1][b][i0][t] = in[b][idx[i1*n_lo + i0]][t]
hipError_t launch_coeffs(hipStream_t s, i64* out, const i64* in, const int32_t* idx, i64 B, i64 n_lo, i64 n_hi, int T,
                         const ModCtx* mod);

// decrypt.hip: errorTerm / decrypt (lol-apps SymmSHE.hs:153-178)
// out = (sum_k comps_k s^k) (* s when times_s), CRT basis; comps_k = comps + k * B*n*T; out may alias comps
hipError_t launch_sk_eval(hipStream_t s, const i64* comps, int ncomp, bool times_s, const i64* s_crt, i64* out, i64 B,
                          i64 n, int T, const ModCtx* mod);
hipError_t launch_addmod(hipStream_t s, i64* y, const i64* a, i64 B, i64 n, int T, const ModCtx* mod);
// rows = B * n coefficients [rows][T] (+ add, may be null) -> [rows] int64: p mode (pmode) or the centred lift
hipError_t launch_lift(hipStream_t s, const i64* in, const i64* add, i64* out, i64 rows, const LiftParams& p, bool pmode,
                       const u64* lift_consts, const ModCtx* mod);

// encrypt.hip: SymmSHE encrypt / errorRounded samplers over the ChaCha20 stream (rng_dev.h)
struct ChaChaKey;
enum { ENC_WRITE = 0, ENC_ADD = 1, ENC_INT = 2 };
// Gaussians of deviation sigma, [B][n] doubles
hipError_t launch_enc_gauss(hipStream_t s, double* d, i64 B, i64 n, const ChaChaKey& key, u64 ctr, int domain,
                            double sigma);
// e = rep + p round((g - rep) / p) per coefficient, g from d (when given) or the stream; rep [B][n] in (-p, p) or null;
// mode ENC_WRITE / ENC_ADD: residues [B][n][T] (mod), ENC_INT: int64 [B][n] (out may alias d)
hipError_t launch_enc_error(hipStream_t s, const double* d, const i64* rep, i64 p, i64* out, i64 B, i64 n, int T,
                            const ModCtx* mod, int mode, const ChaChaKey& key, u64 ctr, int domain, double sigma);
// c1 = uniform c^1 (CRT basis); c0 = c0 - c^1 s^ (combine) or -c^1 s^
hipError_t launch_enc_c1(hipStream_t s, bool combine, i64* c0, i64* c1, const i64* s_crt, i64 B, i64 n, int T,
                         const ModCtx* mod, const ChaChaKey& key, u64 ctr);

// kshint.hip: key-switch hint rows (lol-apps SymmSHE.hs:262-296).  e_crt [B][L][n][T] (the crt'd rounded Gaussians),
// vals [B][n][T], s_crt [n][T] -> hints [B][L][2][n][T]: h1 = c^1 (domain 4, item ctr + b L + j), h0 = g_j val + e - c^1 s
hipError_t launch_kshint_combine(hipStream_t s, const i64* e_crt, const i64* vals, const i64* s_crt, i64* hints, i64 B,
                                 i64 n, const DecompParams& dp, const ModCtx* mod, const ChaChaKey& key, u64 ctr);
// out [rel][n][T]: the powerful-basis unit vector at coeffs[i * n_lo] for row i (0 / 1 residues)
hipError_t launch_unit_rows(hipStream_t s, i64* out, const int32_t* coeffs, i64 rel, i64 n, int T, i64 n_lo);

// khprf.hip: the key-homomorphic ring PRF (lol-apps KeyHomomorphicPRF.hs), one modulus.  A child of node v as the node
// kernel sees it: its prefix is w_v >> shift, its slot w & mask when full, else w - lo (a leaf: full, mask 1)
struct KhprfChild {
  i64 lo;                      // x0 >> s_child
  i64 mask;                    // 2^c_child - 1
  int full;                    // the child's slots are its sub-inputs
  int shift;                   // s_child - s_v
};
struct KhprfNode {
  i64 U;                       // slots of v
  i64 lo;                      // x0 >> s_v
  int full;                    // U = 2^c_v: slot k stands for w_v = k, else for lo + k
  int ell;                     // gadget length
  i64 n;                       // coefficients per polynomial
  i64 R;                       // slots k, k + R, ... share one right slot (2^c_r for a full right child, else U)
  i64 d_digit;                 // stride of digit i in D = [ell][U_r][ell][n]: U_r * ell * n
  KhprfChild l, r;
};
// out [U][ell][n] = L [U_l][ell][n] x D [ell][U_r][ell][n] per slot, CRT basis; fold: Q32 digits per 64-bit sum
hipError_t launch_khprf_node(hipStream_t s, const i64* L, const i64* D, i64* out, const KhprfNode& nd, const ModCtx& mc,
                             int fold);
// out [nkeys][rows][n] = s_crt [key][n] * A [rows][n], CRT basis
hipError_t launch_khprf_keymul(hipStream_t s, const i64* A, const i64* s_crt, i64* out, i64 nkeys, i64 rows, i64 n,
                               const ModCtx& mc);
// y = fst (divModCent (p lift y) q) mod p in place (rescaleMod, q odd, p q < 2^63)
hipError_t launch_khprf_round(hipStream_t s, i64* y, i64 total, i64 p, const ModCtx& mc);
// the lifted family (q = 2^qbits, node products exact mod the NTT prime Q): dst = the pass `mode` of src, words in
// [0, Q) / [0, q); src == dst allowed; 16-byte accesses when both are 16-byte aligned, 8-byte ones otherwise.
// LIFT_FROM_Q: reduce lift_Q x mod q; LIFT_TO_Q: lift_q into [0, Q); LIFT_ROUND: fst (divModCent (p lift_q r) q) mod p
// (needs p q < 2^63; not with LIFT_TO_Q)
enum { LIFT_FROM_Q = 1, LIFT_TO_Q = 2, LIFT_ROUND = 4 };
struct KhprfLift {
  u64 Q;                       // the NTT prime
  u64 p;                       // LIFT_ROUND: the target modulus
  int qbits;                   // q = 2^qbits, 1 <= qbits <= 62
};
hipError_t launch_khprf_lift(hipStream_t s, const i64* src, i64* dst, i64 total, int mode, const KhprfLift& c);

}  // namespace lolhip
