// lol_amd/csrc/hostmath.h — host-side number theory for plan construction.
//
// Product code (linked into liblolhip.so).  Mirrors what Lol's Haskell side
// computes before it calls into C:
//   goodQs / principalRootUnity / mhatInv   lol/Crypto/Lol/Types/Unsafe/ZqBasic.hs:71-73,144-171
//   ppsFact / totientFact / valueHat         lol/Crypto/Lol/FactoredDefs.hs:360-361,428-445
//   ru / ruInv                               lol-cpp/Crypto/Lol/Cyclotomic/Tensor/CPP.hs:422-442
//   gCRTK / gInvCRTK                         lol/Crypto/Lol/Cyclotomic/Tensor.hs:290-337
//   index tables for twace/embed             lol/Crypto/Lol/Cyclotomic/Tensor.hs:390-509
//   powBasisPow                              lol-cpp/Crypto/Lol/Cyclotomic/Tensor/CPP/Extension.hs:131-141
// (crtSetDec / crtSet: crtset.h)
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "lolhip.h"

namespace lolhip {

typedef uint64_t u64;
typedef int64_t i64;
typedef unsigned __int128 u128;

struct PP { int p; int e; };

// a prime-power list as every entry point takes it: ascending primes, exponents >= 1 and, for max_m != 0, the index
// prod p^e at most max_m
bool valid_pps(const std::vector<PP>& pps, u64 max_m = 0);
// the list behind a C array (not validated); false for a negative count or a null array with a positive one
bool to_pps(const lolhip_pp* pps, int npps, std::vector<PP>& out);
// the same prime powers in the same order
inline bool same_pps(const std::vector<PP>& a, const std::vector<PP>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (a[i].p != b[i].p || a[i].e != b[i].e) return false;
  return true;
}

inline u64 mulmod(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
u64 powmod(u64 b, u64 e, u64 q);
// b^-1 mod q, 0 when gcd(b,q) != 1
u64 invmod(u64 b, u64 q);
bool is_prime(u64 n);
// sorted distinct prime factors
std::vector<u64> prime_factors(u64 n);
std::vector<PP> factor_pps(u64 m);

i64 ipow(i64 b, int e);
i64 value_pps(const std::vector<PP>& pps);
i64 totient_pp(int p, int e);           // totient_pp(p,0) == 1
i64 totient_pps(const std::vector<PP>& pps);
i64 value_hat(i64 m);                   // m/2 if even else m
u64 odd_rad(const std::vector<PP>& pps);
i64 digit_rev(int p, int e, i64 j);

// first prime > lower congruent to 1 mod m (head of goodQs m lower)
u64 first_good_q(u64 m, u64 lower);
// smallest generator of Z_q^* for prime q
u64 smallest_generator(u64 q);
// omega_m = g0^((q-1)/m); returns 0 when q is not prime or m does not divide q-1
u64 principal_root(u64 m, u64 q);

// g vectors in the CRT basis, one modulus, length totient(m)
// omega_p[k] = primitive p_k-th root of unity to use (p_k = pps[k].p)
std::vector<u64> g_crt(const std::vector<PP>& pps, const std::vector<u64>& omega_p, u64 q, bool inverse);

// C_m = max_k sum_{i,j} |(b_i b_j)_k| over the powerful basis b of index m: a product of two ring elements whose
// powerful-basis coefficients are bounded by A and B has coefficients bounded by C_m A B.  Saturates at 2^62.
u64 growth(const std::vector<PP>& pps);

// ---- ring-extension index tables (m | m') --------------------------------
struct MergedPP { int p, e, e2; };
// false if pps does not divide pps2
bool merge_pps(const std::vector<PP>& pps, const std::vector<PP>& pps2, std::vector<MergedPP>& out);
std::pair<i64, i64> to_index_pair(const std::vector<std::pair<i64, i64>>& tots, i64 i2);
i64 from_index_pair(const std::vector<std::pair<i64, i64>>& tots, i64 i1, i64 i0);

struct ExtTables {
  i64 phi = 0, phi2 = 0;
  std::vector<int32_t> twace_powdec;   // [phi]   extIndicesPowDec: out[i] = in[idx[i]]
  std::vector<int32_t> ext_crt;        // [phi2]  extIndicesCRT
  std::vector<int32_t> embed_pow;      // [phi2]  source index in O_m or -1 (zero)
  std::vector<int32_t> embed_dec;      // [phi2]  source index, -1 zero; bit 30 set => negate
  std::vector<int32_t> embed_crt;      // [phi2]  baseIndicesCRT
  std::vector<int32_t> coeffs;         // [phi2/phi][phi] extIndicesCoeffs: out[i1][i0] = in[idx[i1*phi + i0]]
};
static const int32_t EMBED_NEG_FLAG = 1 << 30;
bool build_ext_tables(const std::vector<PP>& pps, const std::vector<PP>& pps2, ExtTables& out);
// powBasisPow (CPP/Extension.hs:131-141): the n'/n powerful-basis indices of the relative powerful basis
std::vector<int32_t> pow_basis_pow(const ExtTables& X);

}  // namespace lolhip
