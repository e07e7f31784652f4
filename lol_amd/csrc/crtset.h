// lol_amd/csrc/crtset.h — host number theory of the CRT sets (include/lolhip.h has the definitions and the rule for the
// root of unity).  Product code (linked into liblolhip.so).  Mirrors
//   powBasisPow / crtSetDec       lol-cpp/Crypto/Lol/Cyclotomic/Tensor/CPP/Extension.hs:131-164
//   partitionCosets / order       lol/Crypto/Lol/Types/ZmStar.hs:43-88
//   twCRTs                        lol/Crypto/Lol/Cyclotomic/Tensor.hs:300-313
//   crtSet                        lol/Crypto/Lol/Cyclotomic/UCyc.hs:540-565
// Everything here returns a count, or -1 (invalid arguments) / -2 (a modulus out of range): the values of
// LOLHIP_ERR_INVALID / LOLHIP_ERR_MODULUS.
#pragma once
#include <cstdint>
#include <vector>

#include "hostmath.h"

namespace lolhip {

// ord_m(p) for m >= 1 (1 for m = 1); 0 when gcd(p, m) != 1
i64 mult_order(u64 p, u64 m);
// the prime powers without the prime p
std::vector<PP> strip_prime(const std::vector<PP>& pps, i64 p);
// b^e, or 0 when it is not below 2^62
u64 pow_below62(u64 b, int e);

// K = (phi(m')/ord_m'(p)) / (phi(m)/ord_m(p)) after validation (p prime, p not dividing m', m | m'), or -1 / -2
i64 crtset_count(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p);
// partitionCosets p: K lists of representatives in Z_m'^*, in the reference's order
i64 partition_cosets(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p, std::vector<std::vector<i64>>& reps);
// crtSetDec: out [K][phi(m')] residues in [0, p), decoding basis
i64 crtset_dec(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p, std::vector<i64>& out);

// the smallest prime Q = 1 mod mbar' with C_mbar' floor(p^e/2)^2 < Q/2 and Q < 2^61 (pps2: the prime powers of m'), or -1 / -2
i64 crtset_modulus(const std::vector<PP>& pps2, i64 p, int e);
// does Q certify the products of crtSet over the index pps2bar?
bool crtset_bound_ok(const std::vector<PP>& pps2bar, u64 p, u64 pe, u64 Q);

// l (decoding -> powerful basis) over Z_mod on `rows` host polynomials of the index pps, in place; entries in [0, mod)
void host_l(const std::vector<PP>& pps, u64 mod, i64* y, i64 rows);
// crtSet by schoolbook products on the host: out [K][phi(m')] residues in [0, p^e), powerful basis
i64 crtset_host(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p, int e, std::vector<i64>& out);

}  // namespace lolhip
