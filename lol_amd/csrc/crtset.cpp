// lol_amd/csrc/crtset.cpp — see crtset.h for the reference map and include/lolhip.h for the definitions.
#include "crtset.h"

#include <algorithm>
#include <map>
#include <numeric>

namespace lolhip {

namespace {

const i64 kInvalid = -1, kModulus = -2;

const u64 kMaxIndex = ((u64)1 << 31) - 1;   // every index here is below 2^31

// indexToPow (Tensor.hs:359-362)
i64 index_to_pow(int p, int e, i64 j) { return ipow(p, e - 1) * (j % (p - 1)) + digit_rev(p, e - 1, j / (p - 1)); }

// ---- GF(p^d) = F_p[x]/(f), p < 2^31: elements are d coefficients, constant first -------------------------------------
typedef std::vector<u64> Poly;

struct Field {
  u64 p = 2;
  int d = 1;
  Poly f;   // the d low coefficients of the monic modulus

  Poly one() const { Poly r((size_t)d, 0); r[0] = 1 % p; return r; }
  Poly x() const {
    Poly r((size_t)d, 0);
    if (d == 1) r[0] = (p - f[0]) % p; else r[1] = 1;
    return r;
  }
  Poly mul(const Poly& a, const Poly& b) const {
    Poly t((size_t)(2 * d - 1), 0);
    for (int i = 0; i < d; ++i) {
      if (!a[(size_t)i]) continue;
      for (int j = 0; j < d; ++j) t[(size_t)(i + j)] = (t[(size_t)(i + j)] + a[(size_t)i] * b[(size_t)j]) % p;
    }
    for (int k = 2 * d - 2; k >= d; --k) {
      const u64 c = t[(size_t)k];
      if (!c) continue;
      for (int i = 0; i < d; ++i) t[(size_t)(k - d + i)] = (t[(size_t)(k - d + i)] + (p - f[(size_t)i]) % p * c) % p;
    }
    t.resize((size_t)d);
    return t;
  }
  Poly pow(Poly a, u64 e) const {
    Poly r = one();
    while (e) {
      if (e & 1) r = mul(r, a);
      a = mul(a, a);
      e >>= 1;
    }
    return r;
  }
  bool is_one(const Poly& a) const {
    if (a[0] != 1 % p) return false;
    for (int i = 1; i < d; ++i) if (a[(size_t)i]) return false;
    return true;
  }
};

void trim(Poly& a) { while (!a.empty() && a.back() == 0) a.pop_back(); }

// gcd over F_p of two polynomials (any lengths, constant first); the result's degree is all the caller needs
int gcd_degree(Poly a, Poly b, u64 p) {
  trim(a); trim(b);
  while (!b.empty()) {
    // a <- a mod b
    const u64 inv = invmod(b.back(), p);
    while (a.size() >= b.size()) {
      const u64 c = a.back() * inv % p;
      const size_t off = a.size() - b.size();
      if (c) for (size_t i = 0; i < b.size(); ++i) a[off + i] = (a[off + i] + (p - b[i]) * c) % p;
      a.pop_back();
      trim(a);
    }
    std::swap(a, b);
  }
  return (int)a.size() - 1;
}

// Rabin's test of the monic polynomial x^d + F.f
bool irreducible(const Field& F) {
  const int d = F.d;
  std::vector<Poly> frob((size_t)(d + 1));            // frob[t] = x^(p^t) mod f
  frob[0] = F.x();
  for (int t = 1; t <= d; ++t) frob[(size_t)t] = F.pow(frob[(size_t)(t - 1)], F.p);
  if (frob[(size_t)d] != frob[0]) return false;
  Poly full(F.f);
  full.push_back(1);
  for (u64 r : prime_factors((u64)d)) {
    Poly h = frob[(size_t)(d / (int)r)];
    for (int i = 0; i < d; ++i) h[(size_t)i] = (h[(size_t)i] + F.p - frob[0][(size_t)i]) % F.p;
    if (gcd_degree(full, h, F.p) != 0) return false;
  }
  return true;
}

// the field of include/lolhip.h's rule and its generator; false when p^d is not below 2^62
bool make_field(u64 p, int d, Field& F, Poly& gen) {
  const u64 size = pow_below62(p, d);
  if (!size) return false;
  F.p = p;
  F.d = d;
  for (u64 c = 0;; ++c) {
    F.f.assign((size_t)d, 0);
    u64 v = c;
    for (int i = 0; i < d; ++i) { F.f[(size_t)i] = v % p; v /= p; }
    if (irreducible(F)) break;
  }
  const u64 N = size - 1;
  std::vector<u64> exps;
  if (N > 1) for (u64 r : prime_factors(N)) exps.push_back(N / r);
  for (u64 c = 1;; ++c) {
    gen.assign((size_t)d, 0);
    u64 v = c;
    for (int i = 0; i < d; ++i) { gen[(size_t)i] = v % p; v /= p; }
    bool ok = true;
    for (u64 e : exps) if (F.is_one(F.pow(gen, e))) { ok = false; break; }
    if (ok) return true;
  }
}

// the powerful basis of one index as exponents of zeta_m, and the schoolbook product mod `mod` in it
struct PowRing {
  std::vector<PP> pps;
  i64 n = 1, m = 1;
  std::vector<i64> expo;       // [n]  basis element j = zeta_m^expo[j]
  std::vector<i64> tuple_of;   // [m]  exponent a -> mixed-radix index of (a_k mod pp_k), first prime power fastest
  std::vector<i64> basis_at;   // [n]  the mixed-radix index of basis element j
  mutable std::vector<u64> F, G;   // [m] each: the scratch of mul, allocated once

  explicit PowRing(const std::vector<PP>& pps_) : pps(pps_) {
    n = totient_pps(pps);
    m = value_pps(pps);
    const size_t K = pps.size();
    std::vector<i64> pp(K), phi(K), co(K), coinv(K), stride(K);
    i64 st = 1;
    for (size_t k = 0; k < K; ++k) {
      pp[k] = ipow(pps[k].p, pps[k].e);
      phi[k] = totient_pp(pps[k].p, pps[k].e);
      co[k] = m / pp[k];
      coinv[k] = (i64)invmod((u64)(co[k] % pp[k]), (u64)pp[k]);
      stride[k] = st;
      st *= pp[k];
    }
    expo.assign((size_t)n, 0);
    basis_at.assign((size_t)n, 0);
    for (i64 j = 0; j < n; ++j) {
      i64 jj = j, a = 0, lin = 0;
      for (size_t k = 0; k < K; ++k) {
        const i64 t = index_to_pow(pps[k].p, pps[k].e, jj % phi[k]);
        jj /= phi[k];
        a = (a + t * co[k]) % m;
        lin += t * stride[k];
      }
      expo[(size_t)j] = a;
      basis_at[(size_t)j] = lin;
    }
    tuple_of.assign((size_t)m, 0);
    for (i64 a = 0; a < m; ++a) {
      i64 lin = 0;
      for (size_t k = 0; k < K; ++k) lin += ((a % pp[k]) * coinv[k] % pp[k]) * stride[k];
      tuple_of[(size_t)a] = lin;
    }
  }

  // c = a b, all [n] residues in [0, mod); c may alias a or b
  void mul(const i64* a, const i64* b, i64* c, u64 mod) const {
    F.assign((size_t)m, 0);
    G.assign((size_t)m, 0);
    for (i64 i = 0; i < n; ++i) {
      if (!a[i]) continue;
      for (i64 j = 0; j < n; ++j) {
        if (!b[j]) continue;
        u64& dst = F[(size_t)((expo[(size_t)i] + expo[(size_t)j]) % m)];
        dst = (dst + mulmod((u64)a[i], (u64)b[j], mod)) % mod;
      }
    }
    for (i64 x = 0; x < m; ++x) G[(size_t)tuple_of[(size_t)x]] = F[(size_t)x];
    // z^(phi + r) = -sum_{l < p - 1} z^(l p^(e-1) + r), one prime power after the other
    i64 stride = 1;
    for (const PP& pe : pps) {
      const i64 pk = ipow(pe.p, pe.e), pk1 = pk / pe.p, phi = pk - pk1;
      for (i64 idx = 0; idx < m; ++idx) {
        const i64 t = (idx / stride) % pk;
        const u64 v = G[(size_t)idx];
        if (t < phi || !v) continue;
        G[(size_t)idx] = 0;
        for (i64 l = 0; l + 1 < pe.p; ++l) {
          u64& dst = G[(size_t)(idx + (l * pk1 + (t - phi) - t) * stride)];
          dst = (dst + mod - v) % mod;
        }
      }
      stride *= pk;
    }
    for (i64 j = 0; j < n; ++j) c[j] = (i64)G[(size_t)basis_at[(size_t)j]];
  }
};

}  // namespace

i64 mult_order(u64 p, u64 m) {
  if (m == 1) return 1;
  const u64 pm = p % m;
  if (std::gcd(pm, m) != 1) return 0;
  i64 d = 1;
  for (u64 x = pm; x != 1; x = mulmod(x, pm, m)) ++d;
  return d;
}

std::vector<PP> strip_prime(const std::vector<PP>& pps, i64 p) {
  std::vector<PP> out;
  for (const PP& pe : pps) if (pe.p != p) out.push_back(pe);
  return out;
}

u64 pow_below62(u64 b, int e) {
  unsigned __int128 r = 1;
  for (int i = 0; i < e; ++i) { r *= b; if (r >> 62) return 0; }
  return (u64)r;
}

i64 crtset_count(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p) {
  std::vector<MergedPP> mp;
  if (!valid_pps(pps, kMaxIndex) || !valid_pps(pps2, kMaxIndex) || !merge_pps(pps, pps2, mp)) return kInvalid;
  if (p < 2 || p >= ((i64)1 << 31) || !is_prime((u64)p)) return kInvalid;
  const u64 m = (u64)value_pps(pps), m2 = (u64)value_pps(pps2);
  if (m2 % (u64)p == 0) return kInvalid;
  const i64 d = mult_order((u64)p, m), d2 = mult_order((u64)p, m2);
  return (totient_pps(pps2) / d2) / (totient_pps(pps) / d);
}

i64 partition_cosets(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p, std::vector<std::vector<i64>>& reps) {
  const i64 K = crtset_count(pps, pps2, p);
  if (K < 0) return K;
  const i64 m = value_pps(pps), m2 = value_pps(pps2);
  // the cosets of <p> in Z_m'^* by ascending smallest element, grouped by the smallest residue mod m they reduce to
  std::vector<char> seen((size_t)m2 + 1, 0);
  std::map<i64, std::vector<i64>> groups;
  for (i64 x = 1; x <= m2; ++x) {
    if (seen[(size_t)(x % m2)] || std::gcd(x, m2) != 1) continue;
    i64 key = x % m;
    for (i64 y = x % m2;;) {
      seen[(size_t)y] = 1;
      key = std::min(key, y % m);
      y = (i64)mulmod((u64)y, (u64)(p % m2), (u64)m2);
      if (y == x % m2) break;
    }
    groups[key].push_back(x % m2);
  }
  reps.assign((size_t)K, std::vector<i64>());
  for (auto& g : groups) {
    if ((i64)g.second.size() != K) return kInvalid;
    // insertWith' (++) prepends: each group lists its cosets by descending smallest element
    for (i64 c = 0; c < K; ++c) reps[(size_t)c].push_back(g.second[(size_t)(K - 1 - c)]);
  }
  return K;
}

i64 crtset_dec(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p, std::vector<i64>& out) {
  std::vector<std::vector<i64>> reps;
  const i64 K = partition_cosets(pps, pps2, p, reps);
  if (K < 0) return K;
  const i64 m2 = value_pps(pps2), n2 = totient_pps(pps2);
  const int d = (int)mult_order((u64)p, (u64)m2);
  Field F;
  Poly gen;
  if (!make_field((u64)p, d, F, gen)) return kModulus;
  const u64 up = (u64)p;
  // T[i] = Tr(x^i): the trace is F_p-linear, so Tr[k] = <coefficients of w^k, T>
  std::vector<u64> T((size_t)d, 0);
  {
    Poly xi = F.one();
    const Poly x = F.x();
    for (int i = 0; i < d; ++i) {
      // the sum of the d conjugates, added as whole elements: it lies in F_p
      Poly acc((size_t)d, 0), z = xi;
      for (int t = 0; t < d; ++t) {
        for (int c = 0; c < d; ++c) acc[(size_t)c] = (acc[(size_t)c] + z[(size_t)c]) % up;
        z = F.pow(z, up);
      }
      T[(size_t)i] = acc[0];
      xi = F.mul(xi, x);
    }
  }
  const u64 size = pow_below62(up, d);
  const Poly w = F.pow(gen, (size - 1) / (u64)m2);
  std::vector<i64> tr((size_t)m2, 0);
  {
    Poly wk = F.one();
    for (i64 k = 0; k < m2; ++k) {
      u64 s = 0;
      for (int c = 0; c < d; ++c) s = (s + wk[(size_t)c] * T[(size_t)c]) % up;
      tr[(size_t)k] = (i64)s;
      wk = F.mul(wk, w);
    }
  }
  // A_j = sum_k (m'/pp_k) pow_k(j_k);  the signed exponents B_S = sum_{k in S} m'/p_k over the odd primes
  const size_t NP = pps2.size();
  std::vector<i64> Aj((size_t)n2, 0);
  for (i64 j = 0; j < n2; ++j) {
    i64 jj = j, a = 0;
    for (size_t k = 0; k < NP; ++k) {
      const i64 phi = totient_pp(pps2[k].p, pps2[k].e);
      a = (a + (m2 / ipow(pps2[k].p, pps2[k].e)) * index_to_pow(pps2[k].p, pps2[k].e, jj % phi)) % m2;
      jj /= phi;
    }
    Aj[(size_t)j] = a;
  }
  std::vector<std::pair<i64, int>> BS(1, {0, 1});
  for (size_t k = 0; k < NP; ++k) {
    if (pps2[k].p == 2) continue;
    const size_t cnt = BS.size();
    for (size_t s = 0; s < cnt; ++s) BS.push_back({(BS[s].first + m2 / pps2[k].p) % m2, -BS[s].second});
  }
  const u64 hinv = invmod((u64)value_hat(m2) % up, up);
  out.assign((size_t)(K * n2), 0);
  for (i64 c = 0; c < K; ++c)
    for (i64 j = 0; j < n2; ++j) {
      i64 acc = 0;
      for (const auto& bs : BS) {
        const i64 ex = (bs.first - Aj[(size_t)j] + m2) % m2;
        for (i64 i : reps[(size_t)c]) acc += bs.second * tr[(size_t)(i * ex % m2)];
      }
      const u64 r = (u64)(((acc % p) + p) % p);
      out[(size_t)(c * n2 + j)] = (i64)(r * hinv % up);
    }
  return K;
}

bool crtset_bound_ok(const std::vector<PP>& pps2bar, u64 p, u64 pe, u64 Q) {
  const unsigned __int128 C = growth(pps2bar), h = pe / 2, cap = (unsigned __int128)1 << 61;
  const unsigned __int128 ch = C * h;                                // C <= 2^62, h < 2^61
  if (ch >= cap) return false;
  return 2 * ch * h < Q && (unsigned __int128)2 * (p - 1) * (u64)totient_pps(pps2bar) < Q;
}

i64 crtset_modulus(const std::vector<PP>& pps2, i64 p, int e) {
  if (!valid_pps(pps2, kMaxIndex) || e < 1 || p < 2 || p >= ((i64)1 << 31) || !is_prime((u64)p)) return kInvalid;
  const u64 pe = pow_below62((u64)p, e);
  if (!pe) return kModulus;
  const std::vector<PP> bar = strip_prime(pps2, p);
  const unsigned __int128 C = growth(bar), h = pe / 2, cap = (unsigned __int128)1 << 61;
  const unsigned __int128 ch = C * h;
  if (ch >= cap) return kModulus;
  unsigned __int128 lower = 2 * ch * h;
  // l on the lifted residues: prefix sums below (p - 1) phi, kept below Q/2 as well
  lower = std::max(lower, (unsigned __int128)2 * (u64)(p - 1) * (u64)totient_pps(bar));
  if (lower >= cap) return kModulus;
  const u64 Q = first_good_q((u64)value_pps(bar), (u64)lower);
  return Q < ((u64)1 << 61) ? (i64)Q : kModulus;
}

void host_l(const std::vector<PP>& pps, u64 mod, i64* y, i64 rows) {
  const i64 n = totient_pps(pps);
  i64 rts = 1;
  for (const PP& pe : pps) {
    const i64 d = pe.p - 1;
    if (pe.p != 2)
      for (i64 r = 0; r < rows; ++r)
        for (i64 v = 0; v < n / d; ++v) {
          i64* base = y + r * n + (v / rts) * d * rts + v % rts;
          for (i64 i = 1; i < d; ++i) base[i * rts] = (i64)(((u64)base[i * rts] + (u64)base[(i - 1) * rts]) % mod);
        }
    rts *= totient_pp(pe.p, pe.e);
  }
}

i64 crtset_host(const std::vector<PP>& pps, const std::vector<PP>& pps2, i64 p, int e, std::vector<i64>& out) {
  std::vector<MergedPP> mp;
  if (e < 1 || !valid_pps(pps, kMaxIndex) || !valid_pps(pps2, kMaxIndex) || !merge_pps(pps, pps2, mp)) return kInvalid;
  const std::vector<PP> bar = strip_prime(pps, p), bar2 = strip_prime(pps2, p);
  std::vector<i64> x;
  const i64 K = crtset_dec(bar, bar2, p, x);
  if (K < 0) return K;
  const i64 Q = crtset_modulus(pps2, p, e);                          // the host path reports the device path's statuses
  if (Q < 0) return Q;
  const u64 pe = pow_below62((u64)p, e);
  const i64 nb = totient_pps(bar2), n2 = totient_pps(pps2);
  host_l(bar2, pe, x.data(), K);
  if (e > 1) {
    const PowRing R(bar2);
    std::vector<i64> y((size_t)nb);
    for (i64 c = 0; c < K; ++c) {
      i64* xc = x.data() + c * nb;
      for (int step = 1; step < e; ++step) {
        std::copy(xc, xc + nb, y.begin());
        for (i64 t = 1; t < p; ++t) R.mul(y.data(), xc, y.data(), pe);
        std::copy(y.begin(), y.end(), xc);
      }
    }
  }
  ExtTables X;
  if (!build_ext_tables(bar2, pps2, X)) return kInvalid;
  out.assign((size_t)(K * n2), 0);
  for (i64 c = 0; c < K; ++c)
    for (i64 i2 = 0; i2 < n2; ++i2) {
      const int32_t src = X.embed_pow[(size_t)i2];
      out[(size_t)(c * n2 + i2)] = src < 0 ? 0 : x[(size_t)(c * nb + src)];
    }
  return K;
}

}  // namespace lolhip
