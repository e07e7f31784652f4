// lol_amd/csrc/wire.cpp — reader/writer for Lol's protobuf ring-element messages (host side).
//
// Messages (lol/Lol.proto, proto2):
//   message Rq        { required uint32 m = 1; required uint64 q = 2; repeated sint64 xs = 3; }
//   message RqProduct { repeated Rq rqlist = 1; }
//   message R         { required uint32 m = 1; repeated sint64 xs = 2; }
//   message Kq / KqProduct: as Rq / RqProduct with `repeated double xs`
//   message LinearRq  { required uint32 e = 1; required uint32 r = 2; repeated RqProduct coeffs = 3; }
// and of lol-apps/SHE.proto: SecretKey, RqPolynomial, KSHint (read and write), TunnelHint.
// Conventions (lol/Crypto/Lol/Types/IZipVector.hs:127-205, Lol.proto:18-20): one Rq per
// modulus of the RNS tuple, first component first; xs are the coefficients in the DECODING
// basis, written as centred lifts in [-q/2, q/2) (toProto: `LP.lift`), read back with `reduce`.
// So ingest for the GPU path is: read -> slab [n][T] -> lolhip_l_batch -> lolhip_crt_batch.
//
// The codec is written against the protobuf wire specification (varint, zigzag, length-
// delimited sub-messages); it accepts both the unpacked encoding that proto2 `repeated sint64`
// uses by default (what hprotoc emits) and the packed one.  Unknown fields are skipped.
#include <cstdint>
#include <cstring>
#include <vector>

#include "lolhip.h"

namespace {

struct Reader {
  const uint8_t* p; const uint8_t* end; bool ok = true;
  bool varint(uint64_t& v) {
    v = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      if (p >= end) return ok = false;
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) return true;
    }
    return ok = false;
  }
  bool skip(uint32_t wt) {
    uint64_t v;
    switch (wt) {
      case 0: return varint(v);
      case 1: if (end - p < 8) return ok = false; p += 8; return true;
      case 2: if (!varint(v) || (uint64_t)(end - p) < v) return ok = false; p += v; return true;
      case 5: if (end - p < 4) return ok = false; p += 4; return true;
      default: return ok = false;
    }
  }
};

inline int64_t unzigzag(uint64_t z) { return (int64_t)(z >> 1) ^ -(int64_t)(z & 1); }
inline uint64_t zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }

inline int varint_len(uint64_t v) { int n = 1; while (v >= 0x80) { v >>= 7; ++n; } return n; }
inline void put_varint(uint8_t*& o, uint64_t v) { while (v >= 0x80) { *o++ = (uint8_t)(v | 0x80); v >>= 7; } *o++ = (uint8_t)v; }

struct RqView { uint32_t m = 0; uint64_t q = 0; bool has_m = false, has_q = false; std::vector<int64_t> xs; };

bool parse_rq(const uint8_t* b, const uint8_t* e, RqView& r) {
  Reader rd{b, e};
  while (rd.p < rd.end) {
    uint64_t key;
    if (!rd.varint(key)) return false;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    uint64_t v;
    if (field == 1 && wt == 0) { if (!rd.varint(v)) return false; r.m = (uint32_t)v; r.has_m = true; }
    else if (field == 2 && wt == 0) { if (!rd.varint(v)) return false; r.q = v; r.has_q = true; }
    else if (field == 3 && wt == 0) { if (!rd.varint(v)) return false; r.xs.push_back(unzigzag(v)); }
    else if (field == 3 && wt == 2) {                      // packed
      if (!rd.varint(v) || (uint64_t)(rd.end - rd.p) < v) return false;
      Reader in{rd.p, rd.p + v};
      while (in.p < in.end) { uint64_t z; if (!in.varint(z)) return false; r.xs.push_back(unzigzag(z)); }
      rd.p += v;
    } else if (!rd.skip(wt)) return false;
  }
  return r.has_m && r.has_q;                                // both are `required`
}

}  // namespace

extern "C" {

int64_t lolhip_rqproduct_read(const uint8_t* buf, int64_t len, uint32_t* m_out, int64_t* qs, int cap_T, int* T_out,
                              int64_t* xs, int64_t cap_xs) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  std::vector<RqView> list;
  Reader rd{buf, buf + len};
  while (rd.p < rd.end) {
    uint64_t key;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 2) {
      uint64_t l;
      if (!rd.varint(l) || (uint64_t)(rd.end - rd.p) < l) return LOLHIP_ERR_INVALID;
      list.emplace_back();
      if (!parse_rq(rd.p, rd.p + l, list.back())) return LOLHIP_ERR_INVALID;
      rd.p += l;
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  const int T = (int)list.size();
  if (T == 0) return LOLHIP_ERR_INVALID;
  const int64_t n = (int64_t)list[0].xs.size();
  for (const RqView& r : list) {
    if (r.m != list[0].m || (int64_t)r.xs.size() != n) return LOLHIP_ERR_INVALID;   // one ring, one length
    if (r.q < 2 || r.q >= ((uint64_t)1 << 62)) return LOLHIP_ERR_MODULUS;
  }
  if (m_out) *m_out = list[0].m;
  if (T_out) *T_out = T;
  if (qs) {
    if (cap_T < T) return LOLHIP_ERR_INVALID;
    for (int t = 0; t < T; ++t) qs[t] = (int64_t)list[(size_t)t].q;
  }
  if (xs) {
    if (cap_xs < n * T) return LOLHIP_ERR_INVALID;
    for (int t = 0; t < T; ++t) {
      const int64_t q = (int64_t)list[(size_t)t].q;
      for (int64_t j = 0; j < n; ++j) {                     // `reduce`: canonical residue of any integer
        int64_t r = list[(size_t)t].xs[(size_t)j] % q;
        xs[j * T + t] = r < 0 ? r + q : r;
      }
    }
  }
  return n;
}

int64_t lolhip_rqproduct_write(uint32_t m, const int64_t* qs, int T, const int64_t* xs, int64_t n, uint8_t* out,
                               int64_t cap) {
  if (!qs || T < 1 || n < 0 || (n > 0 && !xs)) return LOLHIP_ERR_INVALID;
  for (int t = 0; t < T; ++t) if (qs[t] < 2) return LOLHIP_ERR_MODULUS;
  // centred lift of component t of coefficient j (ZqBasic.hs:92-94), accepting (-q, q) inputs
  auto lifted = [&](int64_t j, int t) {
    const int64_t q = qs[t];
    int64_t x = xs[j * T + t] % q;
    if (x < 0) x += q;
    return (x < q - x) ? x : x - q;                         // 2x < q  without overflow
  };
  std::vector<int64_t> body((size_t)T);
  int64_t total = 0;
  for (int t = 0; t < T; ++t) {
    int64_t b = 1 + varint_len(m) + 1 + varint_len((uint64_t)qs[t]);
    for (int64_t j = 0; j < n; ++j) b += 1 + varint_len(zigzag(lifted(j, t)));
    body[(size_t)t] = b;
    total += 1 + varint_len((uint64_t)b) + b;
  }
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  for (int t = 0; t < T; ++t) {
    *o++ = 0x0A; put_varint(o, (uint64_t)body[(size_t)t]);  // rqlist = 1, length-delimited
    *o++ = 0x08; put_varint(o, m);                          // m = 1
    *o++ = 0x10; put_varint(o, (uint64_t)qs[t]);            // q = 2
    for (int64_t j = 0; j < n; ++j) { *o++ = 0x18; put_varint(o, zigzag(lifted(j, t))); }   // xs = 3, unpacked sint64
  }
  return (int64_t)(o - out);
}

// KSHint (lol-apps/SHE.proto): { repeated RqPolynomial hint = 1; required TypeRep gad = 2; }
// RqPolynomial: { repeated RqProduct coeffs = 1; }  constant coefficient first.
// Reads the L hint polynomials of K coefficients each into xs [L][K][n][T] (decoding basis,
// canonical residues) — after l and crt over the L*K polynomials, the slab lolhip_keyswitch_batch
// takes.  The gadget TypeRep (a GHC fingerprint, "not intended to be platform independent",
// Lol.proto) is skipped.  Returns n; pass xs = NULL to query L, K, T, m, qs.
int64_t lolhip_kshint_read(const uint8_t* buf, int64_t len, uint32_t* m_out, int64_t* qs, int cap_T, int* T_out,
                           int* L_out, int* K_out, int64_t* xs, int64_t cap_xs) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  struct Span { const uint8_t* p; int64_t n; };
  std::vector<std::vector<Span>> polys;
  Reader rd{buf, buf + len};
  while (rd.p < rd.end) {
    uint64_t key;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 2) {
      uint64_t l;
      if (!rd.varint(l) || (uint64_t)(rd.end - rd.p) < l) return LOLHIP_ERR_INVALID;
      polys.emplace_back();
      Reader in{rd.p, rd.p + l};
      while (in.p < in.end) {
        uint64_t k2;
        if (!in.varint(k2)) return LOLHIP_ERR_INVALID;
        if ((k2 >> 3) == 1 && (k2 & 7) == 2) {
          uint64_t l2;
          if (!in.varint(l2) || (uint64_t)(in.end - in.p) < l2) return LOLHIP_ERR_INVALID;
          polys.back().push_back(Span{in.p, (int64_t)l2});
          in.p += l2;
        } else if (!in.skip((uint32_t)(k2 & 7))) return LOLHIP_ERR_INVALID;
      }
      rd.p += l;
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  const int L = (int)polys.size();
  if (L == 0) return LOLHIP_ERR_INVALID;
  const int K = (int)polys[0].size();
  if (K == 0) return LOLHIP_ERR_INVALID;
  for (auto& pl : polys) if ((int)pl.size() != K) return LOLHIP_ERR_INVALID;
  uint32_t m0 = 0; int T0 = 0;
  std::vector<int64_t> q0(cap_T > 0 ? (size_t)cap_T : 16);
  const int64_t n = lolhip_rqproduct_read(polys[0][0].p, polys[0][0].n, &m0, q0.data(), (int)q0.size(), &T0, nullptr, 0);
  if (n < 0) return n;
  if (m_out) *m_out = m0;
  if (T_out) *T_out = T0;
  if (L_out) *L_out = L;
  if (K_out) *K_out = K;
  if (qs) { if (cap_T < T0) return LOLHIP_ERR_INVALID; for (int t = 0; t < T0; ++t) qs[t] = q0[(size_t)t]; }
  if (!xs) return n;
  if (cap_xs < (int64_t)L * K * n * T0) return LOLHIP_ERR_INVALID;
  std::vector<int64_t> q1(q0.size());
  for (int j = 0; j < L; ++j)
    for (int k = 0; k < K; ++k) {
      uint32_t m1 = 0; int T1 = 0;
      const int64_t n1 = lolhip_rqproduct_read(polys[(size_t)j][(size_t)k].p, polys[(size_t)j][(size_t)k].n, &m1, q1.data(),
                                               (int)q1.size(), &T1, xs + ((int64_t)j * K + k) * n * T0, n * T0);
      if (n1 < 0) return n1;
      if (n1 != n || m1 != m0 || T1 != T0) return LOLHIP_ERR_INVALID;     // every entry over the same ring and moduli
      for (int t = 0; t < T0; ++t) if (q1[(size_t)t] != q0[(size_t)t]) return LOLHIP_ERR_INVALID;
    }
  return n;
}

}  // extern "C"

// ---- the remaining messages of Lol.proto / SHE.proto ---------------------

namespace {

// one length-delimited sub-message: returns false on a malformed length
bool sub(Reader& rd, const uint8_t*& b, int64_t& l) {
  uint64_t v;
  if (!rd.varint(v) || (uint64_t)(rd.end - rd.p) < v) return false;
  b = rd.p; l = (int64_t)v; rd.p += v;
  return true;
}

// message R { required uint32 m = 1; repeated sint64 xs = 2; }
int64_t parse_r(const uint8_t* buf, int64_t len, uint32_t* m_out, int64_t* xs, int64_t cap) {
  Reader rd{buf, buf + len};
  bool has_m = false;
  int64_t n = 0;
  auto put = [&](int64_t v) { if (xs && n < cap) xs[n] = v; ++n; };
  while (rd.p < rd.end) {
    uint64_t key, v;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; if (m_out) *m_out = (uint32_t)v; has_m = true; }
    else if (field == 2 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; put(unzigzag(v)); }
    else if (field == 2 && wt == 2) {
      const uint8_t* b; int64_t l;
      if (!sub(rd, b, l)) return LOLHIP_ERR_INVALID;
      Reader in{b, b + l};
      while (in.p < in.end) { uint64_t z; if (!in.varint(z)) return LOLHIP_ERR_INVALID; put(unzigzag(z)); }
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (!has_m) return LOLHIP_ERR_INVALID;
  if (xs && n > cap) return LOLHIP_ERR_INVALID;
  return n;
}

inline double f64_at(const uint8_t* p) { double d; std::memcpy(&d, p, 8); return d; }

}  // namespace

extern "C" {

int64_t lolhip_r_read(const uint8_t* buf, int64_t len, uint32_t* m, int64_t* xs, int64_t cap_xs) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  return parse_r(buf, len, m, xs, cap_xs);
}

// message SecretKey { required R sk = 1; required double v = 2; }  (SHE.proto:9)
int64_t lolhip_secretkey_read(const uint8_t* buf, int64_t len, uint32_t* m, double* v_out, int64_t* xs, int64_t cap_xs) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  Reader rd{buf, buf + len};
  const uint8_t* rb = nullptr; int64_t rl = 0;
  bool has_v = false;
  while (rd.p < rd.end) {
    uint64_t key;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 2) { if (!sub(rd, rb, rl)) return LOLHIP_ERR_INVALID; }
    else if (field == 2 && wt == 1) { if (rd.end - rd.p < 8) return LOLHIP_ERR_INVALID; if (v_out) *v_out = f64_at(rd.p); rd.p += 8; has_v = true; }
    else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (!rb || !has_v) return LOLHIP_ERR_INVALID;
  return parse_r(rb, rl, m, xs, cap_xs);
}

// message KqProduct { repeated Kq kqlist = 1; }, Kq { m = 1; q = 2; repeated double xs = 3; }
// -> xs [n][T] doubles (decoding basis, as written), qs [T].  Returns n.
int64_t lolhip_kqproduct_read(const uint8_t* buf, int64_t len, uint32_t* m_out, int64_t* qs, int cap_T, int* T_out,
                              double* xs, int64_t cap_xs) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  struct KqView { uint32_t m = 0; uint64_t q = 0; bool hm = false, hq = false; std::vector<double> xs; };
  std::vector<KqView> list;
  Reader rd{buf, buf + len};
  while (rd.p < rd.end) {
    uint64_t key;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 2) {
      const uint8_t* b; int64_t l;
      if (!sub(rd, b, l)) return LOLHIP_ERR_INVALID;
      list.emplace_back();
      KqView& k = list.back();
      Reader in{b, b + l};
      while (in.p < in.end) {
        uint64_t k2, v;
        if (!in.varint(k2)) return LOLHIP_ERR_INVALID;
        const uint32_t f2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
        if (f2 == 1 && w2 == 0) { if (!in.varint(v)) return LOLHIP_ERR_INVALID; k.m = (uint32_t)v; k.hm = true; }
        else if (f2 == 2 && w2 == 0) { if (!in.varint(v)) return LOLHIP_ERR_INVALID; k.q = v; k.hq = true; }
        else if (f2 == 3 && w2 == 1) { if (in.end - in.p < 8) return LOLHIP_ERR_INVALID; k.xs.push_back(f64_at(in.p)); in.p += 8; }
        else if (f2 == 3 && w2 == 2) {
          const uint8_t* pb; int64_t pl;
          if (!sub(in, pb, pl) || pl % 8) return LOLHIP_ERR_INVALID;
          for (int64_t i = 0; i < pl; i += 8) k.xs.push_back(f64_at(pb + i));
        } else if (!in.skip(w2)) return LOLHIP_ERR_INVALID;
      }
      if (!k.hm || !k.hq) return LOLHIP_ERR_INVALID;
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  const int T = (int)list.size();
  if (T == 0) return LOLHIP_ERR_INVALID;
  const int64_t n = (int64_t)list[0].xs.size();
  for (const KqView& k : list) if (k.m != list[0].m || (int64_t)k.xs.size() != n) return LOLHIP_ERR_INVALID;
  if (m_out) *m_out = list[0].m;
  if (T_out) *T_out = T;
  if (qs) { if (cap_T < T) return LOLHIP_ERR_INVALID; for (int t = 0; t < T; ++t) qs[t] = (int64_t)list[(size_t)t].q; }
  if (xs) {
    if (cap_xs < n * T) return LOLHIP_ERR_INVALID;
    for (int t = 0; t < T; ++t) for (int64_t j = 0; j < n; ++j) xs[j * T + t] = list[(size_t)t].xs[(size_t)j];
  }
  return n;
}

// message LinearRq { required uint32 e = 1; required uint32 r = 2; repeated RqProduct coeffs = 3; }
// (Lol.proto:11): the values of an E-linear function on the decoding basis of R/E — after l and
// crt, the ys of lolhip_evallin_batch.  xs [C][n][T] (decoding basis, canonical residues); n, T,
// qs are those of the output ring's RqProducts.  Returns n; xs = NULL queries e, r, C, m, T, qs.
int64_t lolhip_linearrq_read(const uint8_t* buf, int64_t len, uint32_t* e_out, uint32_t* r_out, int* C_out,
                             uint32_t* m_out, int64_t* qs, int cap_T, int* T_out, int64_t* xs, int64_t cap_xs) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  struct Span { const uint8_t* p; int64_t n; };
  std::vector<Span> cs;
  bool he = false, hr = false;
  Reader rd{buf, buf + len};
  while (rd.p < rd.end) {
    uint64_t key, v;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; if (e_out) *e_out = (uint32_t)v; he = true; }
    else if (field == 2 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; if (r_out) *r_out = (uint32_t)v; hr = true; }
    else if (field == 3 && wt == 2) { const uint8_t* b; int64_t l; if (!sub(rd, b, l)) return LOLHIP_ERR_INVALID; cs.push_back(Span{b, l}); }
    else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (!he || !hr) return LOLHIP_ERR_INVALID;
  const int C = (int)cs.size();
  if (C_out) *C_out = C;
  if (C == 0) { if (T_out) *T_out = 0; return 0; }
  uint32_t m0 = 0; int T0 = 0;
  std::vector<int64_t> q0(cap_T > 0 ? (size_t)cap_T : 16), q1(q0.size());
  const int64_t n = lolhip_rqproduct_read(cs[0].p, cs[0].n, &m0, q0.data(), (int)q0.size(), &T0, nullptr, 0);
  if (n < 0) return n;
  if (m_out) *m_out = m0;
  if (T_out) *T_out = T0;
  if (qs) { if (cap_T < T0) return LOLHIP_ERR_INVALID; for (int t = 0; t < T0; ++t) qs[t] = q0[(size_t)t]; }
  if (!xs) return n;
  if (cap_xs < (int64_t)C * n * T0) return LOLHIP_ERR_INVALID;
  for (int i = 0; i < C; ++i) {
    uint32_t m1 = 0; int T1 = 0;
    const int64_t n1 = lolhip_rqproduct_read(cs[(size_t)i].p, cs[(size_t)i].n, &m1, q1.data(), (int)q1.size(), &T1,
                                             xs + (int64_t)i * n * T0, n * T0);
    if (n1 < 0) return n1;
    if (n1 != n || m1 != m0 || T1 != T0) return LOLHIP_ERR_INVALID;
    for (int t = 0; t < T0; ++t) if (q1[(size_t)t] != q0[(size_t)t]) return LOLHIP_ERR_INVALID;
  }
  return n;
}

// KSHint writer: xs [L][K][n][T] decoding-basis residues -> bytes (the inverse of lolhip_kshint_read;
// gad_a / gad_b are the two words of the gadget's GHC fingerprint, TypeRep, copied through).
int64_t lolhip_kshint_write(uint32_t m, const int64_t* qs, int T, int L, int K, const int64_t* xs, int64_t n,
                            uint64_t gad_a, uint64_t gad_b, uint8_t* out, int64_t cap) {
  if (!qs || T < 1 || L < 1 || K < 1 || n < 0 || (n > 0 && !xs)) return LOLHIP_ERR_INVALID;
  std::vector<int64_t> prod((size_t)L * K), poly((size_t)L);
  int64_t total = 0;
  for (int j = 0; j < L; ++j) {
    int64_t pl = 0;
    for (int k = 0; k < K; ++k) {
      const int64_t b = lolhip_rqproduct_write(m, qs, T, xs + ((int64_t)j * K + k) * n * T, n, nullptr, 0);
      if (b < 0) return b;
      prod[(size_t)j * K + k] = b;
      pl += 1 + varint_len((uint64_t)b) + b;
    }
    poly[(size_t)j] = pl;
    total += 1 + varint_len((uint64_t)pl) + pl;
  }
  const int64_t gl = 1 + varint_len(gad_a) + 1 + varint_len(gad_b);
  total += 1 + varint_len((uint64_t)gl) + gl;
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  for (int j = 0; j < L; ++j) {
    *o++ = 0x0A; put_varint(o, (uint64_t)poly[(size_t)j]);             // hint = 1
    for (int k = 0; k < K; ++k) {
      *o++ = 0x0A; put_varint(o, (uint64_t)prod[(size_t)j * K + k]);   // coeffs = 1
      const int64_t w = lolhip_rqproduct_write(m, qs, T, xs + ((int64_t)j * K + k) * n * T, n, o, prod[(size_t)j * K + k]);
      if (w < 0) return w;
      o += w;
    }
  }
  *o++ = 0x12; put_varint(o, (uint64_t)gl);                            // gad = 2
  *o++ = 0x08; put_varint(o, gad_a);
  *o++ = 0x10; put_varint(o, gad_b);
  return (int64_t)(o - out);
}

// message TunnelHint { LinearRq func = 1; repeated KSHint hint = 2; e = 3; r = 4; s = 5; p = 6; }
// (SHE.proto:26): one ring switch.  Returns the number of KSHints and the byte ranges
// (offset, length into buf) of the embedded LinearRq and of up to cap_hints KSHints, to be handed
// to lolhip_linearrq_read / lolhip_kshint_read.
int64_t lolhip_tunnelhint_read(const uint8_t* buf, int64_t len, uint32_t* e, uint32_t* r, uint32_t* s, uint64_t* p,
                               int64_t* func_off, int64_t* func_len, int64_t* hint_off, int64_t* hint_len, int cap_hints) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  Reader rd{buf, buf + len};
  bool hf = false, he = false, hr = false, hs = false, hp = false;
  int64_t nh = 0;
  while (rd.p < rd.end) {
    uint64_t key, v;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if ((field == 1 || field == 2) && wt == 2) {
      const uint8_t* b; int64_t l;
      if (!sub(rd, b, l)) return LOLHIP_ERR_INVALID;
      if (field == 1) { if (func_off) *func_off = b - buf; if (func_len) *func_len = l; hf = true; }
      else { if (nh < cap_hints) { if (hint_off) hint_off[nh] = b - buf; if (hint_len) hint_len[nh] = l; } ++nh; }
    } else if (field >= 3 && field <= 6 && wt == 0) {
      if (!rd.varint(v)) return LOLHIP_ERR_INVALID;
      if (field == 3) { if (e) *e = (uint32_t)v; he = true; }
      else if (field == 4) { if (r) *r = (uint32_t)v; hr = true; }
      else if (field == 5) { if (s) *s = (uint32_t)v; hs = true; }
      else { if (p) *p = v; hp = true; }
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (!(hf && he && hr && hs && hp)) return LOLHIP_ERR_INVALID;        // all `required`
  return nh;
}

// ---- round 3: the writers still missing, and the chain messages of lol-apps/HomomPRF.proto --------------------

// message R { required uint32 m = 1; repeated sint64 xs = 2; }: integer coefficients, decoding basis, as they stand.
int64_t lolhip_r_write(uint32_t m, const int64_t* xs, int64_t n, uint8_t* out, int64_t cap) {
  if (n < 0 || (n > 0 && !xs)) return LOLHIP_ERR_INVALID;
  int64_t total = 1 + varint_len(m);
  for (int64_t j = 0; j < n; ++j) total += 1 + varint_len(zigzag(xs[j]));
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  *o++ = 0x08; put_varint(o, m);
  for (int64_t j = 0; j < n; ++j) { *o++ = 0x10; put_varint(o, zigzag(xs[j])); }          // xs = 2, unpacked sint64
  return (int64_t)(o - out);
}

// message SecretKey { required R sk = 1; required double v = 2; }  (SHE.proto:9)
int64_t lolhip_secretkey_write(uint32_t m, double v, const int64_t* xs, int64_t n, uint8_t* out, int64_t cap) {
  const int64_t rl = lolhip_r_write(m, xs, n, nullptr, 0);
  if (rl < 0) return rl;
  const int64_t total = 1 + varint_len((uint64_t)rl) + rl + 1 + 8;
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  *o++ = 0x0A; put_varint(o, (uint64_t)rl);
  o += lolhip_r_write(m, xs, n, o, rl);
  *o++ = 0x11;                                                                              // v = 2, 64-bit
  std::memcpy(o, &v, 8); o += 8;
  return (int64_t)(o - out);
}

// message LinearRq { required uint32 e = 1; required uint32 r = 2; repeated RqProduct coeffs = 3; }  (Lol.proto:11)
// xs [C][n][T]: the function's values on the relative decoding basis, decoding-basis residues of the output ring m.
int64_t lolhip_linearrq_write(uint32_t e, uint32_t r, uint32_t m, const int64_t* qs, int T, int C, const int64_t* xs, int64_t n,
                              uint8_t* out, int64_t cap) {
  if (C < 0 || (C > 0 && n > 0 && !xs)) return LOLHIP_ERR_INVALID;
  std::vector<int64_t> pl((size_t)C);
  int64_t total = 1 + varint_len(e) + 1 + varint_len(r);
  for (int c = 0; c < C; ++c) {
    const int64_t b = lolhip_rqproduct_write(m, qs, T, xs + (int64_t)c * n * T, n, nullptr, 0);
    if (b < 0) return b;
    pl[(size_t)c] = b;
    total += 1 + varint_len((uint64_t)b) + b;
  }
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  *o++ = 0x08; put_varint(o, e);
  *o++ = 0x10; put_varint(o, r);
  for (int c = 0; c < C; ++c) {
    *o++ = 0x1A; put_varint(o, (uint64_t)pl[(size_t)c]);                                    // coeffs = 3
    const int64_t w = lolhip_rqproduct_write(m, qs, T, xs + (int64_t)c * n * T, n, o, pl[(size_t)c]);
    if (w < 0) return w;
    o += w;
  }
  return (int64_t)(o - out);
}

// message TunnelHint { LinearRq func = 1; repeated KSHint hint = 2; e = 3; r = 4; s = 5; p = 6; }  (SHE.proto:26),
// assembled from an encoded LinearRq and nh encoded KSHints (lolhip_linearrq_write / lolhip_kshint_write).
int64_t lolhip_tunnelhint_write(const uint8_t* func, int64_t func_len, const uint8_t* const* hints, const int64_t* hint_len, int nh,
                                uint32_t e, uint32_t r, uint32_t s, uint64_t p, uint8_t* out, int64_t cap) {
  if (!func || func_len < 0 || nh < 0 || (nh > 0 && (!hints || !hint_len))) return LOLHIP_ERR_INVALID;
  int64_t total = 1 + varint_len((uint64_t)func_len) + func_len + 1 + varint_len(e) + 1 + varint_len(r) + 1 + varint_len(s) + 1 + varint_len(p);
  for (int i = 0; i < nh; ++i) {
    if (!hints[i] || hint_len[i] < 0) return LOLHIP_ERR_INVALID;
    total += 1 + varint_len((uint64_t)hint_len[i]) + hint_len[i];
  }
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  *o++ = 0x0A; put_varint(o, (uint64_t)func_len); std::memcpy(o, func, (size_t)func_len); o += func_len;
  for (int i = 0; i < nh; ++i) { *o++ = 0x12; put_varint(o, (uint64_t)hint_len[i]); std::memcpy(o, hints[i], (size_t)hint_len[i]); o += hint_len[i]; }
  *o++ = 0x18; put_varint(o, e);
  *o++ = 0x20; put_varint(o, r);
  *o++ = 0x28; put_varint(o, s);
  *o++ = 0x30; put_varint(o, p);
  return (int64_t)(o - out);
}

// lol-apps/HomomPRF.proto:18-26 — LinearFuncChain { repeated LinearRq funcs = 1 }, TunnelHintChain { repeated TunnelHint
// hints = 1 }, RoundHintChain { repeated KSHint hints = 1 }: one `repeated` sub-message field each.  read: the number of
// elements and the byte ranges (offset, length into buf) of up to cap of them, for the element readers above.
int64_t lolhip_chain_read(const uint8_t* buf, int64_t len, int64_t* off, int64_t* elem_len, int cap) {
  if (!buf || len < 0) return LOLHIP_ERR_INVALID;
  Reader rd{buf, buf + len};
  int64_t cnt = 0;
  while (rd.p < rd.end) {
    uint64_t key;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t field = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (field == 1 && wt == 2) {
      const uint8_t* b; int64_t l;
      if (!sub(rd, b, l)) return LOLHIP_ERR_INVALID;
      if (cnt < cap) { if (off) off[cnt] = b - buf; if (elem_len) elem_len[cnt] = l; }
      ++cnt;
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  return cnt;
}
int64_t lolhip_chain_write(const uint8_t* const* elems, const int64_t* elem_len, int count, uint8_t* out, int64_t cap) {
  if (count < 0 || (count > 0 && (!elems || !elem_len))) return LOLHIP_ERR_INVALID;
  int64_t total = 0;
  for (int i = 0; i < count; ++i) {
    if (!elems[i] || elem_len[i] < 0) return LOLHIP_ERR_INVALID;
    total += 1 + varint_len((uint64_t)elem_len[i]) + elem_len[i];
  }
  if (!out) return total;
  if (cap < total) return LOLHIP_ERR_INVALID;
  uint8_t* o = out;
  for (int i = 0; i < count; ++i) { *o++ = 0x0A; put_varint(o, (uint64_t)elem_len[i]); std::memcpy(o, elems[i], (size_t)elem_len[i]); o += elem_len[i]; }
  return (int64_t)(o - out);
}

}  // extern "C"

// ---- rlwe-challenges: RLWE.proto (SampleCont/Disc/RLWR[Product]) and Challenges.proto (Challenge, *Params,
// Instance*[Product], Secret[Product]) ----------------------------------------------------------------------------
// kind: 0 = Disc, 1 = Cont, 2 = RLWR, as in lolhip_rlwe_*.  The parameters of a kind travel as ip [4] = (m, q, x,
// numSamples) with x = the int64 bound (Disc), unused (Cont) or p (RLWR), and dp [2] = (svar, the double bound of Cont).
// Ring elements are read in either generation (Verify.hs:199-232): the legacy forms hold one Rq / Kq, the Product
// forms an RqProduct / KqProduct; the first field 1 of the element tells them apart (varint m, or length-delimited
// rqlist).  Both are read through lolhip_rqproduct_read / lolhip_kqproduct_read, a legacy element as a list of one.

namespace {

typedef std::vector<uint8_t> Bytes;
enum { CH_DISC = 0, CH_CONT = 1, CH_RLWR = 2, CH_MAX_T = 64 };

void pv(Bytes& o, uint64_t v) { while (v >= 0x80) { o.push_back((uint8_t)(v | 0x80)); v >>= 7; } o.push_back((uint8_t)v); }
void ptag(Bytes& o, uint32_t f, uint32_t wt) { pv(o, (uint64_t)f << 3 | wt); }
void pint(Bytes& o, uint32_t f, int64_t v) { ptag(o, f, 0); pv(o, (uint64_t)v); }      // int32 / int64: two's complement
void pdbl(Bytes& o, uint32_t f, double d) { ptag(o, f, 1); uint8_t b[8]; std::memcpy(b, &d, 8); o.insert(o.end(), b, b + 8); }
void pbytes(Bytes& o, uint32_t f, const uint8_t* p, size_t n) { ptag(o, f, 2); pv(o, n); if (n) o.insert(o.end(), p, p + n); }
void psub(Bytes& o, uint32_t f, const Bytes& s) { pbytes(o, f, s.data(), s.size()); }

int64_t emit(const Bytes& o, uint8_t* out, int64_t cap) {
  if (!out) return (int64_t)o.size();
  if (cap < (int64_t)o.size()) return LOLHIP_ERR_INVALID;
  if (!o.empty()) std::memcpy(out, o.data(), o.size());
  return (int64_t)o.size();
}

bool kind_ok(int kind) { return kind >= CH_DISC && kind <= CH_RLWR; }

void params_bytes(Bytes& o, int kind, const int64_t* ip, const double* dp) {
  pint(o, 1, ip[0]); pint(o, 2, ip[1]);
  if (kind == CH_RLWR) { pint(o, 3, ip[2]); pint(o, 4, ip[3]); return; }
  pdbl(o, 3, dp[0]);
  if (kind == CH_CONT) pdbl(o, 4, dp[1]); else pint(o, 4, ip[2]);
  pint(o, 5, ip[3]);
}

// every field of the kind's message is `required`
int params_read(const uint8_t* b, int64_t l, int kind, int64_t* ip, double* dp) {
  Reader rd{b, b + l};
  unsigned seen = 0;
  ip[0] = ip[1] = ip[2] = ip[3] = 0; dp[0] = dp[1] = 0;
  while (rd.p < rd.end) {
    uint64_t key, v = 0;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t f = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    const bool dbl = wt == 1 && rd.end - rd.p >= 8;
    if (wt == 1 && !dbl) return LOLHIP_ERR_INVALID;
    const int last = kind == CH_RLWR ? 4 : 5;
    if (f == 1 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; ip[0] = (int32_t)v; seen |= 1; }
    else if (f == 2 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; ip[1] = (int64_t)v; seen |= 2; }
    else if ((int)f == last && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; ip[3] = (int32_t)v; seen |= 16; }
    else if (kind == CH_RLWR && f == 3 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; ip[2] = (int64_t)v; seen |= 4 | 8; }
    else if (kind != CH_RLWR && f == 3 && dbl) { dp[0] = f64_at(rd.p); rd.p += 8; seen |= 4; }
    else if (kind == CH_CONT && f == 4 && dbl) { dp[1] = f64_at(rd.p); rd.p += 8; seen |= 8; }
    else if (kind == CH_DISC && f == 4 && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; ip[2] = (int64_t)v; seen |= 8; }
    else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  return seen == 31 ? LOLHIP_OK : LOLHIP_ERR_INVALID;
}

// one ring element of either generation
struct Elem {
  bool product = false;
  uint32_t m = 0;
  int T = 0;
  int64_t n = 0;
  std::vector<int64_t> qs, xi;      // xi [n][T] canonical residues (integer elements)
  std::vector<double> xd;           // xd [n][T] (Kq elements)
};

int elem_read(const uint8_t* b, int64_t l, bool dbl, Elem& e) {
  // the generation: the wire type of the first field 1
  Reader rd{b, b + l};
  int gen = -1;
  while (rd.p < rd.end && gen < 0) {
    uint64_t key;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    if ((key >> 3) == 1) gen = (key & 7) == 0 ? 0 : (key & 7) == 2 ? 1 : 2;
    else if (!rd.skip((uint32_t)(key & 7))) return LOLHIP_ERR_INVALID;
  }
  if (gen != 0 && gen != 1) return LOLHIP_ERR_INVALID;      // no field 1: m, or a non-empty list, is required
  e.product = gen == 1;
  Bytes wrapped;
  if (!e.product) {                                         // a legacy element as a list of one
    wrapped.push_back(0x0A); pv(wrapped, (uint64_t)l);
    wrapped.insert(wrapped.end(), b, b + l);
    b = wrapped.data(); l = (int64_t)wrapped.size();
  }
  e.qs.assign(CH_MAX_T, 0);
  int64_t n = dbl ? lolhip_kqproduct_read(b, l, &e.m, e.qs.data(), CH_MAX_T, &e.T, nullptr, 0)
                  : lolhip_rqproduct_read(b, l, &e.m, e.qs.data(), CH_MAX_T, &e.T, nullptr, 0);
  if (n < 0) return (int)n;
  e.n = n;
  e.qs.resize((size_t)e.T);
  if (dbl) { e.xd.assign((size_t)(n * e.T), 0.0); n = lolhip_kqproduct_read(b, l, nullptr, nullptr, 0, nullptr, e.xd.data(), n * e.T); }
  else { e.xi.assign((size_t)(n * e.T), 0); n = lolhip_rqproduct_read(b, l, nullptr, nullptr, 0, nullptr, e.xi.data(), n * e.T); }
  return n < 0 ? (int)n : LOLHIP_OK;
}

// the moduli of an element against the modulus q of its parameters: one modulus equal to q, or a tuple whose product is q
bool moduli_are(const std::vector<int64_t>& qs, int64_t q) {
  unsigned __int128 prod = 1;
  for (int64_t v : qs) { if (v < 1) return false; prod *= (unsigned __int128)v; if (prod >> 64) return false; }
  return q > 0 && prod == (unsigned __int128)q;
}

int elem_int_bytes(Bytes& o, bool legacy, uint32_t m, const int64_t* qs, int T, const int64_t* xs, int64_t n) {
  if (legacy && T != 1) return LOLHIP_ERR_INVALID;
  const int64_t len = lolhip_rqproduct_write(m, qs, T, xs, n, nullptr, 0);
  if (len < 0) return (int)len;
  Bytes tmp((size_t)len);
  const int64_t w = lolhip_rqproduct_write(m, qs, T, xs, n, tmp.data(), len);
  if (w != len) return LOLHIP_ERR_INVALID;
  size_t skip = 0;
  if (legacy) { skip = 1; while (tmp[skip] & 0x80) ++skip; ++skip; }        // the rqlist tag and its length
  o.insert(o.end(), tmp.begin() + (long)skip, tmp.end());
  return LOLHIP_OK;
}

int elem_dbl_bytes(Bytes& o, bool legacy, uint32_t m, const int64_t* qs, int T, const double* xs, int64_t n) {
  if (legacy && T != 1) return LOLHIP_ERR_INVALID;
  for (int t = 0; t < T; ++t) {
    if (qs[t] < 2) return LOLHIP_ERR_MODULUS;
    Bytes kq;
    pint(kq, 1, m); pint(kq, 2, qs[t]);
    for (int64_t j = 0; j < n; ++j) pdbl(kq, 3, xs[j * T + t]);
    if (legacy) o.insert(o.end(), kq.begin(), kq.end()); else psub(o, 1, kq);
  }
  return LOLHIP_OK;
}

}  // namespace

extern "C" {

int64_t lolhip_challenge_read(const uint8_t* buf, int64_t len, int64_t* hdr, int* kind_out, int64_t* ip, double* dp) {
  if (!buf || len < 0 || !hdr || !kind_out || !ip || !dp) return LOLHIP_ERR_INVALID;
  Reader rd{buf, buf + len};
  unsigned seen = 0;
  int kind = -1;
  const uint8_t* pb = nullptr; int64_t pl = 0;
  while (rd.p < rd.end) {
    uint64_t key, v = 0;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t f = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (f >= 1 && f <= 4 && wt == 0) {
      if (!rd.varint(v)) return LOLHIP_ERR_INVALID;
      hdr[f - 1] = f == 3 ? (int64_t)v : (int64_t)(int32_t)v;
      seen |= 1u << (f - 1);
    } else if (f >= 5 && f <= 7 && wt == 2) {               // the oneof: the last arm on the wire wins
      if (!sub(rd, pb, pl)) return LOLHIP_ERR_INVALID;
      kind = f == 5 ? CH_CONT : f == 6 ? CH_DISC : CH_RLWR;
    } else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (seen != 15 || kind < 0) return LOLHIP_ERR_INVALID;
  *kind_out = kind;
  return params_read(pb, pl, kind, ip, dp);
}

int64_t lolhip_challenge_write(const int64_t* hdr, int kind, const int64_t* ip, const double* dp, uint8_t* out, int64_t cap) {
  if (!hdr || !ip || !dp || !kind_ok(kind)) return LOLHIP_ERR_INVALID;
  Bytes o, pr;
  for (uint32_t f = 1; f <= 4; ++f) pint(o, f, hdr[f - 1]);
  params_bytes(pr, kind, ip, dp);
  psub(o, kind == CH_CONT ? 5 : kind == CH_DISC ? 6 : 7, pr);
  return emit(o, out, cap);
}

// Instance{Cont,Disc,RLWR}[Product] -> ids [2] = (challengeID, instanceID), the parameters, and the samples: a
// [L][n][T] residues, b [L][n][T] residues mod q (Disc) or mod p (RLWR), or doubles (Cont).  Pass a = b = NULL to
// query count_out = L, T_out, qs and the return value n; product_out = 1 when the samples are the Product forms.
// LOLHIP_ERR_INVALID for truncated data, a missing required field, samples of mixed generations or shapes, or an m or
// q of a sample that disagrees with the parameters (b of an RLWR sample is over p).
int64_t lolhip_instance_read(const uint8_t* buf, int64_t len, int kind, int64_t* ids, int64_t* ip, double* dp, int* product_out,
                             int* T_out, int64_t* qs, int cap_T, int64_t* count_out, int64_t* a, int64_t cap_a, void* b,
                             int64_t cap_b) {
  if (!buf || len < 0 || !kind_ok(kind) || !ids || !ip || !dp) return LOLHIP_ERR_INVALID;
  struct Span { const uint8_t* p; int64_t n; };
  std::vector<Span> samples;
  Reader rd{buf, buf + len};
  unsigned seen = 0;
  const uint8_t* pb = nullptr; int64_t pl = 0;
  while (rd.p < rd.end) {
    uint64_t key, v = 0;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t f = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if ((f == 1 || f == 2) && wt == 0) { if (!rd.varint(v)) return LOLHIP_ERR_INVALID; ids[f - 1] = (int32_t)v; seen |= f; }
    else if (f == 3 && wt == 2) { if (!sub(rd, pb, pl)) return LOLHIP_ERR_INVALID; seen |= 4; }
    else if (f == 4 && wt == 2) { Span s; if (!sub(rd, s.p, s.n)) return LOLHIP_ERR_INVALID; samples.push_back(s); }
    else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (seen != 7) return LOLHIP_ERR_INVALID;
  int rc = params_read(pb, pl, kind, ip, dp); if (rc) return rc;
  const int64_t L = (int64_t)samples.size();
  int T = 0, product = -1;
  int64_t n = 0;
  std::vector<int64_t> q0;
  for (int64_t i = 0; i < L; ++i) {
    Reader sr{samples[(size_t)i].p, samples[(size_t)i].p + samples[(size_t)i].n};
    const uint8_t *ab = nullptr, *bb = nullptr; int64_t al = 0, bl = 0;
    while (sr.p < sr.end) {
      uint64_t key;
      if (!sr.varint(key)) return LOLHIP_ERR_INVALID;
      const uint32_t f = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
      if (f == 1 && wt == 2) { if (!sub(sr, ab, al)) return LOLHIP_ERR_INVALID; }
      else if (f == 2 && wt == 2) { if (!sub(sr, bb, bl)) return LOLHIP_ERR_INVALID; }
      else if (!sr.skip(wt)) return LOLHIP_ERR_INVALID;
    }
    if (!ab || !bb) return LOLHIP_ERR_INVALID;
    Elem ea, eb;
    rc = elem_read(ab, al, false, ea); if (rc) return rc;
    rc = elem_read(bb, bl, kind == CH_CONT, eb); if (rc) return rc;
    if (i == 0) { T = ea.T; n = ea.n; product = ea.product; q0 = ea.qs; }
    if (ea.product != (product != 0) || eb.product != ea.product || ea.T != T || eb.T != T || ea.n != n || eb.n != n)
      return LOLHIP_ERR_INVALID;
    if ((int64_t)ea.m != ip[0] || (int64_t)eb.m != ip[0] || ea.qs != q0 || !moduli_are(ea.qs, ip[1])) return LOLHIP_ERR_INVALID;
    if (kind == CH_RLWR ? !moduli_are(eb.qs, ip[2]) : eb.qs != q0) return LOLHIP_ERR_INVALID;
    if (a) {
      if (!b || cap_a < L * n * T || cap_b < L * n * T) return LOLHIP_ERR_INVALID;
      std::memcpy(a + i * n * T, ea.xi.data(), sizeof(int64_t) * (size_t)(n * T));
      if (kind == CH_CONT) std::memcpy(static_cast<double*>(b) + i * n * T, eb.xd.data(), sizeof(double) * (size_t)(n * T));
      else std::memcpy(static_cast<int64_t*>(b) + i * n * T, eb.xi.data(), sizeof(int64_t) * (size_t)(n * T));
    }
  }
  if (product_out) *product_out = product > 0;
  if (T_out) *T_out = T;
  if (count_out) *count_out = L;
  if (qs) { if (cap_T < T) return LOLHIP_ERR_INVALID; for (int t = 0; t < T; ++t) qs[t] = q0[(size_t)t]; }
  return n;
}

// the Product forms (what Generate.hs writes), or with legacy != 0 the forms of the 2016 release (T = 1).  qs [T]: the
// moduli of a (and of the Disc / Cont b); the RLWR b is written over p = ip[2].
int64_t lolhip_instance_write(int kind, int legacy, const int64_t* ids, const int64_t* ip, const double* dp, const int64_t* qs,
                              int T, int64_t L, int64_t n, const int64_t* a, const void* b, uint8_t* out, int64_t cap) {
  if (!kind_ok(kind) || !ids || !ip || !dp || !qs || T < 1 || T > CH_MAX_T || L < 0 || n < 0) return LOLHIP_ERR_INVALID;
  if (L * n > 0 && (!a || !b)) return LOLHIP_ERR_INVALID;
  if (kind == CH_RLWR && T != 1) return LOLHIP_ERR_INVALID;
  Bytes o, pr;
  pint(o, 1, ids[0]); pint(o, 2, ids[1]);
  params_bytes(pr, kind, ip, dp);
  psub(o, 3, pr);
  const uint32_t m = (uint32_t)ip[0];
  const int64_t pq[1] = {ip[2]};
  for (int64_t i = 0; i < L; ++i) {
    Bytes sa, sb, smp;
    int rc = elem_int_bytes(sa, legacy != 0, m, qs, T, a + i * n * T, n); if (rc) return rc;
    if (kind == CH_CONT) rc = elem_dbl_bytes(sb, legacy != 0, m, qs, T, static_cast<const double*>(b) + i * n * T, n);
    else rc = elem_int_bytes(sb, legacy != 0, m, kind == CH_RLWR ? pq : qs, T, static_cast<const int64_t*>(b) + i * n * T, n);
    if (rc) return rc;
    psub(smp, 1, sa); psub(smp, 2, sb);
    psub(o, 4, smp);
  }
  return emit(o, out, cap);
}

// Secret / SecretProduct -> ids [2], m, q, the seed bytes (seed_len_out; copied when cap_seed holds them) and s [n][T].
// Returns n; xs = NULL queries.  LOLHIP_ERR_INVALID also when the element's m or moduli disagree with the message's.
int64_t lolhip_secret_read(const uint8_t* buf, int64_t len, int64_t* ids, int64_t* m_out, int64_t* q_out, uint8_t* seed,
                           int64_t cap_seed, int64_t* seed_len_out, int* product_out, int* T_out, int64_t* qs, int cap_T,
                           int64_t* xs, int64_t cap_xs) {
  if (!buf || len < 0 || !ids) return LOLHIP_ERR_INVALID;
  Reader rd{buf, buf + len};
  unsigned seen = 0;
  int64_t m = 0, q = 0, sl = 0, el = 0;
  const uint8_t *sb = nullptr, *eb = nullptr;
  while (rd.p < rd.end) {
    uint64_t key, v = 0;
    if (!rd.varint(key)) return LOLHIP_ERR_INVALID;
    const uint32_t f = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
    if (f >= 1 && f <= 4 && wt == 0) {
      if (!rd.varint(v)) return LOLHIP_ERR_INVALID;
      if (f <= 2) ids[f - 1] = (int32_t)v; else if (f == 3) m = (int32_t)v; else q = (int64_t)v;
      seen |= 1u << (f - 1);
    } else if (f == 5 && wt == 2) { if (!sub(rd, sb, sl)) return LOLHIP_ERR_INVALID; seen |= 16; }
    else if (f == 6 && wt == 2) { if (!sub(rd, eb, el)) return LOLHIP_ERR_INVALID; seen |= 32; }
    else if (!rd.skip(wt)) return LOLHIP_ERR_INVALID;
  }
  if (seen != 63) return LOLHIP_ERR_INVALID;
  Elem e;
  const int rc = elem_read(eb, el, false, e); if (rc) return rc;
  if ((int64_t)e.m != m || !moduli_are(e.qs, q)) return LOLHIP_ERR_INVALID;
  if (m_out) *m_out = m;
  if (q_out) *q_out = q;
  if (seed_len_out) *seed_len_out = sl;
  if (seed) { if (cap_seed < sl) return LOLHIP_ERR_INVALID; if (sl) std::memcpy(seed, sb, (size_t)sl); }
  if (product_out) *product_out = e.product;
  if (T_out) *T_out = e.T;
  if (qs) { if (cap_T < e.T) return LOLHIP_ERR_INVALID; for (int t = 0; t < e.T; ++t) qs[t] = e.qs[(size_t)t]; }
  if (xs) { if (cap_xs < e.n * e.T) return LOLHIP_ERR_INVALID; std::memcpy(xs, e.xi.data(), sizeof(int64_t) * (size_t)(e.n * e.T)); }
  return e.n;
}

int64_t lolhip_secret_write(int legacy, const int64_t* ids, int64_t m, int64_t q, const uint8_t* seed, int64_t seed_len,
                            const int64_t* qs, int T, const int64_t* xs, int64_t n, uint8_t* out, int64_t cap) {
  if (!ids || !qs || T < 1 || T > CH_MAX_T || n < 0 || seed_len < 0 || (seed_len > 0 && !seed) || (n > 0 && !xs))
    return LOLHIP_ERR_INVALID;
  Bytes o, s;
  pint(o, 1, ids[0]); pint(o, 2, ids[1]); pint(o, 3, m); pint(o, 4, q);
  pbytes(o, 5, seed, (size_t)seed_len);
  const int rc = elem_int_bytes(s, legacy != 0, (uint32_t)m, qs, T, xs, n); if (rc) return rc;
  psub(o, 6, s);
  return emit(o, out, cap);
}

}  // extern "C"
