// tests/native/challenge_wire_sanitize.cpp — stand-alone driver for the rlwe-challenges messages of lol_amd/csrc/wire.cpp
// (Challenge, Instance*[Product], Secret[Product]), compiled with wire.cpp under -fsanitize=address,undefined by
// tests/test_challenge_host.py.  It writes every message in both generations, reads it back and compares, and then
// feeds the readers every prefix of each message and each message with one byte changed at every position: a reader
// answers a status or a length and never reads outside its buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lolhip.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

namespace {

typedef std::vector<uint8_t> Bytes;
constexpr int N = 6, L = 3;

// every reader on one buffer given as an exact-size heap copy, so one byte past the end is a sanitizer report
void read_all(const uint8_t* p, int64_t len) {
  Bytes copy(p, p + len);
  const uint8_t* b = copy.empty() ? reinterpret_cast<const uint8_t*>("") : copy.data();
  int64_t hdr[4], ip[4], ids[2], qs[64], cnt = 0, m = 0, q = 0, sl = 0, a[L * N], xi[L * N];
  double dp[2], xd[L * N];
  uint8_t seed[64];
  int kind = 0, prod = 0, T = 0;
  lolhip_challenge_read(b, len, hdr, &kind, ip, dp);
  for (int k = 0; k < 3; ++k) {
    lolhip_instance_read(b, len, k, ids, ip, dp, &prod, &T, qs, 64, &cnt, nullptr, 0, nullptr, 0);
    lolhip_instance_read(b, len, k, ids, ip, dp, &prod, &T, qs, 64, &cnt, a, L * N, k == 1 ? (void*)xd : (void*)xi, L * N);
  }
  lolhip_secret_read(b, len, ids, &m, &q, nullptr, 0, &sl, &prod, &T, qs, 64, nullptr, 0);
  lolhip_secret_read(b, len, ids, &m, &q, seed, 64, &sl, &prod, &T, qs, 64, xi, L * N);
}

void torture(const Bytes& msg) {
  for (size_t cut = 0; cut <= msg.size(); ++cut) read_all(msg.data(), (int64_t)cut);
  Bytes x = msg;
  for (size_t i = 0; i < x.size(); ++i) {
    for (uint8_t flip : {uint8_t(0x01), uint8_t(0x80), uint8_t(0xFF)}) {
      x[i] ^= flip;
      read_all(x.data(), (int64_t)x.size());
      x[i] ^= flip;
    }
  }
}

}  // namespace

int main() {
  const int64_t m = 7, q = 97, p = 5;
  const int64_t qs[1] = {q};
  int64_t a[L * N], bi[L * N], s[N];
  double bd[L * N];
  for (int i = 0; i < L * N; ++i) { a[i] = (i * 37 + 5) % q; bi[i] = (i * 11 + 96) % q; bd[i] = 0.5 + i * 1.25; }
  for (int i = 0; i < N; ++i) s[i] = (i * 53 + 48) % q;
  uint8_t seed[48];
  for (int i = 0; i < 48; ++i) seed[i] = (uint8_t)(i * 5);

  // Challenge, the three arms
  for (int kind = 0; kind < 3; ++kind) {
    const int64_t hdr[4] = {515, 32, 1478822400, 63}, ip[4] = {m, q, kind == 2 ? p : 414, L};
    const double dp[2] = {0.5, 112.5};
    const int64_t len = lolhip_challenge_write(hdr, kind, ip, dp, nullptr, 0);
    CHECK(len > 0);
    Bytes msg((size_t)len);
    CHECK(lolhip_challenge_write(hdr, kind, ip, dp, msg.data(), len) == len);
    CHECK(lolhip_challenge_write(hdr, kind, ip, dp, msg.data(), len - 1) == LOLHIP_ERR_INVALID);
    int64_t h2[4], ip2[4]; double dp2[2]; int k2 = -1;
    CHECK(lolhip_challenge_read(msg.data(), len, h2, &k2, ip2, dp2) == 0 && k2 == kind);
    CHECK(!std::memcmp(hdr, h2, sizeof hdr) && ip2[0] == m && ip2[1] == q && ip2[3] == L);
    CHECK(kind == 1 ? dp2[1] == 112.5 : ip2[2] == ip[2]);
    CHECK(lolhip_challenge_read(msg.data(), len - 1, h2, &k2, ip2, dp2) == LOLHIP_ERR_INVALID);
    torture(msg);
  }
  // Instance, three kinds, both generations
  for (int kind = 0; kind < 3; ++kind)
    for (int legacy = 0; legacy < 2; ++legacy) {
      const int64_t ids[2] = {515, 31}, ip[4] = {m, q, kind == 2 ? p : 414, L};
      const double dp[2] = {0.5, 112.5};
      int64_t bp[L * N];
      for (int i = 0; i < L * N; ++i) bp[i] = bi[i] % p;
      const void* b = kind == 1 ? (const void*)bd : kind == 2 ? (const void*)bp : (const void*)bi;
      const int64_t len = lolhip_instance_write(kind, legacy, ids, ip, dp, qs, 1, L, N, a, b, nullptr, 0);
      CHECK(len > 0);
      Bytes msg((size_t)len);
      CHECK(lolhip_instance_write(kind, legacy, ids, ip, dp, qs, 1, L, N, a, b, msg.data(), len) == len);
      int64_t i2[2], ip2[4], q2[4], cnt = 0, a2[L * N], b2[L * N];
      double dp2[2], d2[L * N];
      int prod = -1, T = 0;
      CHECK(lolhip_instance_read(msg.data(), len, kind, i2, ip2, dp2, &prod, &T, q2, 4, &cnt, nullptr, 0, nullptr, 0) == N);
      CHECK(prod == !legacy && T == 1 && cnt == L && q2[0] == q && i2[0] == 515 && i2[1] == 31);
      CHECK(lolhip_instance_read(msg.data(), len, kind, i2, ip2, dp2, &prod, &T, q2, 4, &cnt, a2, L * N,
                                 kind == 1 ? (void*)d2 : (void*)b2, L * N) == N);
      CHECK(!std::memcmp(a, a2, sizeof a));
      CHECK(kind == 1 ? !std::memcmp(bd, d2, sizeof bd) : !std::memcmp(kind == 2 ? bp : bi, b2, sizeof b2));
      CHECK(lolhip_instance_read(msg.data(), len, kind, i2, ip2, dp2, &prod, &T, q2, 4, &cnt, a2, L * N - 1,
                                 kind == 1 ? (void*)d2 : (void*)b2, L * N) == LOLHIP_ERR_INVALID);
      CHECK(lolhip_instance_read(msg.data(), len - 1, kind, i2, ip2, dp2, &prod, &T, q2, 4, &cnt, nullptr, 0, nullptr, 0) < 0);
      // the parameters say another modulus than the samples carry
      const int64_t ipq[4] = {m, q + 4, ip[2], L};
      const int64_t l3 = lolhip_instance_write(kind, legacy, ids, ipq, dp, qs, 1, L, N, a, b, nullptr, 0);
      Bytes bad((size_t)l3);
      CHECK(lolhip_instance_write(kind, legacy, ids, ipq, dp, qs, 1, L, N, a, b, bad.data(), l3) == l3);
      CHECK(lolhip_instance_read(bad.data(), l3, kind, i2, ip2, dp2, &prod, &T, q2, 4, &cnt, nullptr, 0, nullptr, 0) ==
            LOLHIP_ERR_INVALID);
      torture(msg);
    }
  // Secret, both generations
  for (int legacy = 0; legacy < 2; ++legacy) {
    const int64_t ids[2] = {515, 31};
    const int64_t len = lolhip_secret_write(legacy, ids, m, q, seed, 48, qs, 1, s, N, nullptr, 0);
    CHECK(len > 0);
    Bytes msg((size_t)len);
    CHECK(lolhip_secret_write(legacy, ids, m, q, seed, 48, qs, 1, s, N, msg.data(), len) == len);
    int64_t i2[2], m2 = 0, q2 = 0, sl = 0, qq[4], s2[N];
    uint8_t sd[48];
    int prod = -1, T = 0;
    CHECK(lolhip_secret_read(msg.data(), len, i2, &m2, &q2, nullptr, 0, &sl, &prod, &T, qq, 4, nullptr, 0) == N);
    CHECK(sl == 48 && prod == !legacy && T == 1 && m2 == m && q2 == q);
    CHECK(lolhip_secret_read(msg.data(), len, i2, &m2, &q2, sd, 48, &sl, &prod, &T, qq, 4, s2, N) == N);
    CHECK(!std::memcmp(sd, seed, 48) && !std::memcmp(s, s2, sizeof s));
    CHECK(lolhip_secret_read(msg.data(), len, i2, &m2, &q2, sd, 47, &sl, &prod, &T, qq, 4, s2, N) == LOLHIP_ERR_INVALID);
    torture(msg);
  }
  std::printf("challenge wire sanitize ok\n");
  return 0;
}
