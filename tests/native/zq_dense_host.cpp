// tests/native/zq_dense_host.cpp — the host side of the dense Z_q stages (LOLHIP_ROUTE_DENSE_ZQ) under
// AddressSanitizer and UBSan: a stand-alone program over the product's host sources and device_stubs.cpp
// (tests/test_zq_dense_sanitize.py builds and runs it).  Plans are host-only: create / destroy over a grid of indices x
// moduli x route words, both queries on every stage, the table read-backs with cap 0, 1 and exact into buffers with
// a guard word behind them, and the compute entries, which answer LOLHIP_ERR_NO_DEVICE.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lolhip.h"

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static std::vector<lolhip_pp> factor(int64_t m) {
  std::vector<lolhip_pp> out;
  for (int64_t p = 2; m > 1; p += (p == 2 ? 1 : 2)) {
    if (p * p > m) p = m;
    int e = 0;
    while (m % p == 0) { m /= p; ++e; }
    if (e) out.push_back(lolhip_pp{(int16_t)p, (int16_t)e});
  }
  return out;
}

static void tables(const lolhip_plan* p, int T, int route) {
  int64_t prog[4 * 64];
  for (int inverse = 0; inverse < 2; ++inverse) {
    const int64_t len = lolhip_plan_table(p, 10 + inverse, 0, prog, 4 * 64);
    CHECK(len % 4 == 0 && len <= 4 * 64);
    int dense = 0;
    for (int st = -1; st <= len / 4; ++st)
      for (int t = -1; t <= T; ++t)
        for (int limb = -2; limb <= 5; ++limb) {
          const int64_t cnt = lolhip_plan_zq_table(p, inverse, st, t, limb, nullptr, 0);
          CHECK(cnt >= 0);
          if (st < 0 || st >= len / 4 || t < 0 || t >= T || limb < -1 || !route) CHECK(cnt == 0);
          if (!cnt) continue;
          ++dense;
          const int64_t d = prog[4 * st + 2];
          CHECK(prog[4 * st + 1] > 13);
          CHECK(cnt == (limb < 0 ? d * d : ((d + 31) / 32 * 32) * ((d + 31) / 32 * 32)));
          for (int64_t cap : {(int64_t)0, (int64_t)1, cnt}) {
            std::vector<int64_t> buf((size_t)cap + 1, 0x5a5a5a5a5a5a5a5a);
            CHECK(lolhip_plan_zq_table(p, inverse, st, t, limb, buf.data(), cap) == cnt);
            CHECK(buf[(size_t)cap] == 0x5a5a5a5a5a5a5a5a);
            if (limb >= 0) for (int64_t i = 0; i < cap; ++i) CHECK(buf[(size_t)i] >= -128 && buf[(size_t)i] <= 127);
          }
        }
    CHECK((dense > 0) == (route > 0));
  }
}

int main() {
  const int64_t indices[] = {17, 19, 37, 51, 289, 323, 68, 544, 257, 45, 64, 17 * 2048};
  // per index: moduli = 1 (mod m) found by search from these lower bounds; 0 marks "no CRT basis" (q = 2^11)
  const int64_t lowers[] = {1000, 65279, 16711423, 4278124287ll, (int64_t)1 << 32, (int64_t)1 << 58, 0};
  int plans = 0, routed = 0;
  for (int64_t m : indices) {
    const std::vector<lolhip_pp> pps = factor(m);
    for (int64_t lo : lowers)
      for (int T = 1; T <= 2; ++T) {
        int64_t qs[2];
        qs[0] = lo ? lolhip_good_q(m, lo) : 2048;
        qs[1] = lo ? lolhip_good_q(m, qs[0]) : 2048;
        CHECK(qs[0] >= 2 && qs[1] >= 2);
        for (uint32_t flags : {0u, 1u, 2u})
          for (uint32_t routes : {0u, 1u, 2u, 3u, 0x80000000u}) {
            lolhip_plan* p = nullptr;
            const int rc = lolhip_plan_create_routes(pps.data(), (int)pps.size(), qs, T, 1, flags, routes, &p);
            if (flags > 1 || routes > 1) { CHECK(rc == LOLHIP_ERR_INVALID && !p); continue; }
            CHECK(rc == LOLHIP_OK && p);
            ++plans;
            const int r0 = lolhip_plan_zq_route(p, 0), r1 = lolhip_plan_zq_route(p, 1);
            const int r2 = lolhip_plan_zq_route(p, 2);       // the poly-mul: one dense launch on the transforms' route, or composed
            CHECK(r0 == r1 && r0 >= 0 && r0 <= 2 && (r2 == 0 || r2 == r0));
            if (m == 544 || (qs[0] >> 32 && lolhip_plan_n(p) > 4864)) CHECK(r2 == 0);
            CHECK(lolhip_plan_zq_route(p, -1) == 0 && lolhip_plan_zq_route(p, 3) == 0);
            if (!routes || !lolhip_plan_has_crt(p) || lolhip_plan_n(p) > 8192 || m == 45 || m == 64) CHECK(r0 == 0);
            else CHECK(r0 >= 1);
            if (r0 == 2) CHECK(qs[0] <= 4278124287ll && (T == 1 || qs[1] <= 4278124287ll));
            routed += r0 > 0;
            tables(p, T, r0);
            CHECK(lolhip_debug_set("ZQ_DENSE_VALU", 1) == LOLHIP_OK);
            CHECK(lolhip_plan_zq_route(p, 0) == (r0 ? 1 : 0));
            tables(p, T, r0 ? 1 : 0);
            CHECK(lolhip_debug_set("GENERIC_SCALAR", 1) == LOLHIP_OK);
            CHECK(lolhip_plan_zq_route(p, 0) == 0);
            tables(p, T, 0);
            CHECK(lolhip_debug_set("GENERIC_SCALAR", 0) == LOLHIP_OK && lolhip_debug_set("ZQ_DENSE_VALU", 0) == LOLHIP_OK);
            // host-only: every compute entry says so before it looks at its pointers
            int64_t y[4] = {0, 0, 0, 0};
            CHECK(lolhip_crt_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_crtinv_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_polymul_batch(p, nullptr, y, y, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_mul_batch(p, nullptr, y, y, 1) == LOLHIP_ERR_NO_DEVICE);
            lolhip_plan_destroy(p);
          }
      }
  }
  CHECK(lolhip_plan_zq_route(nullptr, 0) == 0 && lolhip_plan_zq_table(nullptr, 0, 0, 0, -1, nullptr, 0) == 0);
  lolhip_plan* p = nullptr;
  CHECK(lolhip_plan_create_routes(nullptr, 0, nullptr, 1, 1, 0, 1, &p) == LOLHIP_ERR_INVALID && !p);
  CHECK(plans > 0 && routed > 0);
  std::printf("zq dense host ok: %d plans, %d routed\n", plans, routed);
  return 0;
}
