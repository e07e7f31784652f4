// tests/native/zq_scan_host.cpp — the host side of the scan route of the prime ops (LOLHIP_ROUTE_SCAN_ZQ) under
// AddressSanitizer and UBSan: a stand-alone program over the product's host sources and device_stubs.cpp
// (tests/test_zq_scan_sanitize.py builds and runs it).  Plans are host-only: both creators over a grid of indices x
// moduli x flag and route words, lolhip_plan_scan_route for every op and out-of-range op across the two switches, null
// arguments, and the six compute entries, which answer LOLHIP_ERR_NO_DEVICE.
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

// the answer for each of the six ops, which must agree, and 0 for every op outside them
static int scan_route(const lolhip_plan* p) {
  const int r = lolhip_plan_scan_route(p, LOLHIP_OP_L);
  CHECK(r == 0 || r == 1);
  for (int op = LOLHIP_OP_L; op <= LOLHIP_OP_DIVGDEC; ++op) CHECK(lolhip_plan_scan_route(p, op) == r);
  for (int op : {-1000, -1, 0, 1, 2, 3, 10, 11, 12, 1 << 30}) CHECK(lolhip_plan_scan_route(p, op) == 0);
  return r;
}

int main() {
  const int64_t indices[] = {17, 34, 136, 221, 289, 323, 257, 45, 91, 64, 17 * 2048};
  // per index: moduli = 1 (mod m) found by search from these lower bounds; 0 marks "no CRT basis" (q = 2^11), -1 q = 2
  const int64_t lowers[] = {1000, (int64_t)1 << 58, 0, -1};
  int plans = 0, routed = 0;
  for (int64_t m : indices) {
    const std::vector<lolhip_pp> pps = factor(m);
    bool large = false, odd = false;
    for (const lolhip_pp& pp : pps) { large = large || pp.prime > 13; odd = odd || pp.prime != 2; }
    for (int64_t lo : lowers)
      for (int T = 1; T <= 2; ++T) {
        int64_t qs[2];
        qs[0] = lo > 0 ? lolhip_good_q(m, lo) : lo == 0 ? 2048 : 2;
        qs[1] = lo > 0 ? lolhip_good_q(m, qs[0]) : 16;
        CHECK(qs[0] >= 2 && qs[1] >= 2);
        for (uint32_t flags : {0u, 1u, 2u, 3u, 4u})
          for (uint32_t routes : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 8u, 0x80000004u}) {
            lolhip_plan* p = nullptr;
            // the older creator refuses the bit, as it refuses LOLHIP_PLAN_DENSE_CPLX
            const int rc_old = lolhip_plan_create_routes(pps.data(), (int)pps.size(), qs, T, 1, flags, routes, &p);
            if (flags > 1 || routes > 1) CHECK(rc_old == LOLHIP_ERR_INVALID && !p);
            else { CHECK(rc_old == LOLHIP_OK && p && scan_route(p) == 0); lolhip_plan_destroy(p); p = nullptr; }
            lolhip_plan_opts opts = {(uint32_t)sizeof(lolhip_plan_opts), flags, routes};
            const int rc = lolhip_plan_create_opts(pps.data(), (int)pps.size(), qs, T, 1, &opts, &p);
            if (flags > 3 || (routes & ~5u)) { CHECK(rc == LOLHIP_ERR_INVALID && !p); continue; }
            CHECK(rc == LOLHIP_OK && p);
            ++plans;
            const bool opted = (routes & LOLHIP_ROUTE_SCAN_ZQ) != 0, fits = lolhip_plan_n(p) <= 8192;
            const int r = scan_route(p);
            CHECK(r == (opted && fits && large ? 1 : 0));
            routed += r;
            CHECK(lolhip_debug_set("ZQ_SCAN", 1) == LOLHIP_OK);
            CHECK(scan_route(p) == (opted && fits && odd ? 1 : 0));
            CHECK(lolhip_debug_set("GENERIC_SCALAR", 1) == LOLHIP_OK);
            CHECK(scan_route(p) == 0);
            CHECK(lolhip_debug_set("ZQ_SCAN", 0) == LOLHIP_OK);
            CHECK(scan_route(p) == 0);
            CHECK(lolhip_debug_set("GENERIC_SCALAR", 0) == LOLHIP_OK);
            CHECK(scan_route(p) == r);
            // the sibling route is what it was
            if (!(routes & LOLHIP_ROUTE_DENSE_ZQ)) CHECK(lolhip_plan_zq_route(p, 0) == 0);
            // host-only: every compute entry says so before it looks at its pointers
            int64_t y[4] = {0, 0, 0, 0};
            CHECK(lolhip_l_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_linv_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_mulgpow_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_mulgdec_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_divgpow_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            CHECK(lolhip_divgdec_batch(p, nullptr, y, 1) == LOLHIP_ERR_NO_DEVICE);
            lolhip_plan_destroy(p);
          }
      }
  }
  CHECK(lolhip_plan_scan_route(nullptr, LOLHIP_OP_L) == 0 && lolhip_plan_scan_route(nullptr, -1) == 0);
  CHECK(lolhip_debug_set("ZQ_SCAN", 1) == LOLHIP_OK && lolhip_plan_scan_route(nullptr, LOLHIP_OP_L) == 0);
  CHECK(lolhip_debug_set("ZQ_SCAN", 0) == LOLHIP_OK);
  lolhip_plan* p = nullptr;
  lolhip_plan_opts opts = {(uint32_t)sizeof(lolhip_plan_opts), 0, LOLHIP_ROUTE_SCAN_ZQ};
  CHECK(lolhip_plan_create_opts(nullptr, 0, nullptr, 1, 1, &opts, &p) == LOLHIP_ERR_INVALID && !p);
  const std::vector<lolhip_pp> pps = factor(17);
  int64_t q = 103;
  CHECK(lolhip_plan_create_opts(pps.data(), 1, &q, 1, 1, nullptr, &p) == LOLHIP_ERR_INVALID && !p);
  opts.size = 8;
  CHECK(lolhip_plan_create_opts(pps.data(), 1, &q, 1, 1, &opts, &p) == LOLHIP_ERR_INVALID && !p);
  CHECK(plans > 0 && routed > 0);
  std::printf("zq scan host ok: %d plans, %d routed\n", plans, routed);
  return 0;
}
