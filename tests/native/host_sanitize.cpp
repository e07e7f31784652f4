// tests/native/host_sanitize.cpp — drives the HOST side of liblolhip (plan construction, number
// theory, index tables, the protobuf codec, argument checking of the C ABI, the device-memory
// owners of devmem.h and the host-only life of every handle kind) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU (sanitizers on the
// CPU build only; GPU ASan is not available on this pool).  Built and run by
// tests/test_sanitize.py with -fsanitize=address,undefined -fno-sanitize-recover.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

#include "lolhip.h"
#include "she_host.h"

#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static std::vector<lolhip_pp> factor(long m) {
  std::vector<lolhip_pp> v;
  for (long p = 2; m > 1; ++p) { int e = 0; while (m % p == 0) { m /= p; ++e; } if (e) v.push_back(lolhip_pp{(int16_t)p, (int16_t)e}); }
  return v;
}

int main() {
  std::mt19937_64 rng(1);
  // ---- plans (host only), tables, extensions ----------------------------------------------
  const long ms[] = {1, 2, 8, 9, 12, 45, 64, 75, 1024, 1728, 15015, 14336, 89, 2 * 97};
  std::vector<lolhip_plan*> plans;
  for (long m : ms) {
    auto pps = factor(m);
    for (int T = 1; T <= 3; ++T) {
      std::vector<int64_t> qs;
      int64_t lower = (int64_t)1 << (10 + 17 * T);
      for (int t = 0; t < T; ++t) { lower = lolhip_good_q(m, lower); CHECK(lower > 1); qs.push_back(lower); }
      lolhip_plan* P = nullptr;
      CHECK(lolhip_plan_create(pps.data(), (int)pps.size(), qs.data(), T, 1, &P) == LOLHIP_OK && P);
      CHECK(lolhip_plan_m(P) == m && lolhip_plan_T(P) == T && lolhip_plan_has_crt(P) == 1);
      const int64_t n = lolhip_plan_n(P);
      for (int which = 0; which < 6; ++which)
        for (int k = -1; k <= (int)pps.size(); ++k) {
          const int64_t cnt = lolhip_plan_table(P, which, k, nullptr, 0);
          std::vector<int64_t> buf((size_t)cnt + 1);
          CHECK(lolhip_plan_table(P, which, k, buf.data(), cnt) == cnt);
          CHECK(lolhip_plan_table(P, which, k, buf.data(), cnt / 2) == cnt);      // short buffer: partial copy only
        }
      // compute entry points refuse to run without a device, whatever the arguments
      std::vector<int64_t> y((size_t)(n * T));
      CHECK(lolhip_crt_batch(P, nullptr, y.data(), 1) == LOLHIP_ERR_NO_DEVICE);
      CHECK(lolhip_polymul_batch(P, nullptr, y.data(), y.data(), y.data(), 1) == LOLHIP_ERR_NO_DEVICE);
      CHECK(lolhip_op_host(P, LOLHIP_OP_L, y.data(), nullptr, 1) == LOLHIP_ERR_NO_DEVICE);
      CHECK(lolhip_crtc_batch(P, nullptr, nullptr, 0) == LOLHIP_ERR_NO_DEVICE);
      for (int64_t base : {(int64_t)0, (int64_t)2, (int64_t)256, (int64_t)1 << 40}) {
        const int L = lolhip_decompose_len(P, base);
        CHECK(L >= T);
        std::vector<int64_t> g((size_t)L * T);
        CHECK(lolhip_gadget(P, base, g.data(), (int64_t)g.size()) == L);
        CHECK(lolhip_gadget(P, base, g.data(), (int64_t)g.size() - 1) == LOLHIP_ERR_INVALID);
      }
      CHECK(lolhip_decompose_len(P, 1) == LOLHIP_ERR_INVALID && lolhip_decompose_len(P, -7) == LOLHIP_ERR_INVALID);
      plans.push_back(P);
    }
  }
  {  // malformed plan requests
    lolhip_plan* P = nullptr;
    lolhip_pp bad1[] = {{4, 1}}, bad2[] = {{3, 1}, {2, 2}}, bad3[] = {{2, 0}};
    int64_t q = 97, q0 = 1, qbig = (int64_t)1 << 62;
    CHECK(lolhip_plan_create(bad1, 1, &q, 1, 1, &P) == LOLHIP_ERR_INVALID);
    CHECK(lolhip_plan_create(bad2, 2, &q, 1, 1, &P) == LOLHIP_ERR_INVALID);
    CHECK(lolhip_plan_create(bad3, 1, &q, 1, 1, &P) == LOLHIP_ERR_INVALID);
    lolhip_pp ok[] = {{2, 3}};
    CHECK(lolhip_plan_create(ok, 1, &q0, 1, 1, &P) == LOLHIP_ERR_MODULUS);
    CHECK(lolhip_plan_create(ok, 1, &qbig, 1, 1, &P) == LOLHIP_ERR_MODULUS);
    CHECK(lolhip_plan_create(ok, 1, &q, 0, 1, &P) == LOLHIP_ERR_INVALID);
    int64_t wrong_root = 5;       // not of order 8 mod 97
    CHECK(lolhip_plan_create_roots(ok, 1, &q, 1, &wrong_root, nullptr, 1, &P) == LOLHIP_ERR_ROOT);
    int64_t q17 = 17;             // 8 | 16: fine; 45 does not divide 16: a plan without CRT basis is still a plan
    auto p45 = factor(45);
    CHECK(lolhip_plan_create(p45.data(), (int)p45.size(), &q17, 1, 1, &P) == LOLHIP_OK);
    CHECK(lolhip_plan_has_crt(P) == 0 && lolhip_plan_table(P, 0, 0, nullptr, 0) == 0);
    lolhip_plan_destroy(P);
    lolhip_plan_destroy(nullptr);
  }
  {  // ring extensions m | m'
    const long pairs[][2] = {{1, 8}, {4, 12}, {3, 21}, {8, 8}, {45, 45 * 7}, {128, 128 * 7 * 13}};
    for (auto& pr : pairs) {
      auto a = factor(pr[0]), b = factor(pr[1]);
      int64_t q = lolhip_good_q(pr[1], 1000);
      lolhip_plan *lo = nullptr, *hi = nullptr;
      CHECK(lolhip_plan_create(a.data(), (int)a.size(), &q, 1, 1, &lo) == LOLHIP_OK);
      CHECK(lolhip_plan_create(b.data(), (int)b.size(), &q, 1, 1, &hi) == LOLHIP_OK);
      lolhip_ext* X = nullptr;
      CHECK(lolhip_ext_create(lo, hi, &X) == LOLHIP_OK && X);
      for (int which = 0; which < 7; ++which) {
        const int64_t cnt = lolhip_ext_table(X, which, nullptr, 0);
        std::vector<int32_t> t((size_t)cnt + 1);
        CHECK(lolhip_ext_table(X, which, t.data(), cnt) == cnt);
      }
      lolhip_ext* Y = nullptr;
      if (pr[0] != pr[1]) CHECK(lolhip_ext_create(hi, lo, &Y) == LOLHIP_ERR_INVALID);     // m' does not divide m
      lolhip_ext_destroy(X);
      lolhip_plan_destroy(lo); lolhip_plan_destroy(hi);
    }
  }
  for (lolhip_plan* P : plans) lolhip_plan_destroy(P);

  // ---- the work-buffer arena (work.h): measuring and carving agree, over an array of len() words and a canary ----------
  for (int64_t B : {0, 1, 3, 8}) {
    for (int first_wins = 0; first_wins < 2; ++first_wins) {
      // a | f (doubles) | then either alt1, or alt2 | z (empty) | last
      struct Regions { int64_t *a; double* f; int64_t *alt1, *alt2, *z, *last; };
      const int64_t n1 = first_wins ? 11 * B : 5 * B;
      auto carve = [&](lolhip::Work& w) {
        Regions r;
        r.a = w.take(3 * B);
        r.f = w.take_f64(B);
        const int64_t m = w.mark();
        CHECK(m == 4 * B);
        r.alt1 = w.take(n1);
        w.rewind(m);
        r.alt2 = w.take(2 * B);
        r.z = w.take(0);
        r.last = w.take(7 * B);
        return r;
      };
      lolhip::Work dry(nullptr);
      const Regions none = carve(dry);
      const int64_t len = dry.len();
      CHECK(len == 4 * B + std::max<int64_t>(n1, 9 * B) && lolhip::measure(carve) == len);
      CHECK(!none.a && !none.f && !none.alt1 && !none.alt2 && !none.z && !none.last);
      std::vector<int64_t> buf((size_t)len + 1);                  // one spare word, so base is never null at B = 0
      int64_t* base = buf.data();
      buf[(size_t)len] = 0x5A;
      lolhip::Work w(base);
      const Regions r = carve(w);
      CHECK(w.len() == len);
      CHECK(r.a == base && (int64_t*)r.f == base + 3 * B && r.alt1 == base + 4 * B && r.alt2 == r.alt1);
      CHECK(r.z == r.alt2 + 2 * B && r.last == r.z);
      CHECK(first_wins ? r.alt1 + n1 == base + len : r.last + 7 * B == base + len);  // the longer alternative ends at len()
      for (int64_t i = 0; i < 3 * B; ++i) r.a[i] = i;             // every word of every region: an overrun traps
      for (int64_t i = 0; i < B; ++i) r.f[i] = 0.5;
      for (int64_t i = 0; i < n1; ++i) r.alt1[i] = i;
      for (int64_t i = 0; i < 2 * B; ++i) r.alt2[i] = i;
      for (int64_t i = 0; i < 7 * B; ++i) r.last[i] = i;
      CHECK(buf[(size_t)len] == 0x5A);
    }
  }
  {  // the shared layouts of she_host.h over real exts 4 | 12 and 4 | 20: the tunnel's regions fill lolhip_tunnel_work_len
    int64_t qs[2];
    qs[0] = lolhip_good_q(60, (int64_t)1 << 29);
    qs[1] = lolhip_good_q(60, qs[0] + 1);
    lolhip_plan* pl[3];
    const long idx[3] = {4, 12, 20};
    for (int i = 0; i < 3; ++i) {
      auto pps = factor(idx[i]);
      CHECK(lolhip_plan_create(pps.data(), (int)pps.size(), qs, 2, 1, &pl[i]) == LOLHIP_OK);
    }
    lolhip_ext *XR = nullptr, *XS = nullptr;
    CHECK(lolhip_ext_create(pl[0], pl[1], &XR) == LOLHIP_OK && lolhip_ext_create(pl[0], pl[2], &XS) == LOLHIP_OK);
    for (int64_t base : {(int64_t)0, (int64_t)2, (int64_t)256}) {
      const int64_t L = lolhip_decompose_len(pl[2], base), nS = lolhip_plan_n(pl[2]), nE = lolhip_plan_n(pl[0]);
      const int64_t rel = lolhip_plan_n(pl[1]) / nE;
      for (int64_t B : {0, 1, 3, 8}) {
        const int64_t len = lolhip_tunnel_work_len(XR, XS, base, B);
        CHECK(len == lolhip::measure(lolhip::tunnel_work, XR->X, XS->X, L, B));
        CHECK(len == rel * B * (nE + nS) * 2 + L * B * nS * 2 && (B > 0 || len == 0));
        std::vector<int64_t> buf((size_t)len + 1);
        lolhip::Work w(buf.data());
        const lolhip::TunnelWork t = lolhip::tunnel_work(w, XR->X, XS->X, L, B);
        CHECK(w.len() == len && t.ev.tmp_e == buf.data() && t.ev.tmp_s == t.ev.tmp_e + rel * B * nE * 2);
        CHECK(t.dig == t.ev.tmp_s + rel * B * nS * 2 && t.dig + L * B * nS * 2 == buf.data() + len);
        for (int64_t* p = t.ev.tmp_e; p < buf.data() + len; ++p) *p = 1;
        // evalLin alone carves the same first two regions
        lolhip::Work w2(buf.data());
        const lolhip::EvalLinWork ev = lolhip::evallin_work(w2, XR->X, XS->X, B);
        CHECK(ev.tmp_e == t.ev.tmp_e && ev.tmp_s == t.ev.tmp_s && buf.data() + w2.len() == t.dig);
      }
    }
    lolhip_ext_destroy(XR); lolhip_ext_destroy(XS);
    for (lolhip_plan* P : pl) lolhip_plan_destroy(P);
  }

  // ---- device-memory owners (devmem.h): the empty states, moves and the no-device answers ---------------------------------
  {
    using lolhip::DevBuf;
    static_assert(!std::is_copy_constructible_v<lolhip::Plan> && !std::is_copy_constructible_v<lolhip::ExtPlan>);
    static_assert(!std::is_copy_constructible_v<DevBuf<int64_t>> && !std::is_copy_assignable_v<DevBuf<int64_t>>);
    static_assert(sizeof(DevBuf<int64_t>) == sizeof(int64_t*));
    DevBuf<int64_t> a;
    CHECK(!a && a.get() == nullptr);
    DevBuf<int64_t> b(std::move(a));
    CHECK(!a && !b);
    a = std::move(b);                                              // onto an empty buffer
    DevBuf<int64_t>& self = a;
    a = std::move(self);                                           // onto itself
    CHECK(!a && !b);
    a.reset(); a.reset();
    CHECK(a.upload(std::vector<int64_t>()) == LOLHIP_OK && !a);
    CHECK(a.alloc(1) == LOLHIP_ERR_HIP && !a);                     // no device here
    CHECK(a.upload(std::vector<int64_t>(3, 7)) == LOLHIP_ERR_HIP && !a);
    std::vector<DevBuf<int64_t>> v(3);                             // as lolhip_pt_tunnel keeps them
    v.resize(40);
    CHECK(!v[39]);
  }
  {  // every handle kind: host-only create and destroy, and a create that fails after the struct is allocated
    auto plan = [](long m, std::vector<int64_t> qs) {
      auto pps = factor(m);
      lolhip_plan* P = nullptr;
      CHECK(lolhip_plan_create(pps.data(), (int)pps.size(), qs.data(), (int)qs.size(), 1, &P) == LOLHIP_OK && P);
      return P;
    };
    {  // plan: a device plan is refused here after its host tables are built
      auto pps = factor(12);
      int64_t q = lolhip_good_q(12, 1000);
      lolhip_plan* P = (lolhip_plan*)8;
      CHECK(lolhip_plan_create(pps.data(), (int)pps.size(), &q, 1, 0, &P) == LOLHIP_ERR_NO_DEVICE && !P);
    }
    // khprf, both families
    const int32_t tree[] = {3, 2, 1, 1, 1}, bad_tree[] = {3, 1, 1};
    {
      const int64_t q = lolhip_good_q(32, 200);
      lolhip_plan* P = plan(32, {q});
      std::vector<int64_t> z((size_t)(lolhip_decompose_len(P, 2) * lolhip_plan_n(P)), 1);
      lolhip_khprf *f = nullptr, *g = (lolhip_khprf*)8;
      CHECK(lolhip_khprf_create(P, 2, tree, 5, z.data(), z.data(), &f) == LOLHIP_OK && f);
      CHECK(lolhip_khprf_work_len(f, 0, 8) > 0);
      CHECK(lolhip_khprf_eval_batch(f, nullptr, 0, 8, z.data(), z.data()) == LOLHIP_ERR_NO_DEVICE);
      CHECK(lolhip_khprf_create(P, 2, bad_tree, 3, z.data(), z.data(), &g) == LOLHIP_ERR_INVALID);    // fails in parse
      CHECK(lolhip_khprf_create(P, 1, tree, 5, z.data(), z.data(), &g) == LOLHIP_ERR_INVALID);        // fails in make_decomp
      lolhip_khprf_destroy(f);
      lolhip_khprf_destroy(nullptr);
      lolhip_plan *Pq = plan(32, {8}), *PQ = plan(32, {lolhip_good_q(32, (int64_t)1 << 30)}), *Psmall = plan(32, {97});
      CHECK(lolhip_khprf_create_lifted(Pq, PQ, 2, tree, 5, z.data(), z.data(), &f) == LOLHIP_OK && f);
      CHECK(lolhip_khprf_work_len(f, 1, 5) > 0);
      CHECK(lolhip_khprf_create_lifted(Pq, Psmall, 2, tree, 5, z.data(), z.data(), &g) == LOLHIP_ERR_MODULUS);   // the bound
      CHECK(lolhip_khprf_create_lifted(P, PQ, 2, tree, 5, z.data(), z.data(), &g) == LOLHIP_ERR_MODULUS);        // q not 2^k
      lolhip_khprf_destroy(f);
      for (lolhip_plan* p : {P, Pq, PQ, Psmall}) lolhip_plan_destroy(p);
    }
    // ringmul
    {
      auto pps = factor(16);
      int64_t q = (int64_t)1 << 32, Qs[3];
      const int K = lolhip_ringmul_moduli(pps.data(), (int)pps.size(), &q, 1, Qs);
      CHECK(K == 2);
      lolhip_plan *Pq = plan(16, {q}), *PQ = plan(16, {Qs[0], Qs[1]}), *Pone = plan(16, {Qs[0]}), *P8 = plan(8, {Qs[0], Qs[1]});
      lolhip_ringmul *h = nullptr, *g = (lolhip_ringmul*)8;
      CHECK(lolhip_ringmul_create(Pq, PQ, &h) == LOLHIP_OK && h);
      CHECK(lolhip_ringmul_work_len(h, 3) > 0);
      CHECK(lolhip_ringmul_create(Pq, Pone, &g) == LOLHIP_ERR_MODULUS);       // one prime: the bound fails
      CHECK(lolhip_ringmul_create(Pq, P8, &g) == LOLHIP_ERR_INVALID);         // another index
      lolhip_ringmul_destroy(h);
      lolhip_ringmul_destroy(nullptr);
      for (lolhip_plan* p : {Pq, PQ, Pone, P8}) lolhip_plan_destroy(p);
    }
    // ptround: e = 3 over four moduli of index 16
    {
      int64_t qs[4];
      qs[0] = lolhip_good_q(16, (int64_t)1 << 29);
      for (int i = 1; i < 4; ++i) qs[i] = lolhip_good_q(16, qs[i - 1]);
      lolhip_plan *lvl[3], *up[2];
      for (int i = 0; i < 3; ++i) lvl[i] = plan(16, std::vector<int64_t>(qs + i + 1, qs + 4));
      for (int i = 0; i < 2; ++i) up[i] = plan(16, std::vector<int64_t>(qs + i, qs + 4));
      lolhip_plan* pp = plan(16, {8});
      const int64_t word = 0;
      const int64_t* hints[2] = {&word, &word};                   // create keeps the addresses and reads nothing
      lolhip_ptround *c = nullptr, *g = (lolhip_ptround*)8;
      CHECK(lolhip_ptround_create(3, 8, lvl, up, hints, 0, pp, nullptr, nullptr, &c) == LOLHIP_OK && c);
      CHECK(lolhip_ptround_work_len(c, 2) > 0);
      CHECK(lolhip_ptround_create(3, 16, lvl, up, hints, 0, pp, nullptr, nullptr, &g) == LOLHIP_ERR_INVALID && !g);   // pp is over 8
      lolhip_plan* up_bad[2] = {up[0], lvl[1]};
      g = (lolhip_ptround*)8;
      CHECK(lolhip_ptround_create(3, 8, lvl, up_bad, hints, 0, pp, nullptr, nullptr, &g) == LOLHIP_ERR_INVALID && !g);  // fails at level 1
      lolhip_ptround_destroy(c);
      lolhip_ptround_destroy(nullptr);
      for (lolhip_plan* p : lvl) lolhip_plan_destroy(p);
      for (lolhip_plan* p : up) lolhip_plan_destroy(p);
      lolhip_plan_destroy(pp);
    }
    // tunnel chain (no hop, and one hop 4 | 12 -> 4 | 20) and pt_tunnel (the same hop over one prime)
    {
      int64_t qs[2];
      qs[0] = lolhip_good_q(60, (int64_t)1 << 29);
      qs[1] = lolhip_good_q(60, qs[0]);
      lolhip_plan *E = plan(4, {qs[0], qs[1]}), *R = plan(12, {qs[0], qs[1]}), *S = plan(20, {qs[0], qs[1]}), *S1 = plan(20, {qs[1]});
      lolhip_ext *XR = nullptr, *XS = nullptr;
      CHECK(lolhip_ext_create(E, R, &XR) == LOLHIP_OK && lolhip_ext_create(E, S, &XS) == LOLHIP_OK);
      const int64_t word = 0;
      const int64_t* dev[1] = {&word};
      lolhip_tunnel_chain *c = nullptr, *g = (lolhip_tunnel_chain*)8;
      CHECK(lolhip_tunnel_chain_create(0, nullptr, nullptr, nullptr, nullptr, 0, S, S1, &c) == LOLHIP_OK && c);
      lolhip_tunnel_chain_destroy(c);
      CHECK(lolhip_tunnel_chain_create(1, &XR, &XS, dev, dev, 0, R, S1, &c) == LOLHIP_OK && c);
      CHECK(lolhip_tunnel_chain_work_len(c, 2) > 0);
      CHECK(lolhip_tunnel_chain_create(1, &XR, &XS, dev, dev, 0, S, S1, &g) == LOLHIP_ERR_INVALID && !g);   // p_in is not of R's index: fails last
      lolhip_tunnel_chain_destroy(c);
      lolhip_tunnel_chain_destroy(nullptr);
      lolhip_ext_destroy(XR); lolhip_ext_destroy(XS);
      for (lolhip_plan* p : {E, R, S, S1}) lolhip_plan_destroy(p);
    }
    {
      auto pr = factor(12), ps = factor(20);
      const int64_t bound = lolhip_pt_tunnel_modulus(pr.data(), (int)pr.size(), ps.data(), (int)ps.size(), 2, 1, 2, 3);
      CHECK(bound > 0);
      const int64_t Q = lolhip_good_q(60, bound), Qsmall = lolhip_good_q(60, 8);
      CHECK(Qsmall <= bound);
      std::vector<int64_t> f((size_t)(2 * 8), 1);                   // [rel = n_R / n_E][n_S]
      const int64_t* funcs[1] = {f.data()};
      for (int64_t q : {Q, Qsmall}) {
        lolhip_plan *E = plan(4, {q}), *R = plan(12, {q}), *S = plan(20, {q});
        lolhip_ext *XR = nullptr, *XS = nullptr;
        CHECK(lolhip_ext_create(E, R, &XR) == LOLHIP_OK && lolhip_ext_create(E, S, &XS) == LOLHIP_OK);
        lolhip_pt_tunnel* t = (lolhip_pt_tunnel*)8;
        if (q == Q) {
          CHECK(lolhip_pt_tunnel_create(1, &XR, &XS, funcs, 2, 3, &t) == LOLHIP_OK && t);
          CHECK(lolhip_pt_tunnel_work_len(t, 2) > 0);
          CHECK(lolhip_pt_tunnel_batch(t, nullptr, f.data(), f.data(), f.data(), 1) == LOLHIP_ERR_NO_DEVICE);
          lolhip_pt_tunnel_destroy(t);
        } else {
          CHECK(lolhip_pt_tunnel_create(1, &XR, &XS, funcs, 2, 3, &t) == LOLHIP_ERR_MODULUS && !t);   // below the hop's bound
        }
        lolhip_ext_destroy(XR); lolhip_ext_destroy(XS);
        for (lolhip_plan* p : {E, R, S}) lolhip_plan_destroy(p);
      }
      lolhip_pt_tunnel_destroy(nullptr);
    }
  }

  // ---- wire format: round trips, every truncation, random mutations ----------------------------
  const int64_t qs[] = {97, ((int64_t)1 << 40) + 15, 12289};
  const int T = 3, n = 24, L = 3, K = 2;
  std::vector<int64_t> xs((size_t)L * K * n * T);
  for (size_t i = 0; i < xs.size(); ++i) xs[i] = (int64_t)(rng() % (uint64_t)qs[i % T]) - (i % 5 == 0 ? qs[i % T] / 2 : 0);
  const int64_t len1 = lolhip_rqproduct_write(12, qs, T, xs.data(), n, nullptr, 0);
  CHECK(len1 > 0);
  std::vector<uint8_t> rq((size_t)len1);
  CHECK(lolhip_rqproduct_write(12, qs, T, xs.data(), n, rq.data(), len1) == len1);
  CHECK(lolhip_rqproduct_write(12, qs, T, xs.data(), n, rq.data(), len1 - 1) == LOLHIP_ERR_INVALID);
  const int64_t len2 = lolhip_kshint_write(12, qs, T, L, K, xs.data(), n, 1, 2, nullptr, 0);
  std::vector<uint8_t> ks((size_t)len2);
  CHECK(lolhip_kshint_write(12, qs, T, L, K, xs.data(), n, 1, 2, ks.data(), len2) == len2);
  auto read_all = [&](const uint8_t* b, int64_t l) {
    uint32_t m, e, r, s; int Tt, Ll, Kk, C; int64_t q[8]; uint64_t p; double v;
    std::vector<int64_t> out((size_t)L * K * n * T);
    std::vector<double> outd((size_t)n * T);
    int64_t fo, fl, ho[4], hl[4];
    (void)lolhip_rqproduct_read(b, l, &m, q, 8, &Tt, out.data(), (int64_t)out.size());
    (void)lolhip_rqproduct_read(b, l, &m, q, 1, &Tt, out.data(), 3);
    (void)lolhip_kshint_read(b, l, &m, q, 8, &Tt, &Ll, &Kk, out.data(), (int64_t)out.size());
    (void)lolhip_kshint_read(b, l, &m, q, 8, &Tt, &Ll, &Kk, nullptr, 0);
    (void)lolhip_r_read(b, l, &m, out.data(), (int64_t)out.size());
    (void)lolhip_secretkey_read(b, l, &m, &v, out.data(), 2);
    (void)lolhip_kqproduct_read(b, l, &m, q, 8, &Tt, outd.data(), (int64_t)outd.size());
    (void)lolhip_linearrq_read(b, l, &e, &r, &C, &m, q, 8, &Tt, out.data(), (int64_t)out.size());
    (void)lolhip_tunnelhint_read(b, l, &e, &r, &s, &p, &fo, &fl, ho, hl, 4);
    (void)lolhip_chain_read(b, l, ho, hl, 4);
    (void)lolhip_chain_read(b, l, nullptr, nullptr, 0);
  };
  {
    uint32_t m; int Tt, Ll, Kk; int64_t q[8];
    std::vector<int64_t> back(xs.size());
    CHECK(lolhip_kshint_read(ks.data(), len2, &m, q, 8, &Tt, &Ll, &Kk, back.data(), (int64_t)back.size()) == n);
    CHECK(m == 12 && Tt == T && Ll == L && Kk == K);
    for (size_t i = 0; i < xs.size(); ++i) { int64_t w = xs[i] % qs[i % T]; if (w < 0) w += qs[i % T]; CHECK(back[i] == w); }
  }
  // round 3 writers: LinearRq, TunnelHint, a chain of them, R, SecretKey — size query = bytes written, short buffers refused
  const int64_t len3 = lolhip_linearrq_write(4, 12, 12, qs, T, K, xs.data(), n, nullptr, 0);
  std::vector<uint8_t> lin((size_t)len3);
  CHECK(len3 > 0 && lolhip_linearrq_write(4, 12, 12, qs, T, K, xs.data(), n, lin.data(), len3) == len3);
  CHECK(lolhip_linearrq_write(4, 12, 12, qs, T, K, xs.data(), n, lin.data(), len3 - 1) == LOLHIP_ERR_INVALID);
  const uint8_t* hp[2] = {ks.data(), ks.data()};
  const int64_t hl2[2] = {len2, len2};
  const int64_t len4 = lolhip_tunnelhint_write(lin.data(), len3, hp, hl2, 2, 4, 12, 12, 257, nullptr, 0);
  std::vector<uint8_t> th((size_t)len4);
  CHECK(len4 > 0 && lolhip_tunnelhint_write(lin.data(), len3, hp, hl2, 2, 4, 12, 12, 257, th.data(), len4) == len4);
  {
    uint32_t e, r, s2; uint64_t p; int64_t fo, fl, ho[4], hl[4];
    CHECK(lolhip_tunnelhint_read(th.data(), len4, &e, &r, &s2, &p, &fo, &fl, ho, hl, 4) == 2);
    CHECK(e == 4 && r == 12 && s2 == 12 && p == 257 && fl == len3 && hl[0] == len2 && hl[1] == len2);
  }
  const uint8_t* cp[3] = {th.data(), th.data(), th.data()};
  const int64_t cl[3] = {len4, len4, len4};
  const int64_t len5 = lolhip_chain_write(cp, cl, 3, nullptr, 0);
  std::vector<uint8_t> chain((size_t)len5);
  CHECK(len5 > 0 && lolhip_chain_write(cp, cl, 3, chain.data(), len5) == len5);
  { int64_t off[4], ln[4]; CHECK(lolhip_chain_read(chain.data(), len5, off, ln, 4) == 3 && ln[2] == len4); }
  const int64_t rv[5] = {-3, 0, 7, ((int64_t)1 << 50), -((int64_t)1 << 50)};
  const int64_t len6 = lolhip_secretkey_write(12, 0.5, rv, 5, nullptr, 0);
  std::vector<uint8_t> skb((size_t)len6);
  CHECK(len6 > 0 && lolhip_secretkey_write(12, 0.5, rv, 5, skb.data(), len6) == len6);
  { uint32_t m; double v; int64_t back[5]; CHECK(lolhip_secretkey_read(skb.data(), len6, &m, &v, back, 5) == 5 && m == 12 && v == 0.5 && back[4] == rv[4]); }
  for (const std::vector<uint8_t>* src : {&rq, &ks, &chain, &skb}) {
    for (int64_t l = 0; l <= (int64_t)src->size(); ++l) {          // every truncation, exact-size heap copy: overreads trap
      std::vector<uint8_t> cut(src->begin(), src->begin() + l);
      read_all(cut.data(), l);
    }
    for (int it = 0; it < 2500; ++it) {                             // random byte mutations
      std::vector<uint8_t> mut(*src);
      const int flips = 1 + (int)(rng() % 3);
      for (int f = 0; f < flips; ++f) mut[rng() % mut.size()] = (uint8_t)rng();
      read_all(mut.data(), (int64_t)mut.size());
    }
  }
  std::printf("host sanitize ok\n");
  return 0;
}
