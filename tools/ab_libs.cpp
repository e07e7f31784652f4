// tools/ab_libs.cpp — same-process A/B of the fused poly-mul between two builds of liblolhip.so (tools/ab_build.sh):
//   ab_libs <name A> <lib A> <name B> <lib B> [alternations = 7] [log2 m = 14] [B = 4096] [launches = 20] [untimed = 5]
// Both libraries are dlopen'ed side by side (RTLD_LOCAL), each builds its own plan for the benchmark's modulus (the
// first NTT-friendly prime above 2^60), and both work on the same operands.  1 s of clock warm-up, then per
// alternation and arm: <untimed> launches, then one HIP-event pair around <launches> launches; the arm order flips
// every alternation.  The outputs of the two arms are compared bit for bit.  Prints every sample (ms per launch).
// Under rocprofv3 --kernel-trace --stats the same run gives per-dispatch durations (the arms' kernels carry the same
// name: tell them apart by order — see the printed schedule).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <random>
#include <vector>
#include "../include/lolhip.h"
#define CK(x) do { if ((x) != hipSuccess) { printf("hip error line %d\n", __LINE__); return 1; } } while (0)

struct Arm {
  const char* name; void* h; lolhip_plan* plan;
  decltype(&lolhip_polymul_batch) polymul;
  std::vector<double> ms;
};

int main(int argc, char** argv) {
  if (argc < 5) { printf("usage: ab_libs <name A> <lib A> <name B> <lib B> [alternations] [log2 m] [B] [launches] [untimed]\n"); return 2; }
  const int alts = argc > 5 ? atoi(argv[5]) : 7, lm = argc > 6 ? atoi(argv[6]) : 14;
  const long B = argc > 7 ? atol(argv[7]) : 4096;
  const int launches = argc > 8 ? atoi(argv[8]) : 20, untimed = argc > 9 ? atoi(argv[9]) : 5;
  Arm arm[2] = {{argv[1]}, {argv[3]}};
  int64_t q = 0;
  for (int i = 0; i < 2; i++) {
    Arm& a = arm[i];
    a.h = dlopen(argv[2 + 2 * i], RTLD_NOW | RTLD_LOCAL);
    if (!a.h) { printf("dlopen %s: %s\n", argv[2 + 2 * i], dlerror()); return 1; }
    auto good_q = (decltype(&lolhip_good_q))dlsym(a.h, "lolhip_good_q");
    auto create = (decltype(&lolhip_plan_create))dlsym(a.h, "lolhip_plan_create");
    a.polymul = (decltype(&lolhip_polymul_batch))dlsym(a.h, "lolhip_polymul_batch");
    if (!good_q || !create || !a.polymul) { printf("missing symbol in %s\n", argv[2 + 2 * i]); return 1; }
    q = good_q((int64_t)1 << lm, (int64_t)1 << 60);
    lolhip_pp pp{2, (int16_t)lm};
    const int rc = create(&pp, 1, &q, 1, 0, &a.plan);
    if (rc) { printf("plan rc=%d (%s)\n", rc, a.name); return 1; }
  }
  const size_t cnt = (size_t)B << (lm - 1);
  std::vector<int64_t> ha(cnt), hb(cnt);
  std::mt19937_64 rng(5);
  for (size_t i = 0; i < cnt; i++) { ha[i] = (int64_t)(rng() % (uint64_t)q); hb[i] = (int64_t)(rng() % (uint64_t)q); }
  int64_t *da, *db, *dc[2];
  CK(hipMalloc(&da, cnt * 8)); CK(hipMalloc(&db, cnt * 8)); CK(hipMalloc(&dc[0], cnt * 8)); CK(hipMalloc(&dc[1], cnt * 8));
  CK(hipMemcpy(da, ha.data(), cnt * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(db, hb.data(), cnt * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("# m=2^%d q=%lld B=%ld: %d alternations, %d launches per sample after %d untimed; ms per launch\n", lm, (long long)q, B, alts, launches, untimed);
  // clock warm-up: 1 s of back-to-back launches, both arms
  const auto t0 = std::chrono::steady_clock::now();
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 1.0) {
    for (int i = 0; i < 2; i++) for (int k = 0; k < 10; k++) if (arm[i].polymul(arm[i].plan, 0, dc[i], da, db, B)) { printf("launch failed\n"); return 1; }
    CK(hipDeviceSynchronize());
  }
  for (int alt = 0; alt < alts; alt++) {
    for (int s = 0; s < 2; s++) {
      const int i = (alt & 1) ? 1 - s : s;
      Arm& a = arm[i];
      for (int k = 0; k < untimed; k++) a.polymul(a.plan, 0, dc[i], da, db, B);
      CK(hipEventRecord(e0, 0));
      for (int k = 0; k < launches; k++) a.polymul(a.plan, 0, dc[i], da, db, B);
      CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      a.ms.push_back(ms / launches);
      printf("alternation %d  %-10s %.4f\n", alt + 1, a.name, ms / launches);
    }
  }
  std::vector<int64_t> h0(cnt), h1(cnt);
  CK(hipMemcpy(h0.data(), dc[0], cnt * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(h1.data(), dc[1], cnt * 8, hipMemcpyDeviceToHost));
  const bool equal = !memcmp(h0.data(), h1.data(), cnt * 8);
  double med[2], lo[2], hi[2];
  for (int i = 0; i < 2; i++) {
    std::vector<double> v = arm[i].ms; std::sort(v.begin(), v.end());
    lo[i] = v.front(); hi[i] = v.back(); med[i] = v[v.size() / 2];
    printf("  %-10s", arm[i].name); for (double x : arm[i].ms) printf(" %.4f", x);
    printf("   min %.4f  median %.4f  max %.4f\n", lo[i], med[i], hi[i]);
  }
  const bool disjoint = hi[0] < lo[1] || hi[1] < lo[0];
  printf("  speedup of %s over %s (medians) %.3f, ranges %s, outputs %s\n", arm[1].name, arm[0].name, med[0] / med[1],
         disjoint ? "do not overlap" : "OVERLAP", equal ? "equal" : "DIFFER");
  return equal ? 0 : 3;
}
