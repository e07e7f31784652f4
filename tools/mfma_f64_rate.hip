// tools/mfma_f64_rate.hip — how fast one SIMD issues v_mfma_f64_16x16x4_f64 (tools/bench_pipelines.py --cplx-dense builds
// and runs it).  Every wave runs ITERS rounds of CHAINS MFMAs: CHAINS = 1 is one dependent chain (each MFMA waits for the
// one before it: the latency), CHAINS = 4 four independent accumulators (back-to-back issue).  One wave per SIMD (256
// threads per block, one block per CU) and, for the occupancy the dense kernel runs at, two.  Timed with HIP events over
// the whole grid; cycles are at the clock the device reports, so they are an upper bound when the clock drops under load.
//
//   hipcc --offload-arch=gfx950 -O3 -o mfma_f64_rate mfma_f64_rate.hip && ./mfma_f64_rate
#include <hip/hip_runtime.h>

#include <cstdio>

typedef double d4 __attribute__((ext_vector_type(4)));

template <int CHAINS>
__global__ void __launch_bounds__(256) k_rate(double* out, int iters, double a, double b) {
  d4 acc[CHAINS];
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
  if (s == 12345.678) out[0] = s;          // never true for a = b = 0: keeps the loop alive without a store per thread
}

template <int CHAINS>
static int run(const char* label, int blocks_per_cu, int cus, double mhz, double* d_out) {
  const int iters = 20000;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
  const dim3 grid((unsigned)(cus * blocks_per_cu)), block(256);
  hipLaunchKernelGGL(k_rate<CHAINS>, grid, block, 0, 0, d_out, 100, 0.0, 0.0);      // warm-up
  float best = 1e30f;
  for (int r = 0; r < 5; ++r) {
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(k_rate<CHAINS>, grid, block, 0, 0, d_out, iters, 0.0, 0.0);
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess) return 1;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  // per SIMD: blocks_per_cu waves, each iters * CHAINS MFMAs
  const double per_simd = (double)iters * CHAINS * blocks_per_cu;
  const double ns = best * 1e6 / per_simd;
  printf("{\"op\": \"mfma_f64_16x16x4\", \"case\": \"%s\", \"waves_per_simd\": %d, \"chains\": %d, \"ms\": %.4f, \"ns_per_mfma_per_simd\": %.3f, "
         "\"cycles_at_reported_clock\": %.2f, \"clock_mhz\": %.0f, \"gmacs_per_s\": %.1f}\n",
         label, blocks_per_cu, CHAINS, best, ns, ns * mhz * 1e-3, mhz, 1024.0 * per_simd * 4 * cus / best / 1e6);
  return 0;
}

int main() {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
  const int cus = prop.multiProcessorCount;
  const double mhz = prop.clockRate / 1000.0;
  double* d_out = nullptr;
  if (hipMalloc(&d_out, 64) != hipSuccess) return 1;
  int rc = run<1>("dependent", 1, cus, mhz, d_out);
  if (!rc) rc = run<4>("independent", 1, cus, mhz, d_out);
  if (!rc) rc = run<4>("independent", 2, cus, mhz, d_out);
  (void)hipFree(d_out);
  return rc;
}
