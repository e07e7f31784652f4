// tools/microbench_csub.hip — the 64-bit class's lazy-range trim (x >= m ? x - m : x, wave-uniform m) as a select
// (csubn, zq_dev.h) against the EXEC-predicated forms (csubx): checked for exactness against plain C, then timed
// (ns per wave-op per SIMD at 1, 4 and 8 launched waves per SIMD).  Development tool; DESIGN.md 3.1e,
// profiles/r05_microbench_csub.txt.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++20 -I../include -I../lol_amd/csrc -o microbench_csub microbench_csub.hip
#include "pow2_impl.h"

#include <stdio.h>
#include <algorithm>
#include <random>
#include <vector>
using namespace lolhip;
typedef unsigned __int128 u128;
constexpr int ITER = 4096, CH = 8;

// ---- trim variants -------------------------------------------------------------------------------------------------
// the four-instruction block and the hoisted-save form WITHOUT the tail padding csubx() carries
__device__ __forceinline__ u64 csubx_raw(u64 x, u64 m, u64 negm) {
  u64 sv;
  asm(LH_CSUBX("x", "sv", "m", "nm") : [x] "+v"(x), [sv] "=&s"(sv) : [m] "s"(m), [nm] "s"(negm) : "vcc");
  return x;
}
__device__ __forceinline__ u64 csubx_saved_raw(u64 x, u64 m, u64 negm, u64 saved) {
  asm(LH_CSUBX_SAVED("x", "sv", "m", "nm") : [x] "+v"(x) : [sv] "s"(saved), [m] "s"(m), [nm] "s"(negm) : "vcc");
  return x;
}
__device__ __forceinline__ u64 csubx2_raw(u64 x, u64 m1, u64 negm1, u64 m2, u64 negm2) {
  u64 sv;
  asm(LH_CSUBX("x", "sv", "m1", "nm1") "\n\t" LH_CSUBX_SAVED("x", "sv", "m2", "nm2")
      : [x] "+v"(x), [sv] "=&s"(sv) : [m1] "s"(m1), [nm1] "s"(negm1), [m2] "s"(m2), [nm2] "s"(negm2) : "vcc");
  return x;
}
enum { T_NONE, T_SEL, T_X, T_XRAW, T_XSAVED, T_XSAVEDRAW, T_SEL2, T_X2, T_X2RAW, T_COUNT };
constexpr bool is_double(int V) { return V == T_SEL2 || V == T_X2 || V == T_X2RAW; }
// single trims: m = 4q; double trims: 4q then 2q
template <int V>
__device__ __forceinline__ u64 trim(u64 x, const QK& k, u64 sv) {
  if constexpr (V == T_SEL) return csubn(x, k.nq4);
  else if constexpr (V == T_X) return csubx(x, k.q4, k.nq4);
  else if constexpr (V == T_XRAW) return csubx_raw(x, k.q4, k.nq4);
  else if constexpr (V == T_XSAVED) return csubx(x, k.q4, k.nq4, sv);
  else if constexpr (V == T_XSAVEDRAW) return csubx_saved_raw(x, k.q4, k.nq4, sv);
  else if constexpr (V == T_SEL2) return csubn(csubn(x, k.nq4), k.nq2);
  else if constexpr (V == T_X2) return csubx2(x, k.q4, k.nq4, k.q2, k.nq2);
  else if constexpr (V == T_X2RAW) return csubx2_raw(x, k.q4, k.nq4, k.q2, k.nq2);
  else return x;
}
// plain C
__host__ __device__ static u64 ref_trim(u64 x, u64 m) { return x >= m ? x - m : x; }

// partial = 0: every lane takes the variant; 1: only the odd lanes do (a divergent branch: the block starts from, and
// has to put back, a partial EXEC), the even ones plain C
template <int V>
__global__ void k_chk_trim(u64* x, u64 q, int partial) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // the grid covers the array exactly
  const QK k(q, std::true_type{});
  u64 v = x[i];
  if (!partial || (i & 1)) {
    const u64 sv = exec_save();
    v = trim<V>(v, k, sv);
  } else {
    v = ref_trim(v, k.q4);
    if (is_double(V)) v = ref_trim(v, k.q2);
  }
  x[i] = v;
}
// CH independent chains per lane: x <- trim(x + inc), inc per lane and chain, so lanes of one wave decide differently
template <int V>
__global__ void __launch_bounds__(256) k_thr_trim(u64* out, u64 q) {
  const QK k(q, std::true_type{});
  const u64 span = is_double(V) ? 6 * q : 4 * q;            // x in [0,2q) + [0,6q), or [0,4q) + [0,4q): always < 8q
  u64 y[CH], inc[CH];
  for (int i = 0; i < CH; i++) {
    y[i] = (((threadIdx.x + i + 1) * 0x9E3779B97F4A7C15ull) >> 4) % q;
    inc[i] = (((threadIdx.x * 8 + i + 3) * 0xD1B54A32D192ED03ull) >> 3) % span;
  }
  for (int it = 0; it < ITER; ++it) {
    u64 sv = 0;
    if constexpr (V == T_XSAVED || V == T_XSAVEDRAW) sv = exec_save();     // one save per CH = 8 trims
#pragma unroll
    for (int i = 0; i < CH; i++) {
      asm volatile("" : "+v"(inc[i]));
      y[i] = trim<V>(y[i] + inc[i], k, sv);
    }
  }
  u64 acc = 0; for (int i = 0; i < CH; i++) acc += y[i];
  out[blockIdx.x * 256 + threadIdx.x] = acc;
}

// ---- whole butterflies ---------------------------------------------------------------------------------------------
// 0: the select form (the code before LOLHIP_CSUB_EXEC); 1: the trim inside the product's first asm statement;
// 2: bfly_fwd<1> / bfly_inv<1> as this build of pow2_impl.h compiles them; 3: csubx as a block of its own
template <int V, bool INV>
__device__ __forceinline__ void bfly(u64& X, u64& Y, u64 w, u64 wp, const QK& k) {
  if constexpr (V == 2) {
    if constexpr (INV) bfly_inv<1>(X, Y, w, wp, k); else bfly_fwd<1>(X, Y, w, wp, k);
  } else if constexpr (!INV) {
    u64 x = X, xn;
    if constexpr (V == 0) { x = csubn(X, k.nq4); xn = shoup_acc<false>(Y, w, wp, k.nq, x); }
    else if constexpr (V == 3) { x = csubx(X, k.q4, k.nq4); xn = shoup_acc<false>(Y, w, wp, k.nq, x); }
    else xn = shoup_acc_csubx<false, true>(Y, w, wp, k.nq, x, k.q4, k.nq4);
    const u64 z = shl1_add64u(x, k.q4);
    X = xn;
    Y = z - xn;
  } else {
    const u64 s = add64(X, Y);
    const u64 d = add64u(X, k.q4) - Y;
    if constexpr (V == 0) { X = csubn(s, k.nq4); Y = shoup_acc<false>(d, w, wp, k.nq, 0); }
    else if constexpr (V == 3) { X = csubx(s, k.q4, k.nq4); Y = shoup_acc<false>(d, w, wp, k.nq, 0); }
    else { X = s; Y = shoup_acc_csubx<false, false>(d, w, wp, k.nq, X, k.q4, k.nq4); }
  }
}
template <int V, bool INV>
__global__ void __launch_bounds__(256) k_thr_bfly(u64* out, const u64* tw, u64 q) {
  const QK k(q, std::true_type{});
  u64 y[CH];
  for (int i = 0; i < CH; i++) y[i] = (((threadIdx.x + i + 1) * 0x9E3779B97F4A7C15ull) >> 4) % q;
  const u64* t = tw + 2 * (threadIdx.x & 63);
  u64 w = t[0], wp = t[1];
  for (int it = 0; it < ITER; ++it) {
    asm volatile("" : "+v"(w), "+v"(wp));
#pragma unroll
    for (int i = 0; i < CH; i += 2) bfly<V, INV>(y[i], y[i + 1], w, wp, k);
    const u64 r = y[0];                       // rotate so the chains mix (X of one feeds Y of the next)
#pragma unroll
    for (int i = 0; i + 1 < CH; i++) y[i] = y[i + 1];
    y[CH - 1] = r;
  }
  u64 acc = 0; for (int i = 0; i < CH; i++) acc += y[i];
  out[blockIdx.x * 256 + threadIdx.x] = acc;
}
template <int V, bool INV>
__global__ void k_chk_bfly(u64* xy, const u64* tw, u64 q, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const QK k(q, std::true_type{});
  u64 X = xy[2 * i], Y = xy[2 * i + 1];
  bfly<V, INV>(X, Y, tw[2 * i], tw[2 * i + 1], k);
  xy[2 * i] = X; xy[2 * i + 1] = Y;
  (void)n;
}

struct Ctx { int cus; u64 q; u64 *dtw, *dxy, *dout; std::vector<u64> tw; int N; hipEvent_t e0, e1; };

template <class F>
static void time3(Ctx& c, int ops_per_iter, F launch, double (&ns)[3]) {
  int wi = 0;
  for (int wps : {1, 4, 8}) {
    const int blocks = c.cus * wps;           // 4 waves per block: wps waves per SIMD
    launch(blocks);                           // untimed
    (void)hipEventRecord(c.e0);
    launch(blocks);
    (void)hipEventRecord(c.e1); (void)hipEventSynchronize(c.e1);
    float ms; (void)hipEventElapsedTime(&ms, c.e0, c.e1);
    ns[wi++] = ms * 1e6 / ((double)ITER * ops_per_iter * wps);
  }
}

// exactness inputs for the trims: every special value in every lane position of a wave whose other lanes hold
// in-range values (so decisions differ inside the wave), alternating below / above m, and random 64-bit values
static std::vector<u64> trim_inputs(u64 m, bool in_range_only) {
  std::vector<u64> sp = {0, m - 1, m, m + 1, 2 * m - 1};
  if (!in_range_only) { sp.push_back(((u64)1 << 63) - 1); sp.push_back((u64)1 << 63); sp.push_back(((u64)1 << 63) + 1); sp.push_back(~(u64)0); }
  std::mt19937_64 rng(11);
  std::vector<u64> in;
  for (u64 s : sp) for (int lane = 0; lane < 64; lane++) for (int l = 0; l < 64; l++)
    in.push_back(l == lane ? s : (u64)(((u128)rng() * (2 * m)) >> 64));
  for (u64 s : sp) for (int l = 0; l < 64; l++) in.push_back(s);                       // a whole wave of each
  for (int i = 0; i < 64 * 64; i++) in.push_back((i & 1) ? m + rng() % m : rng() % m);  // alternating decisions
  for (int i = 0; i < 64 * 64; i++) in.push_back(((i >> 1) & 1) ? m + rng() % m : rng() % m);
  for (int i = 0; i < (1 << 16); i++) in.push_back(in_range_only ? (u64)(((u128)rng() * (2 * m)) >> 64) : rng());
  while (in.size() % 256) in.push_back(0);
  return in;
}

template <int V>
static void run_trim(Ctx& c, const char* name, int valu) {
  const u64 q = c.q, m = 4 * q;
  // the select form needs |x - m| < 2^63 and the second trim of a pair x < 2 m2: those variants get [0,2m) only
  const bool in_range_only = (V == T_SEL || V == T_SEL2);
  long bad = 0, total = 0;
  if constexpr (V != T_NONE) {
    std::vector<u64> in = trim_inputs(m, in_range_only), got(in.size());
    for (int partial = 0; partial < 2; partial++) {
      (void)hipMemcpy(c.dxy, in.data(), in.size() * 8, hipMemcpyHostToDevice);
      hipLaunchKernelGGL((k_chk_trim<V>), dim3(in.size() / 256), dim3(256), 0, 0, c.dxy, q, partial);
      (void)hipMemcpy(got.data(), c.dxy, in.size() * 8, hipMemcpyDeviceToHost);
      for (size_t i = 0; i < in.size(); i++) {
        u64 e = ref_trim(in[i], m);
        if (is_double(V)) e = ref_trim(e, 2 * q);
        bad += (got[i] != e);
      }
    }
    total = (long)in.size();
  }
  double ns[3];
  time3(c, CH, [&](int blocks) { hipLaunchKernelGGL((k_thr_trim<V>), dim3(blocks), dim3(256), 0, 0, c.dout, q); }, ns);
  printf("%-58s VALU %d  checked %7ld bad %ld | ns per wave-op per SIMD at 1/4/8 waves per SIMD: %6.2f %6.2f %6.2f\n", name, valu, total, bad, ns[0], ns[1], ns[2]);
}

template <int V, bool INV>
static void run_bfly(Ctx& c, const char* name, std::vector<u64>* keep) {
  const u64 q = c.q; const int N = c.N;
  std::mt19937_64 rng(7);
  std::vector<u64> in(2 * (size_t)N), xy(2 * (size_t)N);
  const u64 bX = INV ? 4 : 8, bY = INV ? 4 : 0;
  auto draw = [&](u64 boundq, int i) -> u64 {                 // boundq = 0: any 64-bit value
    u64 r = rng();
    if (boundq == 0) return (i % 97 == 0) ? ~0ull - (r % 3) : r;
    if (i % 97 == 0) return boundq * q - 1 - (r % 3);
    if (i % 89 == 0) return r % 3;
    if (i % 83 == 0) return 4 * q - 1 + (r % 3) < boundq * q ? 4 * q - 1 + (r % 3) : 4 * q - 1;   // around the trim's threshold
    return (u64)(((u128)r * (boundq * q)) >> 64);
  };
  for (int i = 0; i < N; i++) { in[2 * i] = draw(bX, i); in[2 * i + 1] = draw(bY, i + 31); }
  (void)hipMemcpy(c.dxy, in.data(), 16ull * N, hipMemcpyHostToDevice);
  hipLaunchKernelGGL((k_chk_bfly<V, INV>), dim3(N / 256), dim3(256), 0, 0, c.dxy, c.dtw, q, N);
  (void)hipMemcpy(xy.data(), c.dxy, 16ull * N, hipMemcpyDeviceToHost);
  long bad = 0, differ = 0;
  const u64 outB = INV ? 4 : 8;
  for (int i = 0; i < N; i++) {
    const u64 X = in[2 * i] % q, Y = in[2 * i + 1] % q, w = c.tw[2 * i]; u64 ex, ey;
    if (!INV) { u64 t = (u64)((u128)Y * w % q); ex = (X + t) % q; ey = (X + q - t) % q; }
    else { ex = (X + Y) % q; ey = (u64)((u128)((X + q - Y) % q) * w % q); }
    if (xy[2 * i] % q != ex || xy[2 * i + 1] % q != ey || xy[2 * i] >= outB * q || xy[2 * i + 1] >= outB * q) bad++;
  }
  if (V == 0) *keep = xy;
  else for (size_t i = 0; i < xy.size(); i++) differ += (xy[i] != (*keep)[i]);
  double ns[3];
  time3(c, CH / 2, [&](int blocks) { hipLaunchKernelGGL((k_thr_bfly<V, INV>), dim3(blocks), dim3(256), 0, 0, c.dout, c.dtw, q); }, ns);
  printf("%-58s checked %7d bad %ld, words differing from the select form %ld | ns per wave-bfly per SIMD at 1/4/8: %6.2f %6.2f %6.2f\n", name, N, bad, differ, ns[0], ns[1], ns[2]);
}

int main() {
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, 0) != hipSuccess) { printf("no device\n"); return 1; }
  Ctx c; c.cus = pr.multiProcessorCount; c.q = 1152921504606994433ull; c.N = 1 << 20;     // 2^60 + 9 2^14 + 1
  const u64 q = c.q;
  std::mt19937_64 rng(1);
  c.tw.resize(2 * (size_t)c.N);
  for (int i = 0; i < c.N; i++) { u64 w = rng() % q; if (i % 101 == 0) w = q - 1 - (i % 3); c.tw[2 * i] = w; c.tw[2 * i + 1] = (u64)(((u128)w << 64) / q); }
  (void)hipMalloc(&c.dtw, 16ull * c.N); (void)hipMalloc(&c.dxy, 16ull * c.N);
  (void)hipMemcpy(c.dtw, c.tw.data(), 16ull * c.N, hipMemcpyHostToDevice);
  (void)hipMalloc(&c.dout, (size_t)c.cus * 8 * 256 * 8);
  (void)hipEventCreate(&c.e0); (void)hipEventCreate(&c.e1);
  printf("device %s CUs=%d q=%llu LOLHIP_CSUB_EXEC=%d\n", pr.name, c.cus, (unsigned long long)q, LOLHIP_CSUB_EXEC);
  printf("# trims: every row also carries one v_lshl_add_u64 (x + inc) per op; row 0 is that add alone\n");
  run_trim<T_NONE>(c, "0  x + inc only (loop overhead)", 1);
  run_trim<T_SEL>(c, "a  csubn: add, v_cmp_gt_i64, 2 v_cndmask", 5);
  run_trim<T_XRAW>(c, "b  four-instruction block (save, v_cmpx, add, restore)", 3);
  run_trim<T_X>(c, "b' csubx(): b + s_nop 1 tail", 3);
  run_trim<T_XSAVEDRAW>(c, "c  save hoisted: one s_mov_b64 per 8 trims", 3);
  run_trim<T_XSAVED>(c, "c' csubx(.., saved): c + s_nop 1 tail", 3);
  run_trim<T_SEL2>(c, "d  csubn(csubn(x, 4q), 2q)", 9);
  run_trim<T_X2RAW>(c, "d  two predicated trims in one block, EXEC restored between", 5);
  run_trim<T_X2>(c, "d' csubx2(): d + s_nop 1 tail", 5);
  std::vector<u64> keepF, keepG;
  run_bfly<0, false>(c, "e  forward, select form", &keepF);
  run_bfly<1, false>(c, "e  forward, trim inside the first Shoup block", &keepF);
  run_bfly<3, false>(c, "e  forward, csubx() as a block of its own", &keepF);
  run_bfly<2, false>(c, "e  forward, bfly_fwd<1> of this build", &keepF);
  run_bfly<0, true>(c, "e  inverse, select form", &keepG);
  run_bfly<1, true>(c, "e  inverse, trim inside the first Shoup block", &keepG);
  run_bfly<3, true>(c, "e  inverse, csubx() as a block of its own", &keepG);
  run_bfly<2, true>(c, "e  inverse, bfly_inv<1> of this build", &keepG);
  return 0;
}
