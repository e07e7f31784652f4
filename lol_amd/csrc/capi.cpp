// lol_amd/csrc/capi.cpp — the C ABI declared in include/lolhip.h.
//
// Group (A) re-implements the reference's extern "C" Z_q symbols on top of cached
// plans; group (B) is the batched plan API.  No CPU fallback exists: every compute
// entry point needs a HIP device and says so when there is none.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "she_host.h"

using namespace lolhip;

// ---- A/B switches (plan.h): one atomic per switch, seeded once from LOLHIP_<NAME> ------------
namespace lolhip {
namespace {
const char* const kSwitchNames[SW_COUNT] = {"GENERIC_SCALAR", "NO_FUSED2", "NO_POW2_PART", "POLYMUL_UNFUSED",
                                            "KEYSWITCH_UNFUSED", "NO_T1", "NO_PIPE", "FORCE_PIPE", "NO_OWN_DIAG", "NO_MERGE", "NO_LAZY", "NO_KRON", "NO_TRUNC", "ELT_GLOBAL", "LPRF_VALU", "RLWE_RING_UNFUSED", "GAUSS_DENSE", "ZQ_DENSE_VALU", "ZQ_DENSE_MFMA", "CPLX_DENSE", "CPLX_DENSE_VALU", "ZQ_SCAN"};
std::atomic<int> g_switch[SW_COUNT];
std::once_flag g_switch_once;
void switches_init() {
  std::call_once(g_switch_once, [] {
    for (int i = 0; i < SW_COUNT; ++i) {
      const std::string name = std::string("LOLHIP_") + kSwitchNames[i];
      g_switch[i].store(getenv(name.c_str()) != nullptr ? 1 : 0, std::memory_order_relaxed);
    }
  });
}
}  // namespace
bool sw(Switch which) {
  switches_init();
  return g_switch[which].load(std::memory_order_relaxed) != 0;
}
}  // namespace lolhip

namespace {

thread_local int g_last_status = LOLHIP_OK;

int device_count() {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int make_plan(const lolhip_pp* pps, int npps, const int64_t* qs, int T, const int64_t* omega_pp,
              const int64_t* mhatinv, int host_only, lolhip_plan** out, uint32_t flags = 0, uint32_t routes = 0,
              uint32_t known_flags = LOLHIP_PLAN_DENSE_GAUSS,        // the flag and route bits the calling creator honours
              uint32_t known_routes = LOLHIP_ROUTE_DENSE_ZQ) {
  std::vector<PP> v;
  if (!out || T < 1 || !qs || !to_pps(pps, npps, v) || (flags & ~known_flags) || (routes & ~known_routes)) return LOLHIP_ERR_INVALID;
  *out = nullptr;
  std::vector<u64> q;
  for (int t = 0; t < T; ++t) {
    if (qs[t] < 2) return LOLHIP_ERR_MODULUS;
    q.push_back((u64)qs[t]);
  }
  std::vector<u64> om;
  if (omega_pp) for (int i = 0; i < npps * T; ++i) {
    i64 qq = qs[i % T];
    om.push_back((u64)(((omega_pp[i] % qq) + qq) % qq));
  }
  std::unique_ptr<lolhip_plan> p(new lolhip_plan());
  int rc = plan_build_host(p->P, v, q, omega_pp ? om.data() : nullptr, mhatinv, flags, routes);
  if (rc != LOLHIP_OK) return rc;
  if (!host_only) {
    rc = plan_upload(p->P);
    if (rc != LOLHIP_OK) return rc;
  }
  *out = p.release();
  return LOLHIP_OK;
}

bool use_mixed(const Plan& P, const StageProgram& sp) {
  return !sw(SW_GENERIC_SCALAR) && mixed_ok(P.n, sp.stages.data(), (int)sp.stages.size(), P.qs.data(), P.T);
}

// the Z_q CRT programs the vector interpreter runs: the merged prime-power form where the plan has one (class 2)
// big_ok: the caller launches kernels that take 18-/20-element vectors (lone transforms, the fused poly-mul)
const StageProgram& zq_crt(const Plan& P, bool inverse, bool big_ok = true) {
  const StageProgram& plain = inverse ? P.prog_crtinv : P.prog_crt;
  const StageProgram& mg = inverse ? P.prog_crtinv_mg : P.prog_crt_mg;
  const StageProgram& mg_big = inverse ? P.prog_crtinv_mg_big : P.prog_crt_mg_big;
  if (sw(SW_GENERIC_SCALAR)) return plain;
  if (big_ok && !mg_big.stages.empty()) return mg_big;
  return !mg.stages.empty() ? mg : plain;
}
// the one-launch programs of m = 2^e * odd (valid when use_fused2)
const StageProgram& fused_crt(const Plan& P, bool inverse, bool big_ok = true) {
  const StageProgram& big = inverse ? P.prog_crtinv_fused_big : P.prog_crt_fused_big;
  return (big_ok && !big.stages.empty()) ? big : (inverse ? P.prog_crtinv_fused : P.prog_crt_fused);
}

// the launch of the vector interpreter that computes y = program sp of a over the plan's tables (the fused poly-mul
// adds b and its second program)
MixedLaunch mixed_launch(const Plan& P, hipStream_t s, int64_t* y, const int64_t* a, int64_t B, const StageProgram& sp) {
  MixedLaunch m;
  m.stream = s; m.y = y; m.a = a; m.b = nullptr; m.B = B; m.T = P.T; m.n = P.n;
  m.st_a = sp.d_stages; m.n_a = sp.nstages; m.st_b = nullptr; m.n_b = 0; m.big = sp.big;
  m.consts = P.d_consts_mont ? P.d_consts_mont : P.d_consts; m.consts32 = P.d_consts32; m.cpc = P.consts_per_comp;
  m.mod = P.d_mod; m.cls = P.mixed_cls; m.fused = false;
  return m;
}

// Whether the launch of stage program sp takes the dense route (ZqDenseLaunch::route, kernels.h), and which.  ONE
// decision, read by run_prog and by lolhip_plan_zq_route: the plan opted in (LOLHIP_ROUTE_DENSE_ZQ; plan_build_host
// builds the copies for n <= 8192 only), GENERIC_SCALAR is off, the program would go to the scalar interpreter, and
// it holds a stage of a prime above 13.
constexpr int ZQ_MFMA_MIN_D = 48;
int zq_dense_route(const Plan& P, const StageProgram& sp) {
  if (!(P.routes & LOLHIP_ROUTE_DENSE_ZQ) || P.zq_mats.empty() || sw(SW_GENERIC_SCALAR)) return 0;
  if (use_mixed(P, sp) || sp.stages.size() > (size_t)ZQ_MAX_STAGES) return 0;
  int dmax = 0;
  for (const Stage& st : sp.stages) if (zq_dense_stage(st) && st.d > dmax) dmax = st.d;
  if (!dmax) return 0;
  // the matrix cores where every modulus fits W <= 4 balanced limbs (Plan::zq_W) and the longest dense vector is worth
  // a 32-deep unit (ZQ_MFMA_MIN_D, measured: DESIGN.md 3.4q), else the vector ALU
  // (ZQ_DENSE_MFMA lifts the length condition, ZQ_DENSE_VALU wins over it: tests and measurements)
  return (P.zq_W && (dmax >= ZQ_MFMA_MIN_D || sw(SW_ZQ_DENSE_MFMA)) && !sw(SW_ZQ_DENSE_VALU)) ? 2 : 1;
}
const ZqDenseMat* zq_mat_of(const Plan& P, const Stage& st) {
  if (zq_dense_stage(st)) for (const ZqDenseMat& zm : P.zq_mats) if (zm.mat_off == st.mat_off) return &zm;
  return nullptr;
}

// the per-stage fields of ZqDenseLaunch for program sp, written from slot `at` on; the longest dense vector goes to dmax
void zq_fill(const Plan& P, const StageProgram& sp, size_t at, ZqDenseLaunch& z) {
  z.W = P.zq_W; z.fold = P.zq_fold;
  z.mt = P.d_zq_mt; z.mtpc = P.zq_mt_per_comp;
  z.planes = P.d_zq_planes; z.plpc = P.zq_pl_per_comp;
  for (size_t i = 0; i < sp.stages.size(); ++i) {
    const Stage& st = sp.stages[i];
    const ZqDenseMat* zm = zq_mat_of(P, st);
    if (zm && st.d > z.dmax) z.dmax = st.d;
    z.kind[at + i] = !zm ? ZQ_ELT : lanes_along_r(st) ? ZQ_COLS : ZQ_ROWS;
    z.mt_off[at + i] = zm ? zm->mt_off : -1; z.dp[at + i] = zm ? zm->dp : 0; z.pl_off[at + i] = zm ? zm->pl_off : -1;
  }
}

// Whether the launch of stage program sp takes the scan kernel (ZqScanLaunch::route, kernels.h).  ONE decision, read by
// run_prog and by lolhip_plan_scan_route: the plan opted in (LOLHIP_ROUTE_SCAN_ZQ), GENERIC_SCALAR is off, n <= 8192
// (one LDS buffer of a polynomial), the program would go to the scalar interpreter, it holds at most ZQ_MAX_STAGES
// stages, nothing but prime-op stages and diagonals (what the kernel runs in place; true of every prime-op program),
// and a prime-op stage of a prime above 13.  ZQ_SCAN (tests, measurements) drops the last condition and the
// interpreter condition, so the indices the vector interpreter runs can be compared against it.
int zq_scan_route(const Plan& P, const StageProgram& sp) {
  if (!(P.routes & LOLHIP_ROUTE_SCAN_ZQ) || sw(SW_GENERIC_SCALAR) || P.n > 8192) return 0;
  const bool forced = sw(SW_ZQ_SCAN);
  if ((!forced && use_mixed(P, sp)) || sp.stages.size() > (size_t)ZQ_MAX_STAGES) return 0;
  bool hit = false;
  for (const Stage& st : sp.stages) {
    if (zq_scan_stage(st)) hit = hit || st.p > 13 || forced;
    else if (st.kind != ST_DIAG && st.kind != ST_SCALE) return 0;
  }
  return hit ? 1 : 0;
}

bool q_below(const Plan& P, int bits) {
  for (u64 q : P.qs) if (q >> bits) return false;
  return true;
}

// m = 2^e * odd in one launch of the vector interpreter (plan.h: prog_crt_fused)
bool use_fused2(const Plan& P) {
  return !sw(SW_NO_FUSED2) && P.fused2 && use_mixed(P, P.prog_crt_fused) && use_mixed(P, P.prog_crtinv_fused);
}

int run_pow2(const Plan& P, int mode, hipStream_t s, int64_t* y, const int64_t* a, const int64_t* b, int64_t B) {
  Pow2Launch l;
  l.stream = s; l.y = y; l.a = a; l.b = b; l.B = B; l.T = P.T; l.L = P.pow2.L;
  l.mod = P.d_mod;
  if (P.pow2.arith32) {             // every modulus < 2^27 (class 4), < 2^30 (2) or < 2^31 (3): 32-bit arithmetic
    l.arith = P.pow2.arith32; l.tw_fwd = P.pow2.d_tw_fwd32; l.tw_inv = P.pow2.d_tw_inv32; l.scale = P.pow2.d_scale32;
  } else {
    l.arith = 1;
    for (u64 q : P.qs) if (q >= (1ull << 61) || !(q & 1)) l.arith = 0;      // class 1's pointwise product is a Montgomery step: odd q
    l.tw_fwd = P.pow2.d_tw_fwd; l.tw_inv = P.pow2.d_tw_inv; l.scale = P.pow2.d_scale;
    l.trunc = (l.arith == 1 && mode == 2 && !sw(SW_NO_TRUNC)) ? 1 : 0;
  }
  return hip_status(launch_pow2(l, mode));
}

}  // namespace

// ---- what the other host translation units call too (she_host.h) --------------------------------------------------
namespace lolhip {

int need_device(const Plan& P) {
  if (!P.device) return LOLHIP_ERR_NO_DEVICE;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LOLHIP_ERR_HIP;
  if (dev != P.device_id) return LOLHIP_ERR_DEVICE;        // the plan's tables live on another GPU
  return LOLHIP_OK;
}

int need_device(const lolhip_plan* p) { return p ? need_device(p->P) : LOLHIP_ERR_INVALID; }

int run_prog(const Plan& P, const StageProgram& sp, hipStream_t s, int64_t* y, int64_t B, const int64_t* src) {
  const int scan = zq_scan_route(P, sp);          // before the vector interpreter: ZQ_SCAN takes its indices too
  if (!scan && use_mixed(P, sp)) return hip_status(launch_mixed(mixed_launch(P, s, y, src ? src : y, B, sp)));
  GenericLaunch a;
  a.stream = s; a.y = y; a.B = B; a.T = P.T; a.n = P.n;
  a.stages = sp.d_stages; a.nstages = sp.nstages;
  a.consts = P.d_consts; a.cpc = P.consts_per_comp; a.mod = P.d_mod;
  StreamBuf ring(s);
  a.scratch = nullptr; a.scratch_bytes = 0;
  if (P.needs_scratch && B > 0) {       // one ping-pong pair per resident workgroup, at most 512 of them
    const i64 groups = B * P.T < 512 ? B * P.T : 512;
    a.scratch_bytes = (size_t)groups * 2 * (size_t)P.n * sizeof(u64);
    if (!ring.alloc(a.scratch_bytes)) return LOLHIP_ERR_HIP;
    a.scratch = (u64*)ring.p;
  }
  a.q32 = true;
  for (u64 q : P.qs) if (q >= ((u64)1 << 32)) a.q32 = false;
  if (scan) {                           // the scan kernel reads src itself
    a.scan.route = scan;
    a.scan.src = (src && src != y) ? src : nullptr;
    a.scan.host_stages = sp.stages.data();
    for (size_t i = 0; i < sp.stages.size(); ++i)
      a.scan.kind[i] = !zq_scan_stage(sp.stages[i]) ? ZS_ELT : lanes_along_r(sp.stages[i]) ? ZS_COLS : ZS_LANES;
    return hip_status(launch_generic(a));
  }
  a.zq.route = zq_dense_route(P, sp);
  if (a.zq.route) {                     // the dense kernels read src themselves
    zq_fill(P, sp, 0, a.zq);
    a.zq.src = (src && src != y) ? src : nullptr;
    return hip_status(launch_generic(a));
  }
  if (src && src != y) {                // the scalar interpreter works in place
    if (hipMemcpyAsync(y, src, sizeof(int64_t) * (size_t)(B * P.n * P.T), hipMemcpyDeviceToDevice, s) != hipSuccess) return LOLHIP_ERR_HIP;
  }
  return hip_status(launch_generic(a));
}

// How a lone crt / crtInv of the plan runs.  ONE choice for do_crt and for lolhip_plan_table 10 / 11, so the table
// cannot report a program that is never launched:
//   POW2    the m = 2^k kernels;
//   FUSED2  m = 2^e * odd in one launch of the vector interpreter (2-power tiles + the odd primes' stages), except with
//           64-bit residues and e >= 5, where the m = 2^k kernels' cheaper butterflies outweigh the second pass over
//           the slab (measured at 58 bits: m = 11648 0.62 vs 0.55 ms, m = 14336 0.65 vs 0.52 ms; with the even/odd
//           form of round 3 0.54 vs 0.48 and 0.62 vs 0.50, m = 14400 0.457 vs 0.448; at 26 bits fused wins everywhere);
//   SPLIT   the 2-power factor through the m = 2^k kernels, the odd primes through prog_crt(inv)_odd;
//   STAGES  the stage program alone (zq_crt).
// The 2-power tiles exist in the vector interpreter only: a plan it refuses (mixed_ok) never takes FUSED2.
enum CrtRoute { ROUTE_POW2, ROUTE_FUSED2, ROUTE_SPLIT, ROUTE_STAGES };
CrtRoute crt_route(const Plan& P) {
  if (P.is_pow2) return ROUTE_POW2;
  const bool wide = P.mixed_cls == 0 || P.mixed_cls == 3;
  if (use_fused2(P) && !(wide && P.pow2_part)) return ROUTE_FUSED2;
  if (P.pow2_part && !sw(SW_NO_POW2_PART)) return ROUTE_SPLIT;
  return ROUTE_STAGES;
}
// the stage program of that route (POW2 launches none: the staged list, for inspection)
const StageProgram& crt_route_prog(const Plan& P, CrtRoute r, bool inverse) {
  switch (r) {
    case ROUTE_FUSED2: return fused_crt(P, inverse);
    case ROUTE_SPLIT: return inverse ? P.prog_crtinv_odd : P.prog_crt_odd;
    default: return zq_crt(P, inverse);
  }
}
// poly-mul as ONE launch of the vector interpreter (a-hat in registers, b through the same LDS buffer); otherwise it is
// composed from lone transforms
bool polymul_one_launch(const Plan& P) {
  if (P.is_pow2 || sw(SW_POLYMUL_UNFUSED)) return false;
  const bool fused2 = use_fused2(P);
  const bool split2 = !fused2 && P.pow2_part && !sw(SW_NO_POW2_PART);   // the 2-power factor has its own kernels
  return !split2 && (fused2 || (use_mixed(P, zq_crt(P, false)) && use_mixed(P, zq_crt(P, true))));
}
// the forward / inverse program of that one launch (valid when polymul_one_launch).  ONE choice for
// lolhip_polymul_batch and for lolhip_plan_table 13 / 14
const StageProgram& polymul_prog(const Plan& P, bool inverse) {
  return use_fused2(P) ? fused_crt(P, inverse) : zq_crt(P, inverse);
}

// The poly-mul of an opted-in plan as ONE launch of the dense kernels (zqdense.hip): both operands side by side in the
// LDS tile, the forward program over both, the pointwise product and the inverse program on the first.  Taken when the
// stage programs alone make the transform (no 2-power part with kernels of its own), both take the dense route, they
// hold at most ZQ_MAX_STAGES stages together, and 4 n words (two operands, two ping-pong buffers) fit the LDS budget:
// every n <= 8192 at 4-byte words, n <= 4864 at 8-byte words; and the inverse program, which runs on half the tile, still
// has a whole register tile of columns to work on in a 64 KiB tile (32 columns on the matrix cores, 8 / 4 on the vector
// ALU at 4- / 8-byte words): below that the composed form measured faster.  Returns the route (the vector ALU unless both programs
// take the matrix cores) or 0: composed of lone transforms.  ONE decision, for lolhip_polymul_batch and
// lolhip_plan_zq_route(p, 2).
int zq_polymul_route(const Plan& P) {
  if (P.is_pow2 || !P.has_crt || sw(SW_POLYMUL_UNFUSED) || polymul_one_launch(P)) return 0;
  if (P.pow2_part && !sw(SW_NO_POW2_PART)) return 0;
  const StageProgram& pf = zq_crt(P, false);
  const StageProgram& pi = zq_crt(P, true);
  const int rf = zq_dense_route(P, pf), ri = zq_dense_route(P, pi);
  if (!rf || !ri || pf.stages.size() + pi.stages.size() > (size_t)ZQ_MAX_STAGES) return 0;
  const size_t per = 4 * (size_t)P.n * (q_below(P, 32) ? 4 : 8);
  if (per > ZQ_LDS_BUDGET) return 0;
  const int route = rf == 2 && ri == 2 ? 2 : 1;
  int dmax = 0;
  for (const StageProgram* sp : {&pf, &pi}) for (const Stage& st : sp->stages) if (zq_dense_stage(st) && st.d > dmax) dmax = st.d;
  const size_t items = 64 * 1024 / per > 0 ? 64 * 1024 / per : 1;
  const size_t want = route == 2 ? 32 : q_below(P, 32) ? 8 : 4;
  return items * (size_t)(P.n / dmax) >= want ? route : 0;
}

// crt / crtInv of B polynomials through whichever path the plan has (crt_route)
int do_crt(const Plan& P, hipStream_t s, int64_t* y, int64_t B, bool inverse) {
  const CrtRoute r = crt_route(P);
  const StageProgram& sp = crt_route_prog(P, r, inverse);
  switch (r) {
    case ROUTE_POW2: return run_pow2(P, inverse ? 1 : 0, s, y, nullptr, nullptr, B);
    case ROUTE_SPLIT: {
      const int64_t blocks = B * (P.n >> P.pow2.L);       // contiguous 2^(e-1)-coefficient blocks
      if (!inverse) {
        int rc = run_pow2(P, 0, s, y, nullptr, nullptr, blocks);
        return rc ? rc : run_prog(P, sp, s, y, B);
      }
      int rc = run_prog(P, sp, s, y, B);
      return rc ? rc : run_pow2(P, 1, s, y, nullptr, nullptr, blocks);
    }
    default: return run_prog(P, sp, s, y, B);
  }
}

int divg_ok(const Plan& P) {
  for (u64 v : P.oddrad_inv) if (v == 0) return 0;
  return 1;
}

static int gadlen(u64 b, u64 q) {   // ZqBasic.hs:238-240: base-b digits of q
  int k = 0;
  while (q != 0) { ++k; q /= b; }
  return k;
}

// digit counts and the invariant-divisor constants for `base` over the plan's moduli
int make_decomp(const Plan& P, int64_t base, DecompParams& d) {
  if (P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (base != 0 && base < 2) return LOLHIP_ERR_INVALID;
  d.T = P.T;
  d.base = base;
  d.L = 0;
  for (int t = 0; t < P.T; ++t) {
    d.k[t] = base == 0 ? 1 : gadlen((u64)base, P.qs[t]);
    d.L += d.k[t];
  }
  d.magic = 1; d.sh1 = 0; d.sh2 = 0;
  if (base >= 2) inv_div((u64)base, d.magic, d.sh1, d.sh2);
  return LOLHIP_OK;
}

}  // namespace lolhip

extern "C" {

int lolhip_device_count(void) { return device_count(); }
const char* lolhip_version(void) { return "lolhip 0.1 (gfx950)"; }
int lolhip_last_status(void) { return g_last_status; }
int lolhip_copy_slab(void* stream, void* dst, const void* src, int64_t bytes, int variant) {
  if (bytes < 0 || (bytes && (!dst || !src))) return LOLHIP_ERR_INVALID;
  if (device_count() == 0) return LOLHIP_ERR_NO_DEVICE;
  const hipError_t e = launch_copy16((hipStream_t)stream, dst, src, (size_t)bytes, variant);
  return e == hipSuccess ? LOLHIP_OK : e == hipErrorInvalidValue ? LOLHIP_ERR_INVALID : LOLHIP_ERR_HIP;
}
int lolhip_debug_set(const char* name, int value) {
  if (!name) return LOLHIP_ERR_INVALID;
  switches_init();
  for (int i = 0; i < SW_COUNT; ++i)
    if (!strcmp(name, kSwitchNames[i])) { g_switch[i].store(value ? 1 : 0, std::memory_order_relaxed); return LOLHIP_OK; }
  return LOLHIP_ERR_INVALID;
}

int lolhip_plan_create(const lolhip_pp* pps, int npps, const int64_t* qs, int T, int host_only, lolhip_plan** out) {
  return make_plan(pps, npps, qs, T, nullptr, nullptr, host_only, out);
}
int lolhip_plan_create_roots(const lolhip_pp* pps, int npps, const int64_t* qs, int T, const int64_t* omega_pp,
                             const int64_t* mhatinv, int host_only, lolhip_plan** out) {
  return make_plan(pps, npps, qs, T, omega_pp, mhatinv, host_only, out);
}
int lolhip_plan_create_flags(const lolhip_pp* pps, int npps, const int64_t* qs, int T, int host_only, uint32_t flags,
                             lolhip_plan** out) {
  return make_plan(pps, npps, qs, T, nullptr, nullptr, host_only, out, flags);
}
int lolhip_plan_create_routes(const lolhip_pp* pps, int npps, const int64_t* qs, int T, int host_only, uint32_t flags,
                              uint32_t routes, lolhip_plan** out) {
  return make_plan(pps, npps, qs, T, nullptr, nullptr, host_only, out, flags, routes);
}
int lolhip_plan_create_opts(const lolhip_pp* pps, int npps, const int64_t* qs, int T, int host_only, const lolhip_plan_opts* opts,
                            lolhip_plan** out) {
  if (out) *out = nullptr;
  if (!opts || opts->size != sizeof(lolhip_plan_opts)) return LOLHIP_ERR_INVALID;
  return make_plan(pps, npps, qs, T, nullptr, nullptr, host_only, out, opts->flags, opts->routes,
                   LOLHIP_PLAN_DENSE_GAUSS | LOLHIP_PLAN_DENSE_CPLX, LOLHIP_ROUTE_DENSE_ZQ | LOLHIP_ROUTE_SCAN_ZQ);
}
int lolhip_plan_cplx_route(const lolhip_plan* p) { return p ? p->P.cplx_route : 0; }
int64_t lolhip_plan_cplx_table(const lolhip_plan* p, int inverse, int stage, int form, double* out, int64_t cap) {
  if (!p || p->P.cplx_route != 2 || stage < 0 || form < 0 || form > 3) return 0;
  const Plan& P = p->P;
  const std::vector<Stage>& st = P.prog_crtc[inverse ? 1 : 0].stages;
  if (stage >= (int)st.size() || stage_route(P.cplx_word[inverse ? 1 : 0], stage) == CPLX_REG) return 0;
  const Stage& s = st[(size_t)stage];
  if (s.kind == ST_DIAG || s.kind == ST_SCALE) return 0;
  const int64_t d = s.d, dpr = (d + 15) / 16 * 16, dpc = (d + 3) / 4 * 4;
  const int64_t avail = form == 0 ? 2 * d * d : dpr * dpc;
  const double* src = P.host_cconsts.data() + (form == 0 ? 2 * (int64_t)s.wp_off : (int64_t)s.pad[0] + (form - 1) * dpr * dpc);
  if (out && cap > 0) std::memcpy(out, src, sizeof(double) * (size_t)(cap < avail ? cap : avail));
  return avail;
}
int lolhip_plan_zq_route(const lolhip_plan* p, int what) {
  if (!p || what < 0 || what > 2) return 0;
  if (what == 2) return zq_polymul_route(p->P);
  const CrtRoute r = crt_route(p->P);
  return r == ROUTE_POW2 ? 0 : zq_dense_route(p->P, crt_route_prog(p->P, r, what == 1));
}
int lolhip_plan_scan_route(const lolhip_plan* p, int op) {
  if (!p) return 0;
  const Plan& P = p->P;
  switch (op) {
    case LOLHIP_OP_L: return zq_scan_route(P, P.prog_l);
    case LOLHIP_OP_LINV: return zq_scan_route(P, P.prog_linv);
    case LOLHIP_OP_MULGPOW: return zq_scan_route(P, P.prog_gpow);
    case LOLHIP_OP_MULGDEC: return zq_scan_route(P, P.prog_gdec);
    case LOLHIP_OP_DIVGPOW: return zq_scan_route(P, P.prog_ginvpow);
    case LOLHIP_OP_DIVGDEC: return zq_scan_route(P, P.prog_ginvdec);
    default: return 0;
  }
}
int64_t lolhip_plan_zq_table(const lolhip_plan* p, int inverse, int stage, int t, int limb, int64_t* out, int64_t cap) {
  if (!p || t < 0 || t >= p->P.T || stage < 0 || limb < -1) return 0;
  const Plan& P = p->P;
  const CrtRoute r = crt_route(P);
  if (r == ROUTE_POW2) return 0;
  const StageProgram& sp = crt_route_prog(P, r, inverse != 0);
  if (stage >= (int)sp.stages.size() || !zq_dense_route(P, sp)) return 0;
  const ZqDenseMat* zm = zq_mat_of(P, sp.stages[(size_t)stage]);
  if (!zm) return 0;
  if (limb < 0) {
    const int64_t avail = (int64_t)zm->d * zm->d;
    const u64* src = P.host_zq_mt.data() + (size_t)t * P.zq_mt_per_comp + zm->mt_off;
    for (int64_t i = 0; out && i < cap && i < avail; ++i) out[i] = (int64_t)src[i];
    return avail;
  }
  if (limb >= P.zq_W || zm->pl_off < 0) return 0;
  const int64_t avail = (int64_t)zm->dp * zm->dp;
  const int8_t* src = P.host_zq_planes.data() + (size_t)t * P.zq_pl_per_comp + zm->pl_off + (size_t)limb * avail;
  for (int64_t i = 0; out && i < cap && i < avail; ++i) out[i] = src[i];
  return avail;
}
int lolhip_plan_gauss_route(const lolhip_plan* p) { return p ? p->P.gauss_route : 0; }
int64_t lolhip_plan_gauss_table(const lolhip_plan* p, int k, int transposed, double* out, int64_t len) {
  if (!p || k < 0 || k >= (int)p->P.pps.size() || p->P.pps[(size_t)k].p == 2) return 0;
  for (const Stage& st : p->P.prog_gauss.stages) {
    if (st.p != p->P.pps[(size_t)k].p) continue;
    const int off = transposed ? st.wp_off : st.mat_off;
    if (off <= 0) return 0;
    const int64_t avail = (int64_t)st.d * st.d;
    if (out && len > 0) std::memcpy(out, p->P.host_rconsts.data() + off, sizeof(double) * (size_t)(len < avail ? len : avail));
    return avail;
  }
  return 0;
}
void lolhip_plan_destroy(lolhip_plan* p) { delete p; }
int64_t lolhip_plan_n(const lolhip_plan* p) { return p ? p->P.n : 0; }
int64_t lolhip_plan_m(const lolhip_plan* p) { return p ? p->P.m : 0; }
int lolhip_plan_T(const lolhip_plan* p) { return p ? p->P.T : 0; }
int lolhip_plan_has_crt(const lolhip_plan* p) { return p && p->P.has_crt ? 1 : 0; }

int64_t lolhip_plan_table(const lolhip_plan* p, int which, int k, int64_t* out, int64_t len) {
  if (!p) return 0;
  const Plan& P = p->P;
  const std::vector<i64>* src = nullptr;
  std::vector<i64> tmp;
  switch (which) {
    case 0: if (k >= 0 && k < (int)P.ru.size()) src = &P.ru[(size_t)k]; break;
    case 1: if (k >= 0 && k < (int)P.ruinv.size()) src = &P.ruinv[(size_t)k]; break;
    case 2: if (P.has_crt) src = &P.mhatinv; break;
    case 3: src = &P.gcrt; break;
    case 4: if (P.has_ginvcrt) src = &P.ginvcrt; break;
    case 5: for (u64 q : P.qs) tmp.push_back((i64)q); src = &tmp; break;
    case 10: case 11:        // the stage program a lone crt (10) / crtInv (11) launches (do_crt's own choice), four values per stage
    case 13: case 14: {      // the forward (13) / inverse (14) program of the one-launch poly-mul; empty when it is composed of lone transforms
      const bool inv = which == 11 || which == 14;
      const StageProgram* sp = nullptr;
      if (which <= 11) sp = &crt_route_prog(P, crt_route(P), inv);
      else if (polymul_one_launch(P)) sp = &polymul_prog(P, inv);
      if (sp) for (const Stage& st : sp->stages) { tmp.push_back(st.kind); tmp.push_back(st.p); tmp.push_back(st.d); tmp.push_back(st.rts); }
      src = &tmp;
      break;
    }
    case 20: case 21: {      // the stage program of crtc (20) / crtinvc (21), five values per stage, the route last
      const int dir = which - 20;
      if (P.cplx_route) {
        const std::vector<Stage>& st = (dir ? P.prog_crtinv : P.prog_crt).stages;
        for (size_t i = 0; i < st.size(); ++i) {
          tmp.push_back(st[i].kind); tmp.push_back(st[i].p); tmp.push_back(st[i].d); tmp.push_back(st[i].rts);
          const int r = P.cplx_route == 2 ? stage_route(P.cplx_word[dir], (int)i) : 0;
          tmp.push_back(r == CPLX_VALU_COLS ? CPLX_VALU : r);       // the table tells the unit, not the layout
        }
      }
      src = &tmp;
      break;
    }
    case 12:                 // the lift constants of errorTerm / decrypt (plan.h lift_consts), [T + T*T + T]
      tmp.assign(P.lift_consts.begin(), P.lift_consts.end());
      src = &tmp;
      break;
    default: break;
  }
  if (!src) return 0;
  const int64_t avail = (int64_t)src->size();
  if (out && len > 0) std::memcpy(out, src->data(), sizeof(int64_t) * (size_t)(len < avail ? len : avail));
  return avail;
}

int64_t lolhip_good_q(int64_t m, int64_t lower) {
  if (m < 1 || lower < 0) return 0;
  return (int64_t)first_good_q((u64)m, (u64)lower);
}

// ---- batched device-pointer operations ---------------------------------------------

int lolhip_crt_batch(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  return do_crt(p->P, (hipStream_t)stream, y, B, false);
}
int lolhip_crtinv_batch(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  return do_crt(p->P, (hipStream_t)stream, y, B, true);
}
int lolhip_mul_batch(const lolhip_plan* p, void* stream, int64_t* a, const int64_t* b, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (B < 0 || (B > 0 && (!a || !b))) return LOLHIP_ERR_INVALID;
  const i64 total = B * p->P.n * p->P.T;
  return launch_pointwise_mul((hipStream_t)stream, a, b, total, total > 0 ? total : 1, p->P.T, p->P.d_mod) == hipSuccess
             ? LOLHIP_OK : LOLHIP_ERR_HIP;
}
int lolhip_polymul_batch(const lolhip_plan* p, void* stream, int64_t* c, const int64_t* a, const int64_t* b, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (B < 0 || (B > 0 && (!a || !b || !c))) return LOLHIP_ERR_INVALID;
  const Plan& P = p->P;
  hipStream_t s = (hipStream_t)stream;
  if (P.is_pow2) return run_pow2(P, 2, s, c, a, b, B);
  if (polymul_one_launch(P)) {
    // one launch: a-hat in registers, b through the same LDS buffer, 3 slab passes (mixed.hip)
    const StageProgram& pf = polymul_prog(P, false);
    const StageProgram& pi = polymul_prog(P, true);
    MixedLaunch m = mixed_launch(P, s, c, a, B, pf);
    m.b = b; m.st_b = pi.d_stages; m.n_b = pi.nstages; m.fused = true; m.big = pf.big || pi.big;
    return hip_status(launch_mixed(m));
  }
  if (const int zr = zq_polymul_route(P)) {
    // one launch of the dense kernels: a and b side by side in the tile, 3 slab passes (zqdense.hip)
    const StageProgram& pf = zq_crt(P, false);
    const StageProgram& pi = zq_crt(P, true);
    GenericLaunch g;
    g.stream = s; g.y = c; g.B = B; g.T = P.T; g.n = P.n;
    g.stages = pf.d_stages; g.nstages = pf.nstages;
    g.consts = P.d_consts; g.cpc = P.consts_per_comp; g.mod = P.d_mod;
    g.scratch = nullptr; g.scratch_bytes = 0;
    g.q32 = q_below(P, 32);
    g.zq.route = zr;
    zq_fill(P, pf, 0, g.zq);
    zq_fill(P, pi, pf.stages.size(), g.zq);
    g.zq.src = a != c ? a : nullptr;
    g.zq.b = b; g.zq.stages_inv = pi.d_stages; g.zq.nstages_inv = pi.nstages;
    return hip_status(launch_generic(g));
  }
  // otherwise: crt(a) -> c, crt(b) -> temp, multiply, crtInv.  c may alias a or b.  The temp is a
  // stream-ordered allocation of this call (the pool recycles it: no device synchronisation).
  const size_t bytes = sizeof(int64_t) * (size_t)(B * P.n * P.T);
  if (bytes == 0) return LOLHIP_OK;
  StreamBuf tmpbuf(s);
  if (!tmpbuf.alloc(bytes)) return LOLHIP_ERR_HIP;
  int64_t* tmp = (int64_t*)tmpbuf.p;
  rc = LOLHIP_OK;
  if (!P.pow2_part || sw(SW_NO_POW2_PART)) {
    // stage program alone: transform b into the temp first (c may alias b), then a into c
    rc = run_prog(P, zq_crt(P, false), s, tmp, B, b);
    if (!rc) rc = run_prog(P, zq_crt(P, false), s, c, B, c != a ? a : nullptr);
  } else {
    if (hipMemcpyAsync(tmp, b, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = LOLHIP_ERR_HIP;
    if (!rc && c != a && hipMemcpyAsync(c, a, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = LOLHIP_ERR_HIP;
    if (!rc) rc = do_crt(P, s, c, B, false);
    if (!rc) rc = do_crt(P, s, tmp, B, false);
  }
  if (!rc) rc = lolhip_mul_batch(p, stream, c, tmp, B);
  if (!rc) rc = do_crt(P, s, c, B, true);
  return rc;
}

#define PRIME_OP(NAME, PROG)                                                            \
  int NAME(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {                 \
    int rc = need_device(p); if (rc) return rc;                                         \
    if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;                              \
    return run_prog(p->P, p->P.PROG, (hipStream_t)stream, y, B);                        \
  }
PRIME_OP(lolhip_l_batch, prog_l)
PRIME_OP(lolhip_linv_batch, prog_linv)
PRIME_OP(lolhip_mulgpow_batch, prog_gpow)
PRIME_OP(lolhip_mulgdec_batch, prog_gdec)

int lolhip_divgpow_batch(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!divg_ok(p->P)) return LOLHIP_ERR_NOT_DIVISIBLE;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  return run_prog(p->P, p->P.prog_ginvpow, (hipStream_t)stream, y, B);
}
int lolhip_divgdec_batch(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!divg_ok(p->P)) return LOLHIP_ERR_NOT_DIVISIBLE;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  return run_prog(p->P, p->P.prog_ginvdec, (hipStream_t)stream, y, B);
}
int lolhip_mulgcrt_batch(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  const i64 per = p->P.n * p->P.T;
  return hip_status(launch_pointwise_mul((hipStream_t)stream, y, p->P.d_gcrt, B * per, per, p->P.T, p->P.d_mod));
}
int lolhip_divgcrt_batch(const lolhip_plan* p, void* stream, int64_t* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (!p->P.has_ginvcrt) return LOLHIP_ERR_NOT_DIVISIBLE;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  const i64 per = p->P.n * p->P.T;
  return hip_status(launch_pointwise_mul((hipStream_t)stream, y, p->P.d_ginvcrt, B * per, per, p->P.T, p->P.d_mod));
}

// ---- floating-point members of the class ---------------------------------

static int cplx_ready(const lolhip_plan* p) {
  int rc = need_device(p); if (rc) return rc;
  return p->P.cplx_route ? LOLHIP_OK : LOLHIP_ERR_INVALID;    // n > 8192, or a prime > 13 on a plan that has not opted in
}
// the program and stage word of crtC / crtInvC: the plan's own stage list on k_cplx, or the copy with the offsets of the
// dense forms on k_cplx_dense (Plan::cplx_route)
static int run_cplx(const Plan& P, void* stream, double* y, int64_t B, int dir) {
  const StageProgram& sp = P.cplx_route == 2 ? P.prog_crtc[dir] : (dir ? P.prog_crtinv : P.prog_crt);
  const int word = P.cplx_route == 2 ? P.cplx_word[dir] : sp.nstages;
  return hip_status(launch_cplx((hipStream_t)stream, y, B, P.n, sp.d_stages, word, P.d_cconsts));
}
int lolhip_crtc_batch(const lolhip_plan* p, void* stream, double* y, int64_t B) {
  int rc = cplx_ready(p); if (rc) return rc;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  return run_cplx(p->P, stream, y, B, 0);
}
int lolhip_crtinvc_batch(const lolhip_plan* p, void* stream, double* y, int64_t B) {
  int rc = cplx_ready(p); if (rc) return rc;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  return run_cplx(p->P, stream, y, B, 1);
}
int lolhip_gaussian_dec_batch(const lolhip_plan* p, void* stream, double* y, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.gauss_route) return LOLHIP_ERR_INVALID;           // n > 8192, or a prime > 13 on a plan that has not opted in
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  const Plan& P = p->P;
  return hip_status(launch_gauss((hipStream_t)stream, y, B, P.n, P.prog_gauss.d_stages, P.gauss_word,
                                 P.d_rconsts));
}

// ---- ring-level pipelines ---------------------------------------------

int lolhip_ctmul_crt_batch(const lolhip_plan* p, void* stream, const int64_t* c0, const int64_t* c1,
                           const int64_t* d0, const int64_t* d1, int64_t* e0, int64_t* e1, int64_t* e2, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (!p->P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (p->P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (B < 0 || (B > 0 && (!c0 || !c1 || !d0 || !d1 || !e0 || !e1 || !e2))) return LOLHIP_ERR_INVALID;
  return hip_status(launch_ctmul((hipStream_t)stream, c0, c1, d0, d1, e0, e1, e2, p->P.d_gcrt, B, p->P.n, p->P.T,
                                 p->P.d_mod));
}

int lolhip_decompose_len(const lolhip_plan* p, int64_t base) {
  if (!p) return LOLHIP_ERR_INVALID;
  DecompParams d;
  int rc = make_decomp(p->P, base, d);
  return rc ? rc : d.L;
}

int lolhip_gadget(const lolhip_plan* p, int64_t base, int64_t* out, int64_t cap) {
  if (!p || !out) return LOLHIP_ERR_INVALID;
  DecompParams d;
  int rc = make_decomp(p->P, base, d); if (rc) return rc;
  const int T = p->P.T;
  if (cap < (int64_t)d.L * T) return LOLHIP_ERR_INVALID;
  int j = 0;
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < d.k[t]; ++k, ++j)
      for (int s = 0; s < T; ++s)
        out[(int64_t)j * T + s] = s != t ? 0 : (base == 0 ? 1 % (int64_t)p->P.qs[t] : (int64_t)powmod((u64)base % p->P.qs[t], (u64)k, p->P.qs[t]));
  return d.L;
}

int lolhip_decompose_batch(const lolhip_plan* p, void* stream, const int64_t* c_pow, int64_t base, int64_t* digits,
                           int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  DecompParams d;
  rc = make_decomp(p->P, base, d); if (rc) return rc;
  if (B < 0 || (B > 0 && (!c_pow || !digits))) return LOLHIP_ERR_INVALID;
  return hip_status(launch_decompose((hipStream_t)stream, c_pow, digits, B, p->P.n, d, p->P.d_mod, q_below(p->P, 31)));
}

int lolhip_knapsack_batch(const lolhip_plan* p, void* stream, const int64_t* xs_crt, int L, const int64_t* hint,
                          int K, const int64_t* addend, int64_t* out, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (L < 0 || K < 1 || K > 3 || B < 0 || p->P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (B > 0 && (!out || (L > 0 && (!xs_crt || !hint)))) return LOLHIP_ERR_INVALID;
  return hip_status(launch_knapsack((hipStream_t)stream, xs_crt, L, hint, K, addend, out, B, p->P.n, p->P.T,
                                    p->P.d_mod, q_below(p->P, 29)));
}

}  // extern "C"

namespace {
// `switch` on one plan: the fused single-pass kernel where it applies, else decompose -> crt -> knapsack
int keyswitch_impl(const Plan& P, hipStream_t stream, const int64_t* c2_pow, int64_t base, const int64_t* hint, int K,
                   const int64_t* addend, int64_t* out, int64_t* work, int64_t B) {
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  DecompParams d;
  int rc = make_decomp(P, base, d); if (rc) return rc;
  if (K < 1 || K > 3 || B < 0 || (B > 0 && (!c2_pow || !hint || !out || !work))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  // one fused pass when the plan is in the 32-bit class of the m = 2^k path (every q_t < 2^30)
  if (P.is_pow2 && (P.pow2.arith32 == 2 || P.pow2.arith32 == 4) && K == 2 && (base == 0 || base < ((int64_t)1 << 31)) &&
      (u64)d.L * 2 * (u64)P.n * (u64)P.T * 8 < ((u64)1 << 32) && !sw(SW_KEYSWITCH_UNFUSED)) {
    KeySwitchLaunch l;
    l.stream = stream; l.c2 = c2_pow; l.hint = hint; l.addend = addend; l.out = out; l.B = B;
    l.T = P.T; l.L = P.pow2.L; l.tw_fwd32 = P.pow2.d_tw_fwd32; l.mod = P.d_mod; l.dp = d; l.arith = P.pow2.arith32;
    l.magic32 = magic32(base);
    return hip_status(launch_keyswitch_fused(l));
  }
  // ... and for every other index the vector interpreter takes, in its 32-bit Montgomery class (mixed_ks.hip)
  if (!P.is_pow2 && (P.mixed_cls == 2 || P.mixed_cls == 4) && P.d_consts32 && K == 2 && (base == 0 || base < ((int64_t)1 << 31)) &&
      (u64)d.L * 2 * (u64)P.n * (u64)P.T * 8 < ((u64)1 << 32) && !sw(SW_KEYSWITCH_UNFUSED)) {
    const bool fused2 = use_fused2(P);
    const bool split2 = !fused2 && P.pow2_part && !sw(SW_NO_POW2_PART);
    // the key-switch kernel holds two accumulator sets per coefficient: 20-element vectors only at <= 12 coefficients per thread
    const bool big_ok = mixed_keyswitch_big_ok(P.n);
    const StageProgram& pf = fused2 ? fused_crt(P, false, big_ok) : zq_crt(P, false, big_ok);
    if (!split2 && (fused2 || use_mixed(P, pf))) {
      MixedKeySwitchLaunch l;
      l.stream = stream; l.c2 = c2_pow; l.hint = hint; l.addend = addend; l.out = out; l.B = B; l.T = P.T; l.n = P.n;
      l.st_crt = pf.d_stages; l.n_crt = pf.nstages; l.big = pf.big; l.consts32 = P.d_consts32; l.cpc = P.consts_per_comp; l.mod = P.d_mod; l.dp = d;
      l.magic32 = magic32(base);
      return hip_status(launch_mixed_keyswitch(l));
    }
  }
  if (launch_decompose(stream, c2_pow, work, B, P.n, d, P.d_mod, q_below(P, 31)) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(P, stream, work, (int64_t)d.L * B, false);                 // all L*B digit polynomials in one launch
  if (rc) return rc;
  return hip_status(launch_knapsack(stream, work, d.L, hint, K, addend, out, B, P.n, P.T, P.d_mod, q_below(P, 29)));
}
}  // namespace

extern "C" {

int lolhip_keyswitch_batch(const lolhip_plan* p, void* stream, const int64_t* c2_pow, int64_t base,
                           const int64_t* hint, int K, const int64_t* addend, int64_t* out, int64_t* work, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  return keyswitch_impl(p->P, (hipStream_t)stream, c2_pow, base, hint, K, addend, out, work, B);
}

int lolhip_rescale_drop_batch(const lolhip_plan* p, void* stream, const int64_t* c, int64_t* out, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  const Plan& P = p->P;
  if (P.T < 2 || P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (B < 0 || (B > 0 && (!c || !out))) return LOLHIP_ERR_INVALID;
  RescaleParams r;
  r.T = P.T;
  r.qa_inv[0] = 0;
  for (int s = 1; s < P.T; ++s) {
    r.qa_inv[s] = invmod(P.qs[0] % P.qs[s], P.qs[s]);
    if (r.qa_inv[s] == 0) return LOLHIP_ERR_MODULUS;
  }
  return hip_status(launch_rescale((hipStream_t)stream, c, out, B, P.n, r, P.d_mod));
}

// ---- ring extensions -----------------------------------------------------------------

int lolhip_ext_create(const lolhip_plan* lo, const lolhip_plan* hi, lolhip_ext** out) {
  if (!lo || !hi || !out) return LOLHIP_ERR_INVALID;
  *out = nullptr;
  if (lo->P.T != hi->P.T || lo->P.qs != hi->P.qs) return LOLHIP_ERR_INVALID;
  std::unique_ptr<lolhip_ext> x(new lolhip_ext());
  ExtPlan& X = x->X;
  X.lo = &lo->P; X.hi = &hi->P;
  if (!build_ext_tables(lo->P.pps, hi->P.pps, X.host)) return LOLHIP_ERR_INVALID;
  const int T = lo->P.T;
  // tweak = mhat * g' / (m'hat * g) (Extension.hs:110-125); needs both CRT bases and g^-1
  if (lo->P.has_crt && hi->P.has_crt && lo->P.has_ginvcrt) {
    X.tweak.assign((size_t)(X.host.phi2 * T), 0);
    for (int t = 0; t < T; ++t) {
      const u64 q = lo->P.qs[(size_t)t];
      const u64 ratio = mulmod((u64)hi->P.mhatinv[(size_t)t], (u64)value_hat(lo->P.m) % q, q);
      for (i64 i2 = 0; i2 < X.host.phi2; ++i2) {
        const u64 gi = (u64)lo->P.ginvcrt[(size_t)(X.host.embed_crt[(size_t)i2] * T + t)];
        const u64 gp = (u64)hi->P.gcrt[(size_t)(i2 * T + t)];
        X.tweak[(size_t)(i2 * T + t)] = (i64)mulmod(mulmod(gi, gp, q), ratio, q);
      }
    }
  }
  if (lo->P.device && hi->P.device) {
    if (X.d_twace_powdec.upload(X.host.twace_powdec) || X.d_ext_crt.upload(X.host.ext_crt) ||
        X.d_embed_pow.upload(X.host.embed_pow) || X.d_embed_dec.upload(X.host.embed_dec) ||
        X.d_embed_crt.upload(X.host.embed_crt) || X.d_coeffs.upload(X.host.coeffs) || X.d_tweak.upload(X.tweak))
      return LOLHIP_ERR_HIP;
  }
  *out = x.release();
  return LOLHIP_OK;
}
void lolhip_ext_destroy(lolhip_ext* x) { delete x; }
int64_t lolhip_ext_table(const lolhip_ext* x, int which, int32_t* out, int64_t len) {
  if (!x) return 0;
  const std::vector<int32_t>* src = nullptr;
  std::vector<int32_t> pbp;
  switch (which) {
    case 0: src = &x->X.host.twace_powdec; break;
    case 1: src = &x->X.host.ext_crt; break;
    case 2: src = &x->X.host.embed_pow; break;
    case 3: src = &x->X.host.embed_dec; break;
    case 4: src = &x->X.host.embed_crt; break;
    case 5: src = &x->X.host.coeffs; break;
    case 6: pbp = pow_basis_pow(x->X.host); src = &pbp; break;
    default: return 0;
  }
  const int64_t avail = (int64_t)src->size();
  if (out && len > 0) std::memcpy(out, src->data(), sizeof(int32_t) * (size_t)(len < avail ? len : avail));
  return avail;
}

static int ext_gather(const lolhip_ext* x, void* stream, int64_t* out, const int64_t* in, int64_t B,
                      const int32_t* idx, bool to_hi, bool replicating = false) {
  if (!x) return LOLHIP_ERR_INVALID;
  if (!idx) return LOLHIP_ERR_NO_DEVICE;
  if (B < 0 || (B > 0 && (!out || !in))) return LOLHIP_ERR_INVALID;
  const ExtPlan& X = x->X;
  const i64 n_out = to_hi ? X.host.phi2 : X.host.phi, n_in = to_hi ? X.host.phi : X.host.phi2;
  return hip_status(launch_gather((hipStream_t)stream, out, in, idx, B, n_out, n_in, X.lo->T, X.lo->d_mod,
                                  replicating));
}
int lolhip_twace_powdec_batch(const lolhip_ext* x, void* s, int64_t* lo_out, const int64_t* hi_in, int64_t B) {
  return ext_gather(x, s, lo_out, hi_in, B, x ? x->X.d_twace_powdec.get() : nullptr, false);
}
int lolhip_coeffs_batch(const lolhip_ext* x, void* s, int64_t* lo_out, const int64_t* hi_in, int64_t B) {
  if (!x) return LOLHIP_ERR_INVALID;
  if (!x->X.d_coeffs) return LOLHIP_ERR_NO_DEVICE;
  if (B < 0 || (B > 0 && (!lo_out || !hi_in))) return LOLHIP_ERR_INVALID;
  const ExtPlan& X = x->X;
  return hip_status(launch_coeffs((hipStream_t)s, lo_out, hi_in, X.d_coeffs, B, X.host.phi, X.host.phi2, X.lo->T,
                                  X.lo->d_mod));
}
int lolhip_evallin_batch(const lolhip_ext* x_er, const lolhip_ext* x_es, void* s, const int64_t* r_dec,
                         const int64_t* ys_crt, int64_t* out, int64_t* work, int64_t B) {
  if (!x_er || !x_es) return LOLHIP_ERR_INVALID;
  const ExtPlan &ER = x_er->X, &ES = x_es->X;
  if (!ER.d_coeffs || !ES.d_embed_dec) return LOLHIP_ERR_NO_DEVICE;
  if (ER.host.phi != ES.host.phi || ER.lo->T != ES.lo->T || ER.lo->qs != ES.lo->qs || ER.lo->pps.size() != ES.lo->pps.size())
    return LOLHIP_ERR_INVALID;                                     // the two extensions must share E
  if (ER.lo->T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (!ES.hi->has_crt) return LOLHIP_ERR_NO_CRT;
  if (B < 0 || (B > 0 && (!r_dec || !ys_crt || !out || !work))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  const i64 rel = ER.host.phi2 / ER.host.phi;
  Work w(work);
  const auto [tmp_e, tmp_s] = evallin_work(w, ER, ES, B);
  const Plan* PS = ES.hi;                                          // the S-side plan
  int rc = lolhip_coeffs_batch(x_er, s, tmp_e, r_dec, B);
  if (!rc) rc = lolhip_embed_dec_batch(x_es, s, tmp_s, tmp_e, rel * B);
  if (!rc) rc = run_prog(*PS, PS->prog_l, (hipStream_t)s, tmp_s, rel * B);                 // Dec -> Pow
  if (!rc) rc = do_crt(*PS, (hipStream_t)s, tmp_s, rel * B, false);
  if (rc) return rc;
  return hip_status(launch_knapsack((hipStream_t)s, tmp_s, (int)rel, ys_crt, 1, nullptr, out, B, PS->n, PS->T,
                                    PS->d_mod, q_below(*PS, 29)));
}
int64_t lolhip_tunnel_work_len(const lolhip_ext* x_er, const lolhip_ext* x_es, int64_t base, int64_t B) {
  if (!x_er || !x_es || B < 0) return LOLHIP_ERR_INVALID;
  DecompParams d;
  int rc = make_decomp(*x_es->X.hi, base, d); if (rc) return rc;
  return measure(tunnel_work, x_er->X, x_es->X, d.L, B);
}

// tunnel (SymmSHE.hs:549-570), the body after toMSD . absorbGFactors: with [c0, c1] the linear
// ciphertext over R',
//   c0' = evalLin f c0;   c1s = coeffsPow c1 :: [E'];   c1' = sum_i switch hints_i (embed c1s_i)
//   result = const c0' + c1'     (a linear ciphertext over S', CRT basis)
// as a composition of the batch kernels: evalLin (coeffs gather, embedDec, l, crt, knapsack), then
// ONE coeffs gather and ONE embedPow over all n_R/n_E coefficient vectors, then one key switch
// per coefficient accumulating into the two output slabs.
int lolhip_tunnel_batch(const lolhip_ext* x_er, const lolhip_ext* x_es, void* stream, const int64_t* c0_dec,
                        const int64_t* c1_pow, const int64_t* ys_crt, const int64_t* hints, int64_t base,
                        int64_t* out, int64_t* work, int64_t B) {
  if (!x_er || !x_es) return LOLHIP_ERR_INVALID;
  const ExtPlan &ER = x_er->X, &ES = x_es->X;
  if (!ER.d_coeffs || !ES.d_embed_pow) return LOLHIP_ERR_NO_DEVICE;
  if (ER.host.phi != ES.host.phi || ER.lo->T != ES.lo->T || ER.lo->qs != ES.lo->qs || ER.lo->T > PIPE_MAX_T)
    return LOLHIP_ERR_INVALID;
  if (B < 0 || (B > 0 && (!c0_dec || !c1_pow || !ys_crt || !hints || !out || !work))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  const Plan& PS = *ES.hi;
  DecompParams d;
  int rc = make_decomp(PS, base, d); if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const i64 rel = ER.host.phi2 / ER.host.phi;
  const int T = PS.T;
  const i64 nS = ES.host.phi2;
  const size_t slabS = (size_t)B * nS * T;
  Work w(work);
  const TunnelWork tw = tunnel_work(w, ER, ES, d.L, B);
  int64_t *tmp_e = tw.ev.tmp_e, *tmp_s = tw.ev.tmp_s, *ks_work = tw.dig;
  // c0' into out[0] (evalLin carves tmp_e and tmp_s for itself first); out[1] starts at zero
  rc = lolhip_evallin_batch(x_er, x_es, stream, c0_dec, ys_crt, out, tmp_e, B); if (rc) return rc;
  if (hipMemsetAsync(out + slabS, 0, slabS * sizeof(int64_t), s) != hipSuccess) return LOLHIP_ERR_HIP;
  // coefficient vectors of c1 over the relative powerful basis, embedded into S' (powerful basis)
  rc = lolhip_coeffs_batch(x_er, stream, tmp_e, c1_pow, B); if (rc) return rc;
  rc = lolhip_embed_pow_batch(x_es, stream, tmp_s, tmp_e, rel * B); if (rc) return rc;
  const size_t hint_i = (size_t)d.L * 2 * nS * T;          // one coefficient's hint: [L][2][n_S][T]
  for (i64 i = 0; i < rel; ++i) {
    rc = keyswitch_impl(PS, s, tmp_s + (size_t)i * slabS, base, hints + (size_t)i * hint_i, 2, out, out, ks_work, B);
    if (rc) return rc;
  }
  return LOLHIP_OK;
}

int lolhip_embed_pow_batch(const lolhip_ext* x, void* s, int64_t* hi_out, const int64_t* lo_in, int64_t B) {
  return ext_gather(x, s, hi_out, lo_in, B, x ? x->X.d_embed_pow.get() : nullptr, true);
}
int lolhip_embed_dec_batch(const lolhip_ext* x, void* s, int64_t* hi_out, const int64_t* lo_in, int64_t B) {
  return ext_gather(x, s, hi_out, lo_in, B, x ? x->X.d_embed_dec.get() : nullptr, true);
}
int lolhip_embed_crt_batch(const lolhip_ext* x, void* s, int64_t* hi_out, const int64_t* lo_in, int64_t B) {
  if (x && !(x->X.lo->has_crt && x->X.hi->has_crt)) return LOLHIP_ERR_NO_CRT;   // Extension.hs:81-85 demands crtInfo m'
  return ext_gather(x, s, hi_out, lo_in, B, x ? x->X.d_embed_crt.get() : nullptr, true, true);
}
int lolhip_twace_crt_batch(const lolhip_ext* x, void* s, int64_t* lo_out, const int64_t* hi_in, int64_t B) {
  if (!x) return LOLHIP_ERR_INVALID;
  const ExtPlan& X = x->X;
  if (X.tweak.empty()) return LOLHIP_ERR_NO_CRT;
  if (!X.d_tweak) return LOLHIP_ERR_NO_DEVICE;
  if (B < 0 || (B > 0 && (!lo_out || !hi_in))) return LOLHIP_ERR_INVALID;
  return hip_status(launch_twace_crt((hipStream_t)s, lo_out, hi_in, X.d_ext_crt, X.d_tweak, B, X.host.phi,
                                     X.host.phi2, X.lo->T, X.lo->d_mod));
}

// ---- host-pointer convenience ----------------------------------------------------------

}  // extern "C"

namespace {

// A staging set = one stream, one pinned staging area and two device buffers, grown on demand and kept.
// A host-pointer call CHECKS ONE OUT of a process-wide pool for its duration and returns it (StageLease):
// the steady state is memcpy -> H2D -> kernels -> D2H -> hipStreamSynchronize on that set's own stream — no
// hipMalloc/hipFree, no device-wide synchronisation, nothing shared between concurrent calls (what the
// reference's callers need: CPP.hs:325-337 thaws a fresh vector and calls one tensor*Rq per ring operation).
// The pool holds as many sets as calls have ever run at the same time; nothing belongs to a thread, so a worker
// thread that exits (a GHC safe-FFI worker, a thread pool) leaves nothing behind.  (Round 2 kept the sets in
// thread_local storage without a destructor: every exiting thread leaked a stream, pinned memory and HBM.)
struct HostStage {
  int dev = -1;
  hipStream_t stream = nullptr;
  char* pinned = nullptr; size_t pinned_bytes = 0;
  DevBuf<char> d[2]; size_t d_bytes[2] = {0, 0};
  bool grow_pinned(size_t bytes) {
    if (bytes <= pinned_bytes) return true;
    if (pinned) (void)hipHostFree(pinned);
    pinned = nullptr; pinned_bytes = 0;
    size_t cap = 1 << 16;
    while (cap < bytes) cap <<= 1;
    if (hipHostMalloc((void**)&pinned, cap, hipHostMallocDefault) != hipSuccess) return false;
    pinned_bytes = cap;
    return true;
  }
  bool grow_dev(int i, size_t bytes) {
    if (bytes <= d_bytes[i]) return true;
    if (stream && hipStreamSynchronize(stream) != hipSuccess) return false;
    d[i].reset(); d_bytes[i] = 0;
    size_t cap = 1 << 16;
    while (cap < bytes) cap <<= 1;
    if (d[i].alloc(cap)) return false;
    d_bytes[i] = cap;
    return true;
  }
  void release() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    if (pinned) (void)hipHostFree(pinned);
    *this = HostStage();                          // frees d[]
  }
};
struct StagePool {
  std::mutex mu;
  std::vector<HostStage*> idle;
  HostStage* acquire() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    {
      std::lock_guard<std::mutex> g(mu);
      for (size_t i = 0; i < idle.size(); ++i)
        if (idle[i]->dev == dev) { HostStage* h = idle[i]; idle.erase(idle.begin() + (long)i); return h; }
    }
    HostStage* h = new HostStage();
    h->dev = dev;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return nullptr; }
    return h;
  }
  void give_back(HostStage* h) { std::lock_guard<std::mutex> g(mu); idle.push_back(h); }
  void release_all() {
    std::vector<HostStage*> all;
    { std::lock_guard<std::mutex> g(mu); all.swap(idle); }
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (HostStage* h : all) { (void)hipSetDevice(h->dev); h->release(); delete h; }
    if (cur >= 0) (void)hipSetDevice(cur);
  }
};
StagePool& stage_pool() { static StagePool* pool = new StagePool(); return *pool; }   // never destroyed: no HIP call at process teardown

// one call's hold on a staging set.  `enqueued` = something of this call may be in flight on the set's stream:
// every exit then waits for the stream first, so the next user never copies into a pinned area a transfer is
// still reading.
struct StageLease {
  HostStage* h;
  bool enqueued = false;
  StageLease() : h(stage_pool().acquire()) {}
  ~StageLease() {
    if (!h) return;
    if (enqueued) (void)hipStreamSynchronize(h->stream);
    stage_pool().give_back(h);
  }
  StageLease(const StageLease&) = delete;
  StageLease& operator=(const StageLease&) = delete;
};

}  // namespace

extern "C" {

void lolhip_thread_release(void) { stage_pool().release_all(); }

int lolhip_op_host(const lolhip_plan* p, int op, int64_t* y, const int64_t* b, int64_t B) {
  int rc = need_device(p); if (rc) return rc;
  if (B < 0 || (B > 0 && !y)) return LOLHIP_ERR_INVALID;
  if ((op == LOLHIP_OP_DIVGPOW || op == LOLHIP_OP_DIVGDEC) && !divg_ok(p->P)) return LOLHIP_ERR_NOT_DIVISIBLE;
  if (op < LOLHIP_OP_CRT || op > LOLHIP_OP_DIVGCRT) return LOLHIP_ERR_INVALID;
  const size_t bytes = sizeof(int64_t) * (size_t)(B * p->P.n * p->P.T);
  if (bytes == 0) return LOLHIP_OK;
  const bool two = (op == LOLHIP_OP_MUL || op == LOLHIP_OP_POLYMUL);
  if (two && !b) return LOLHIP_ERR_INVALID;
  StageLease lease;
  HostStage* h = lease.h;
  if (!h) return LOLHIP_ERR_HIP;
  if (!h->grow_pinned(two ? 2 * bytes : bytes) || !h->grow_dev(0, bytes) || (two && !h->grow_dev(1, bytes))) return LOLHIP_ERR_HIP;
  hipStream_t s = h->stream;
  int64_t* dy = (int64_t*)h->d[0].get();
  int64_t* db = (int64_t*)h->d[1].get();
  std::memcpy(h->pinned, y, bytes);
  lease.enqueued = true;                       // from here on every return waits for the stream (StageLease)
  if (hipMemcpyAsync(dy, h->pinned, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return LOLHIP_ERR_HIP;
  if (two) {
    std::memcpy(h->pinned + bytes, b, bytes);
    if (hipMemcpyAsync(db, h->pinned + bytes, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return LOLHIP_ERR_HIP;
  }
  switch (op) {
    case LOLHIP_OP_CRT: rc = lolhip_crt_batch(p, s, dy, B); break;
    case LOLHIP_OP_CRTINV: rc = lolhip_crtinv_batch(p, s, dy, B); break;
    case LOLHIP_OP_MUL: rc = lolhip_mul_batch(p, s, dy, db, B); break;
    case LOLHIP_OP_POLYMUL: rc = lolhip_polymul_batch(p, s, dy, dy, db, B); break;
    case LOLHIP_OP_L: rc = lolhip_l_batch(p, s, dy, B); break;
    case LOLHIP_OP_LINV: rc = lolhip_linv_batch(p, s, dy, B); break;
    case LOLHIP_OP_MULGPOW: rc = lolhip_mulgpow_batch(p, s, dy, B); break;
    case LOLHIP_OP_MULGDEC: rc = lolhip_mulgdec_batch(p, s, dy, B); break;
    case LOLHIP_OP_DIVGPOW: rc = lolhip_divgpow_batch(p, s, dy, B); break;
    case LOLHIP_OP_DIVGDEC: rc = lolhip_divgdec_batch(p, s, dy, B); break;
    case LOLHIP_OP_MULGCRT: rc = lolhip_mulgcrt_batch(p, s, dy, B); break;
    default: rc = lolhip_divgcrt_batch(p, s, dy, B); break;
  }
  if (!rc && hipMemcpyAsync(h->pinned, dy, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) rc = LOLHIP_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return LOLHIP_ERR_HIP;   // also on error: nothing of ours stays in flight
  lease.enqueued = false;
  if (rc) return rc;
  std::memcpy(y, h->pinned, bytes);
  return LOLHIP_OK;
}

int lolhip_ext_host(const lolhip_ext* x, int op, int64_t* out, const int64_t* in, int64_t B) {
  if (!x) return LOLHIP_ERR_INVALID;
  if (!x->X.d_embed_pow) return LOLHIP_ERR_NO_DEVICE;
  if (B < 0 || (B > 0 && (!out || !in))) return LOLHIP_ERR_INVALID;
  const bool to_hi = op >= LOLHIP_EXT_EMBED_POW && op != LOLHIP_EXT_COEFFS;
  const int T = x->X.lo->T;
  const size_t bin = sizeof(int64_t) * (size_t)(B * (to_hi ? x->X.host.phi : x->X.host.phi2) * T);
  const size_t bout = sizeof(int64_t) * (size_t)(B * ((to_hi || op == LOLHIP_EXT_COEFFS) ? x->X.host.phi2 : x->X.host.phi) * T);
  if (bout == 0) return LOLHIP_OK;
  if (op < LOLHIP_EXT_TWACE_POWDEC || op > LOLHIP_EXT_COEFFS) return LOLHIP_ERR_INVALID;
  StageLease lease;
  HostStage* h = lease.h;
  if (!h) return LOLHIP_ERR_HIP;
  if (!h->grow_pinned(bin > bout ? bin : bout) || !h->grow_dev(0, bin) || !h->grow_dev(1, bout)) return LOLHIP_ERR_HIP;
  hipStream_t s = h->stream;
  int64_t* di = (int64_t*)h->d[0].get();
  int64_t* dout = (int64_t*)h->d[1].get();
  std::memcpy(h->pinned, in, bin);
  lease.enqueued = true;
  if (hipMemcpyAsync(di, h->pinned, bin, hipMemcpyHostToDevice, s) != hipSuccess) return LOLHIP_ERR_HIP;
  int rc;
  switch (op) {
    case LOLHIP_EXT_TWACE_POWDEC: rc = lolhip_twace_powdec_batch(x, s, dout, di, B); break;
    case LOLHIP_EXT_TWACE_CRT: rc = lolhip_twace_crt_batch(x, s, dout, di, B); break;
    case LOLHIP_EXT_EMBED_POW: rc = lolhip_embed_pow_batch(x, s, dout, di, B); break;
    case LOLHIP_EXT_EMBED_DEC: rc = lolhip_embed_dec_batch(x, s, dout, di, B); break;
    case LOLHIP_EXT_EMBED_CRT: rc = lolhip_embed_crt_batch(x, s, dout, di, B); break;
    case LOLHIP_EXT_COEFFS: rc = lolhip_coeffs_batch(x, s, dout, di, B); break;
    default: return LOLHIP_ERR_INVALID;
  }
  if (!rc && hipMemcpyAsync(h->pinned, dout, bout, hipMemcpyDeviceToHost, s) != hipSuccess) rc = LOLHIP_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return LOLHIP_ERR_HIP;
  lease.enqueued = false;
  if (rc) return rc;
  std::memcpy(out, h->pinned, bout);
  return LOLHIP_OK;
}

// ---- (A) drop-in symbols ----------------------------------------------------------------
// Plans are cached per (prime powers, moduli, roots); the reference re-derives nothing per
// call either (its twiddles arrive as arguments), so steady-state cost is the transfer.

namespace {

struct PlanCache {
  std::mutex mu;
  std::map<std::vector<int64_t>, lolhip_plan*> plans;
  lolhip_plan* get(const lolhip_pp* pe, int npe, const int64_t* qs, int T, const int64_t* omega, const int64_t* mh, int* rc) {
    std::vector<int64_t> key;
    key.push_back(npe); key.push_back(T);
    for (int i = 0; i < npe; ++i) { key.push_back(pe[i].prime); key.push_back(pe[i].exponent); }
    for (int t = 0; t < T; ++t) key.push_back(qs[t]);
    key.push_back(omega ? 1 : 0);
    if (omega) for (int i = 0; i < npe * T; ++i) key.push_back(omega[i]);
    key.push_back(mh ? 1 : 0);
    if (mh) for (int t = 0; t < T; ++t) key.push_back(mh[t]);
    std::lock_guard<std::mutex> g(mu);
    auto it = plans.find(key);
    if (it != plans.end()) { *rc = LOLHIP_OK; return it->second; }
    lolhip_plan* p = nullptr;
    *rc = make_plan(pe, npe, qs, T, omega, mh, 0, &p);
    if (*rc == LOLHIP_OK) plans[key] = p;
    return p;
  }
};
PlanCache* cache() { static PlanCache c; return &c; }

int check_totm(const lolhip_plan* p, int64_t totm) { return (p && p->P.n == totm) ? LOLHIP_OK : LOLHIP_ERR_INVALID; }

int dropin_prime(int op, int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) {
  int rc;
  lolhip_plan* p = cache()->get(pe, npe, qs, T, nullptr, nullptr, &rc);
  if (rc) return rc;
  if ((rc = check_totm(p, totm))) return rc;
  return lolhip_op_host(p, op, y, nullptr, 1);
}

}  // namespace

void tensorCRTRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t** ru, int64_t* qs) {
  // the caller's omega_{pp_k,t} is ru[k][1*T + t]
  std::vector<int64_t> om;
  for (int k = 0; k < npe; ++k) for (int t = 0; t < T; ++t) om.push_back(ru[k][T + t]);
  int rc;
  lolhip_plan* p = cache()->get(pe, npe, qs, T, npe ? om.data() : nullptr, nullptr, &rc);
  if (!rc) rc = check_totm(p, totm);
  if (!rc) rc = lolhip_op_host(p, LOLHIP_OP_CRT, y, nullptr, 1);
  g_last_status = rc;
}

void tensorCRTInvRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t** ruinv, int64_t* mhatInv, int64_t* qs) {
  // ruinv[k][1*T+t] = omega^-1; invert it back so the plan is keyed on omega itself
  std::vector<int64_t> om;
  int rc = LOLHIP_OK;
  for (int k = 0; k < npe && !rc; ++k) for (int t = 0; t < T; ++t) {
    i64 q = qs[t];
    if (q < 2) { rc = LOLHIP_ERR_MODULUS; break; }
    u64 wi = (u64)(((ruinv[k][T + t] % q) + q) % q);
    u64 w = invmod(wi, (u64)q);
    if (w == 0) { rc = LOLHIP_ERR_ROOT; break; }
    om.push_back((int64_t)w);
  }
  lolhip_plan* p = nullptr;
  if (!rc) p = cache()->get(pe, npe, qs, T, npe ? om.data() : nullptr, mhatInv, &rc);
  if (!rc) rc = check_totm(p, totm);
  if (!rc) rc = lolhip_op_host(p, LOLHIP_OP_CRTINV, y, nullptr, 1);
  g_last_status = rc;
}

void mulRq(int16_t T, int64_t* a, int64_t* b, int64_t totm, int64_t* qs) {
  // no prime powers in this signature: use the index-1 plan (n = 1) over totm "polynomials"
  int rc;
  lolhip_plan* p = cache()->get(nullptr, 0, qs, T, nullptr, nullptr, &rc);
  if (!rc) rc = lolhip_op_host(p, LOLHIP_OP_MUL, a, b, totm);
  g_last_status = rc;
}

void tensorLRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) { g_last_status = dropin_prime(LOLHIP_OP_L, T, y, totm, pe, npe, qs); }
void tensorLInvRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) { g_last_status = dropin_prime(LOLHIP_OP_LINV, T, y, totm, pe, npe, qs); }
void tensorGPowRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) { g_last_status = dropin_prime(LOLHIP_OP_MULGPOW, T, y, totm, pe, npe, qs); }
void tensorGDecRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) { g_last_status = dropin_prime(LOLHIP_OP_MULGDEC, T, y, totm, pe, npe, qs); }
int16_t tensorGInvPowRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) {
  g_last_status = dropin_prime(LOLHIP_OP_DIVGPOW, T, y, totm, pe, npe, qs);
  return g_last_status == LOLHIP_OK ? 1 : 0;
}
int16_t tensorGInvDecRq(int16_t T, int64_t* y, int64_t totm, lolhip_pp* pe, int16_t npe, int64_t* qs) {
  g_last_status = dropin_prime(LOLHIP_OP_DIVGDEC, T, y, totm, pe, npe, qs);
  return g_last_status == LOLHIP_OK ? 1 : 0;
}

}  // extern "C"
