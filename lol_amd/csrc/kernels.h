// lol_amd/csrc/kernels.h — launcher interface between the C ABI (capi.cpp) and kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "pipeline.h"
#include "plan.h"
#include "tile_host.h"

namespace lolhip {

static const int32_t EMBED_NEG_FLAG_DEV = 1 << 30;   // == hostmath.h EMBED_NEG_FLAG

struct Pow2Launch {
  hipStream_t stream;
  i64* y;            // in-place operand (modes 0,1) or output c (mode 2)
  const i64* a;      // mode 2 inputs
  const i64* b;
  i64 B;
  int T;
  int L;
  const void *tw_fwd, *tw_inv, *scale;   // Shoup-pair tables: u64 pairs (arith 0/1) or u32 pairs (arith 2)
  const ModCtx* mod;
  int arith;         // 4: every modulus < 2^27; 2: < 2^30; 3: < 2^31 (32-bit paths); 1: every modulus < 2^61; 0: exact 64-bit
  int trunc = 0;     // arith 1, mode 2, L >= 11: the truncated transforms with the degree-3 base case (pow2_impl.h)
};
// mode 0 = crt, 1 = crtInv, 2 = fused poly-mul
hipError_t launch_pow2(const Pow2Launch& a, int mode);

// mode 2 only: the persistent, LDS-DMA-pipelined fused poly-mul of the 32-bit classes (pow2_pipe.hip)
bool pow2_pipe_ok(const Pow2Launch& a, bool forced);
hipError_t launch_pow2_pipe(const Pow2Launch& a);

// fused key switch (m = 2^k, 32-bit arithmetic class, two hint coefficients)
struct KeySwitchLaunch {
  hipStream_t stream;
  const i64* c2;        // [B][n][T] powerful basis
  const i64* hint;      // [L][2][n][T] CRT basis
  const i64* addend;    // [2][B][n][T] CRT basis or null
  i64* out;             // [2][B][n][T]
  i64 B;
  int T;
  int L;                // n = 2^L
  const uint32_t* tw_fwd32;
  const ModCtx* mod;
  DecompParams dp;
  uint32_t magic32;     // 32-bit invariant-divisor constant of dp.base
  int arith;            // 2 or 4 (Pow2Launch::arith)
};
hipError_t launch_keyswitch_fused(const KeySwitchLaunch& a);

// The dense route of a stage program at primes above 13 (zqdense.hip; plans created with LOLHIP_ROUTE_DENSE_ZQ).  It rides
// in GenericLaunch, so the host translation units reference no launcher of its own: launch_generic dispatches on `route`.
constexpr int ZQ_MAX_STAGES = 24;
constexpr size_t ZQ_LDS_BUDGET = 152 * 1024;      // dynamic LDS of a workgroup: what launch_generic requests for k_generic
// element-wise on the tile (the arithmetic of k_generic); dense with lanes along the output rows (stride below a wave);
// dense with lanes along r (stride of at least a wave)
enum ZqStageKind : uint8_t { ZQ_ELT = 0, ZQ_ROWS = 1, ZQ_COLS = 2 };
struct ZqDenseLaunch {
  int route = 0;                 // 0: k_generic (everything below unused); 1: dense stages on the vector ALU; 2: on the matrix cores
  int W = 0;                     // route 2: balanced base-256 limbs per residue (2..4)
  int dmax = 0;                  // route 2: the longest dense vector of the program(s) (tile sizing)
  int fold = 0;                  // every modulus < 2^32: products a 64-bit accumulator takes between folds (Plan::zq_fold)
  const i64* src = nullptr;      // input slab when it is not y (null: in place)
  // one-launch poly-mul: y = crtInv(crt(src or y) * crt(b)).  The tile holds both operands side by side as twice the
  // columns; GenericLaunch::stages is the forward program, stages_inv the inverse one, run on the pointwise product
  const i64* b = nullptr;
  const Stage* stages_inv = nullptr;
  int nstages_inv = 0;
  const u64* mt = nullptr;       // transposed word matrices [T][mtpc] (Plan::d_zq_mt)
  i64 mtpc = 0;
  const int8_t* planes = nullptr;      // limb planes [T][plpc] bytes (Plan::d_zq_planes), route 2
  i64 plpc = 0;
  // per stage of the program (the one-launch poly-mul: of `stages`, then of `stages_inv`): how it runs (the host decides, the kernel and the info line obey), the
  // offset into mt / planes of its dense copies and the padded size of a plane (mt_off -1 for an element-wise stage)
  uint8_t kind[ZQ_MAX_STAGES];   // ZqStageKind
  int32_t mt_off[ZQ_MAX_STAGES];
  int32_t dp[ZQ_MAX_STAGES];
  i64 pl_off[ZQ_MAX_STAGES];
};

// The scan route of the prime ops' stage programs (zqscan.hip; plans created with LOLHIP_ROUTE_SCAN_ZQ).  It rides in
// GenericLaunch as the dense route does.  Per stage the host decides the layout, the kernel and the info line obey:
// element-wise (diagonals); the wave scans across lanes (stride below a wave); a lane walks one column (stride of at
// least a wave).
enum ZqScanKind : uint8_t { ZS_ELT = 0, ZS_LANES = 1, ZS_COLS = 2 };
struct ZqScanLaunch {
  int route = 0;                 // 0: not taken (everything below unused); 1: k_zq_scan
  const i64* src = nullptr;      // input slab when it is not y (null: in place)
  const Stage* host_stages = nullptr;   // the program's host copy (the info line)
  uint8_t kind[ZQ_MAX_STAGES] = {};   // ZqScanKind
};

struct GenericLaunch {
  hipStream_t stream;
  i64* y;
  i64 B;
  int T;
  i64 n;
  const Stage* stages;
  int nstages;
  const u64* consts;
  int cpc;
  const ModCtx* mod;
  u64* scratch;
  size_t scratch_bytes;
  bool q32;          // every modulus < 2^32: 32-bit operand products in the dot-product stages
  ZqDenseLaunch zq;  // route 0 unless the plan opted in and the program holds a dense stage of a prime above 13
  ZqScanLaunch scan; // route 0 unless the plan opted in and the program holds a prime-op stage of a prime above 13
};
hipError_t launch_generic(const GenericLaunch& a);
hipError_t launch_zq_dense(const GenericLaunch& a);   // zqdense.hip; called by launch_generic only
hipError_t launch_zq_scan(const GenericLaunch& a);    // zqscan.hip; called by launch_generic only

// vector-per-thread interpreter + fused mixed-radix poly-mul (mixed.hip); every prime <= 13, n <= 8192
struct MixedLaunch {
  hipStream_t stream;
  i64* y;                // output
  const i64* a;          // input (may equal y) / first operand
  const i64* b;          // second operand of the fused poly-mul
  i64 B;
  int T;
  i64 n;
  const Stage* st_a; int n_a;     // the program, or crt for the fused poly-mul
  const Stage* st_b; int n_b;     // crtInv for the fused poly-mul
  bool big = false;               // a program holds 18- or 20-element vectors (merged prime powers, class 2): the BIG kernels
  const u64* consts;              // the pool (classes 2 and 3: the Montgomery copy)
  const uint32_t* consts32;       // its 32-bit copy (classes 1 and 2), else null
  int cpc;
  const ModCtx* mod;
  int cls;               // Plan::mixed_cls (plan.cpp): 0/1 exact division, 2/3 Montgomery with `consts` = the
                         // pool pre-scaled by 2^32 / 2^64
  bool fused;
};
bool mixed_ok(i64 n, const Stage* host_stages, int nstages, const u64* qs, int T);
// fused key switch on the vector interpreter, arithmetic class 2 (mixed_ks.hip): any m with every prime <= 13, n <= 8192
struct MixedKeySwitchLaunch {
  hipStream_t stream;
  const i64* c2;        // [B][n][T] powerful basis
  const i64* hint;      // [L][2][n][T] CRT basis
  const i64* addend;    // [2][B][n][T] CRT basis or null
  i64* out;             // [2][B][n][T]
  i64 B;
  int T;
  i64 n;
  const Stage* st_crt; int n_crt;   // the plan's forward program (device copy)
  const uint32_t* consts32;         // class 2's 32-bit Montgomery pool
  int cpc;
  const ModCtx* mod;
  DecompParams dp;
  uint32_t magic32;     // 32-bit invariant-divisor constant of dp.base
  bool big = false;     // st_crt holds 18-/20-element vectors: only where mixed_keyswitch_big_ok(n)
};
bool mixed_keyswitch_big_ok(i64 n);
hipError_t launch_mixed_keyswitch(const MixedKeySwitchLaunch& a);
hipError_t launch_mixed(const MixedLaunch& a);

// floating-point side (floatpath.hip): y [B][n] complex doubles (re, im interleaved) / doubles, in place.  `word` is a
// stage word (stage_route, tile_host.h): the routes are what pick the kernel, its LDS tile and the info line.
// launch_cplx: a plain count (every stage CPLX_REG) launches k_cplx, as it always did; a word with a dense stage
// (Plan::cplx_word) launches k_cplx_dense over Plan::prog_crtc (plan.h), whose dense stages carry the offsets of their
// matrix forms in the complex pool.  LOLHIP_CPLX_INFO prints one line per launch.
// register vectors; dense on the vector ALU, lanes along the rows; dense on the matrix cores; the vector ALU, lanes along r.
// Two values mean the vector ALU: ask a route whether it is CPLX_REG or CPLX_MFMA, never whether it is CPLX_VALU.
enum CplxRoute : int { CPLX_REG = 0, CPLX_VALU = 1, CPLX_MFMA = 2, CPLX_VALU_COLS = 3 };
hipError_t launch_cplx(hipStream_t s, double* y, i64 B, i64 n, const Stage* stages, int word, const double* cconsts);
// launch_gauss: Plan::gauss_word over Plan::prog_gauss; a plain count launches k_gauss.  LOLHIP_GAUSS_INFO prints one
// line per launch.
enum GaussRoute : int { GAUSS_REG = 0, GAUSS_ROWS = 1, GAUSS_COLS = 2 };   // register vectors; dense, lanes along rows / along r
hipError_t launch_gauss(hipStream_t s, double* y, i64 B, i64 n, const Stage* stages, int word, const double* rconsts);

// 16-byte-per-lane copy of a slab: the measured ceiling of a read-once/write-once kernel (bench.py's yardstick)
hipError_t launch_copy16(hipStream_t s, void* dst, const void* src, size_t bytes, int variant);
hipError_t launch_pointwise_mul(hipStream_t s, i64* a, const i64* b, i64 total, i64 bperiod, int T, const ModCtx* mod);
// replicating: every output has a source (embedCRT) — worth staging the source polynomial in LDS
hipError_t launch_gather(hipStream_t s, i64* out, const i64* in, const int32_t* idx, i64 B, i64 n_out, i64 n_in,
                         int T, const ModCtx* mod, bool replicating = false);
hipError_t launch_twace_crt(hipStream_t s, i64* out, const i64* in, const int32_t* idx, const i64* tweak, i64 B,
                            i64 n_out, i64 n_in, int T, const ModCtx* mod);

}  // namespace lolhip
