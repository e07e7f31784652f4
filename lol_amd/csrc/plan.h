// lol_amd/csrc/plan.h — the run-time "plan": everything the reference recomputes or
// re-marshals per call (twiddle vectors CPP.hs:422-442, g vectors CPP.hs:444-454,
// moduli Backend.hs:195-199, prime-power list CPP.hs:325-337), built once per
// (prime powers, moduli, roots) and kept resident in HBM.
#pragma once
#include <cstdint>
#include <vector>

#include "devmem.h"
#include "hostmath.h"
#include "zq_dev.h"

namespace lolhip {

// ---- generic (any m) stage program ----------------------------------------
// One stage = (I_lts (x) A (x) I_rts) on a length-n planar component, written
// out-of-place:  out[x] = post[x] * sum_c M(row,c) * (pre * in)[base + c*rts]
// (tensor.h:39-95 gives the lts/rts bookkeeping this flattens).
enum StageKind : int32_t {
  ST_DIAG = 0,     // out[x] = tw[x'] * in[x]                    crtTwiddle (crt.cpp:35-81)
  ST_DFTP = 1,     // p-point DFT, optional post/pre twiddle     dftp+dftTwiddle (crt.cpp:131-246, 84-126)
  ST_CRTP = 2,     // (p-1)-point CRT_p                          crtp (crt.cpp:248-346)
  ST_CRTPINV = 3,  // scaled inverse CRT_p                       crtpinv (crt.cpp:349-457)
  ST_L = 4,        // prefix sums                                lp (l.cpp:28-57)
  ST_LINV = 5,     // adjacent differences                       lpInv (l.cpp:67-98)
  ST_GPOW = 6,     //                                            gPow (g.cpp:16-35)
  ST_GDEC = 7,     //                                            gDec (g.cpp:37-58)
  ST_GINVPOW = 8,  //                                            gInvPow (g.cpp:60-90)
  ST_GINVDEC = 9,  //                                            gInvDec (g.cpp:92-123)
  ST_SCALE = 10,   // out[x] = s * in[x]  (mhatInv crt.cpp:573-579, oddRad^-1 g.cpp:194-204)
  ST_GAUSS = 11,   // real (p-1) x (p-1) map of tensorGaussianDec           primeD (random.cpp:19-50)
  // Levels p .. p+d-1 (1-based, d <= 4) of the negacyclic 2-power transform on every contiguous block of
  // tw_mod = 2^(e-1) coefficients (the innermost tensor factor of m = 2^e * odd, tensor.h:46-73), one
  // 2^d-element register tile per thread: level s pairs x and x + 2^(s-1) inside blocks of 2^s with the
  // twiddle table entry 2^(s-1) + (x mod 2^(s-1)) (the same merged-twist network as the m = 2^k kernels;
  // CRT_{2^e} of crt.cpp:459-538 in a different but exact factorisation).  rts = 2^(p-1).  Z_q programs of
  // the vector interpreter only (mixed_impl.h).
  ST_POW2F = 12,   // forward: X' = X + w Y, Y' = X - w Y, levels ascending
  ST_POW2I = 13    // inverse: X' = X + Y, Y' = w^-1 (X - Y), levels descending; mat_off >= 0: level 1 also carries mhat^-1
};

struct Stage {
  int32_t kind;
  int32_t p;        // prime
  int32_t d;        // vector length (p or p-1; 1 for DIAG/SCALE)
  int32_t rts;      // stride between vector elements
  int32_t wp_off;   // offset (u64 units, per component) of omega_p^j table, j < p; ST_GAUSS: offset of the transposed
                    // matrix in the real pool when the stage takes the dense route (floatpath.hip), 0 for the register route
  int32_t tw_off;   // offset of diagonal table or -1
  int32_t tw_mod;   // diagonal index = (x / tw_div) % tw_mod
  int32_t tw_div;
  int32_t mat_off;  // offset of the d x d coefficient matrix (DFTP/CRTP/CRTPINV), row-major
  // tw_per > 0: the diagonal belongs to THIS stage's own vectors (tw_div == rts, d | tw_mod), so element i of the
  // vector in block blk takes entry (blk mod tw_per) * d + i — one division per vector instead of two per element
  int32_t tw_per;   // tw_mod / d, or 0
  int32_t pad[2];
  // multiply-shift reciprocals (floor(2^40/v)+1) of rts, d, tw_div, tw_mod, tw_per: x/v = (x*M)>>40 for x < 2^20
  uint64_t m_rts, m_d, m_twdiv, m_twmod, m_twper;
};

struct StageProgram {
  std::vector<Stage> stages;   // host copy
  DevBuf<Stage> d_stages;      // device copy
  int nstages = 0;
  bool big = false;            // holds a dense vector of length 18, 20 (merged 3^3 / 5^2) or 8 (3 (x) 5): the BIG kernels of classes 2 / 4 only
};

// ---- power-of-two fast path -------------------------------------------------
struct Pow2Tables {
  int L = 0;                       // n = 2^L
  // per component t, n Shoup pairs: entry (N/2 + i) = psi_N^(2i+1), N = 2..n (entry 0 unused)
  DevBuf<u64> d_tw_fwd;            // [T][n][2]
  DevBuf<u64> d_tw_inv;            // [T][n][2]  inverse twiddles; the level-1 entry is pre-scaled
  DevBuf<u64> d_scale;             // [T][8]     Shoup pairs of mhatInv, the level-1 inverse twiddle times mhatInv, and both times 2^64 (plan.cpp),
                                   // then [T][4]: both times 4 2^64 (the fused poly-mul's truncated route)
  // the same three tables as 32-bit Shoup pairs (w, floor(w*2^32/q)) when every q_t < 2^31
  DevBuf<uint32_t> d_tw_fwd32, d_tw_inv32, d_scale32;
  int arith32 = 0;                 // 4: every q_t < 2^27; 2: < 2^30; 3: < 2^31; 0: no 32-bit tables
};

// One dense matrix of a prime above 13 as the dense Z_q stages read it (zqdense.hip; plans created with
// LOLHIP_ROUTE_DENSE_ZQ only): every stage of any program whose mat_off is `mat_off` takes these copies.
//   mt_off  offset (u64 units, per component, into host_zq_mt) of the transposed word matrix [d][d], residues in [0, q)
//   pl_off  offset (bytes, per component, into host_zq_planes) of the first of W int8 limb planes [dp][dp], dp = d
//           rounded up to a multiple of 32, zero padded: sum_w 256^w plane_w = the centred residue; -1: no planes
struct ZqDenseMat { int32_t mat_off, d, dp, mt_off; int64_t pl_off; };
// the stages the dense route runs as matrix products: a DFT_p / CRT_p / CRT_p^-1 of a prime above 13
inline bool zq_dense_stage(const Stage& s) {
  return (s.kind == ST_DFTP || s.kind == ST_CRTP || s.kind == ST_CRTPINV) && s.p > 13;
}

// the stages the scan route runs as prefix sums, totals and neighbour differences (zqscan.hip; plans created with
// LOLHIP_ROUTE_SCAN_ZQ): L, L^-1, mulG and divG of one prime
inline bool zq_scan_stage(const Stage& s) { return s.kind >= ST_L && s.kind <= ST_GINVDEC; }

// dense complex stages at primes above 13 (plans created with LOLHIP_PLAN_DENSE_CPLX; floatpath.hip k_cplx_dense)
constexpr int CPLX_DENSE_MAX_P = 1021;              // 84 MB of matrix forms for both directions at the cap
constexpr int CPLX_MAX_STAGES = 12;                 // two route bits per stage above the count in launch_cplx's word
constexpr size_t CPLX_LDS_BUDGET = 152 * 1024;      // dynamic LDS of one workgroup of k_cplx_dense
// The least vector length and the least number of columns in an LDS tile at which a stage takes the matrix cores: one
// whole 16 x 16 output tile.  Measured: ahead of the vector ALU at every d from 16 to 256 where the
// tile holds 16 columns, behind it at m = 797 where it holds 5.
constexpr int CPLX_MFMA_MIN_D = 16;
constexpr int CPLX_MFMA_MIN_COLS = 16;

struct Plan {
  std::vector<PP> pps;
  int T = 0;
  i64 m = 0, n = 0;
  std::vector<u64> qs;
  bool has_crt = false;            // every q_t prime with m | q_t - 1 (or caller-supplied roots)
  bool device = false;             // device tables uploaded

  // host tables (the reference's marshalled arguments)
  std::vector<std::vector<u64>> omega_pp;   // [k][t]   omega_{pp_k} mod q_t
  std::vector<std::vector<i64>> ru, ruinv;  // [k][pp_k*T] interleaved, tensor.h:91
  std::vector<i64> mhatinv;                 // [T]
  std::vector<i64> gcrt, ginvcrt;           // [n*T] AoS
  std::vector<u64> oddrad_inv;              // [T], 0 when not invertible
  bool has_ginvcrt = false;                 // every odd p | m invertible mod every q_t
  std::vector<u64> host_consts;             // [T][consts_per_comp] generic-path constant pool
  // lift from Z_q0 x ... x Z_q(T-1) to the integers (decrypt.hip k_lift, mixed-radix / Garner form), [T + T*T + T]:
  //   pinv[i]        (q_0 ... q_(i-1))^-1 mod q_i            (1 for i = 0)
  //   qmod[i*T + j]  q_j mod q_i
  //   half[i]        digit i of floor((Q-1)/2) in the mixed radix (q_0, q_1, ...), Q = prod q_t
  // lift_ok: the moduli are pairwise coprime (every pinv exists)
  std::vector<u64> lift_consts;
  bool lift_ok = false;

  // device tables: each owns its allocation (devmem.h), so a Plan cannot be copied and frees them when it is deleted
  DevBuf<ModCtx> d_mod;                     // [T]
  DevBuf<u64> d_consts;                     // generic-path constant pool, [T][consts_per_comp]
  DevBuf<u64> d_consts_mont;                // the same pool times 2^64 mod q_t (every q_t odd): Montgomery class of mixed.hip
  DevBuf<uint32_t> d_consts32;              // 32-bit copy of the pool the 32-bit classes of the vector interpreter read (class 2: the Montgomery one)
  int consts_per_comp = 0;
  StageProgram prog_crt, prog_crtinv, prog_l, prog_linv, prog_gpow, prog_gdec, prog_ginvpow, prog_ginvdec;
  // m = 2^e * odd, 5 <= e <= 15: the 2-power tensor factor is innermost (tensor.h:46-73), i.e. it
  // acts on contiguous blocks of 2^(e-1) coefficients — a batch of B*n/2^(e-1) short transforms
  // for the m = 2^k kernels; these programs hold only the odd primes' stages (the inverse one
  // without mhat^-1, which the 2-power inverse kernel folds in).
  bool pow2_part = false;
  StageProgram prog_crt_odd, prog_crtinv_odd;
  // m = 2^e * odd, e >= 2, in ONE launch of the vector interpreter: ST_POW2F/ST_POW2I tiles for the
  // 2-power factor followed / preceded by the odd primes' stages.  This is what makes the poly-mul of the
  // reference's own parameter sets (64*27, 64*81, 64*9*25, 128*7*13 ...) a fused 3-pass kernel.
  bool fused2 = false;
  StageProgram prog_crt_fused, prog_crtinv_fused;
  // classes 2 / 4 of the vector interpreter: prime powers of small totient as ONE dense stage each (plan.cpp
  // merge_stages).  Totients up to 13 (3^2) run in every kernel: prog_crt_fused / prog_crtinv_fused are merged
  // in place, prog_crt_mg / prog_crtinv_mg are the merged copies of prog_crt / prog_crtinv (empty when nothing
  // merges).  Vector lengths 18 and 20 (3^3, 5^2), 8 (3 (x) 5 as one Kronecker stage) and 9 (the DFT_9 tail of 3^e,
  // e >= 4) need the BIG kernels (mixed_impl.h): the *_big programs, empty when they would equal the others; lone
  // transforms and the fused poly-mul take them, the fused key switch at <= 12 coefficients per thread.
  StageProgram prog_crt_mg, prog_crtinv_mg, prog_crt_mg_big, prog_crtinv_mg_big, prog_crt_fused_big, prog_crtinv_fused_big;
  DevBuf<i64> d_gcrt;                       // [n*T]
  DevBuf<u64> d_lift;                       // lift_consts
  DevBuf<i64> d_ginvcrt;                    // [n*T]
  Pow2Tables pow2;
  bool is_pow2 = false;
  int device_id = -1;                       // HIP device the tables were uploaded to
  int mixed_cls = 0;                        // arithmetic/storage class of the vector interpreter (mixed.hip): 0-3, 4 = 2 with lazy dense stages
  // floating-point side (floatpath.hip): the CRT stage lists over C — a second
  // constant pool, (re, im) interleaved, same offsets as host_consts — and the real maps of
  // tensorGaussianDec
  std::vector<double> host_cconsts, host_rconsts;
  DevBuf<double> d_cconsts, d_rconsts;
  StageProgram prog_gauss;
  // one predicate per family (one LDS-resident polynomial each).  gauss_route: 0 refused; 1 n <= 8192 and register stages only (every odd prime <= 13); 2 n <= 8192, the
  // plan was created with LOLHIP_PLAN_DENSE_GAUSS and an odd prime (below 2^15) takes the dense stage: a prime above
  // 13, or every odd prime under the GAUSS_DENSE switch.  A function of (pps, flags, switch), so host-only plans have it.
  // gauss_word is launch_gauss's stage word over prog_gauss (kernels.h), as cplx_word below.
  uint32_t flags = 0;                       // LOLHIP_PLAN_* of lolhip_plan_create_flags
  // dense Z_q stages at primes above 13 (lolhip_plan_create_routes, LOLHIP_ROUTE_DENSE_ZQ).  Built by plan_build_host for
  // opted-in plans with n <= 8192 only; empty otherwise.  zq_W: limbs of the matrix-core form (2..4), 0 when a modulus
  // is too wide for it.  zq_fold: how many products of two residues a 64-bit accumulator that starts below q takes
  // before it has to be folded (every modulus below 2^32), 0 otherwise.
  uint32_t routes = 0;
  std::vector<ZqDenseMat> zq_mats;
  std::vector<u64> host_zq_mt;              // [T][zq_mt_per_comp]
  std::vector<int8_t> host_zq_planes;       // [T][zq_pl_per_comp]
  i64 zq_mt_per_comp = 0, zq_pl_per_comp = 0;
  int zq_W = 0, zq_fold = 0;
  DevBuf<u64> d_zq_mt;
  DevBuf<int8_t> d_zq_planes;
  int gauss_route = 0, gauss_word = 0;
  // crtC / crtInvC (floatpath.hip).  cplx_route: 0 refused; 1 n <= 8192 and every prime <= 13: k_cplx, register stages
  // only; 2 the plan was created with LOLHIP_PLAN_DENSE_CPLX and at least one stage is dense (a DFT_p, CRT_p or CRT_p^-1 of a prime above 13): every
  // prime <= CPLX_DENSE_MAX_P, both programs <= CPLX_MAX_STAGES stages and nbuf * 16 n <= CPLX_LDS_BUDGET bytes, nbuf = 2
  // when a dense stage is followed by another stage (LDS ping-pong), else 1 (the last stage writes the slab).  A function
  // of (pps, flags, CPLX_DENSE / CPLX_DENSE_VALU at creation), so host-only plans have it.  Route 2 only: prog_crtc[dir]
  // is the copy of prog_crt / prog_crtinv k_cplx_dense reads - a dense stage's wp_off is the offset (complex units) of
  // the transposed matrix [c][row] in the complex pool, pad[0] the offset (doubles) of its planes M_re, M_im, -M_im,
  // each [d rounded up to 16][d rounded up to 4], zero padded; the forms are appended to host_cconsts (row-major there,
  // tile by tile in lane order on the device: plan_upload) - and cplx_word[dir] is launch_cplx's stage word (kernels.h).
  int cplx_route = 0;
  int cplx_word[2] = {0, 0};
  StageProgram prog_crtc[2];
  struct CplxDenseMat { int32_t mat_off, d; int64_t mt_off, pl_off; };     // mt_off: complex units; pl_off: doubles
  std::vector<CplxDenseMat> cplx_mats;
  // Nothing in a plan is written after plan_upload(): per-call workspaces (the operand copy of the
  // unfused poly-mul, the HBM ping-pong ring of polynomials too large for LDS) are stream-ordered
  // allocations made by the call that needs them, so host threads and streams can share a plan.
  bool needs_scratch = false;               // 2 * n * 8 B exceeds the LDS ping-pong budget
};

// ring-extension plan for m | m'
struct ExtPlan {
  const Plan* lo = nullptr;    // index m
  const Plan* hi = nullptr;    // index m'
  ExtTables host;
  DevBuf<int32_t> d_twace_powdec, d_ext_crt, d_embed_pow, d_embed_dec, d_embed_crt, d_coeffs;
  std::vector<i64> tweak;      // [n'*T] AoS, twaceCRT's tweak vector (Extension.hs:110-125)
  DevBuf<i64> d_tweak;
};

// plan.cpp
int plan_build_host(Plan& P, const std::vector<PP>& pps, const std::vector<u64>& qs,
                    const u64* omega_pp /* [npp*T] or null */, const i64* mhatinv /* [T] or null */, uint32_t flags = 0, uint32_t routes = 0);
int plan_upload(Plan& P);

// A/B switches of the launch paths (development and tests): read ONCE from the environment
// (LOLHIP_<NAME>) into atomics; tests flip them through lolhip_debug_set, never through setenv
// (getenv racing with setenv is undefined behaviour, and plans are used from concurrent threads).
enum Switch { SW_GENERIC_SCALAR, SW_NO_FUSED2, SW_NO_POW2_PART, SW_POLYMUL_UNFUSED, SW_KEYSWITCH_UNFUSED, SW_NO_T1, SW_NO_PIPE, SW_FORCE_PIPE, SW_NO_OWN_DIAG, SW_NO_MERGE, SW_NO_LAZY, SW_NO_KRON, SW_NO_TRUNC, SW_ELT_GLOBAL, SW_LPRF_VALU, SW_RLWE_RING_UNFUSED, SW_GAUSS_DENSE, SW_ZQ_DENSE_VALU, SW_ZQ_DENSE_MFMA, SW_CPLX_DENSE, SW_CPLX_DENSE_VALU, SW_ZQ_SCAN, SW_COUNT };
bool sw(Switch which);
inline bool pow2_no_t1() { return sw(SW_NO_T1); }

}  // namespace lolhip
