/*
 * include/lolhip.h — C ABI of liblolhip.so, the MI355X-native backend for the
 * Z_q hot path of Lol's `Tensor` class.
 *
 * Two groups of entry points:
 *
 *  (A) DROP-IN SYMBOLS: the nine `extern "C"` functions lol-cpp exports for Z_q and
 *      that lol-cpp's Haskell shim binds with `foreign import ccall unsafe`
 *      (lol-cpp/Crypto/Lol/Cyclotomic/Tensor/CPP/Backend.hs:304-337).  Same names,
 *      same argument order and meaning, host pointers, in place, one polynomial
 *      per call — so the existing `CT` shim links against liblolhip unchanged.
 *      `totm` is declared int64_t because that is what Haskell passes
 *      (Backend.hs:157; the C++ declares int32 hDim_t, types.h:22).
 *
 *  (B) BATCHED PLAN API: what a `lol-hip` backend binds (INTEGRATION.md shows the
 *      Haskell stubs).  A plan is built once per (prime powers, moduli); data
 *      stays in HBM; every call takes a leading batch dimension B.
 *
 * Data layout everywhere (reference: tensor.h:69, mul.cpp:21, Backend.hs:134-149):
 *   coefficient j of RNS component t of polynomial b is  y[(b*n + j)*T + t],
 *   int64, n = totient(m), T = tupSize.  Inputs may be in (-q_t, q_t); outputs are
 *   always canonical in [0, q_t) (zq.cpp:57-68).
 *
 * All functions are re-entrant (no global modulus, cf. types.h:59): any number of host threads may
 * call into one plan concurrently, on the same or on different streams; per-call workspaces are
 * stream-ordered allocations or caller-provided.  A plan belongs to the HIP device that was
 * current when it was created; calling it with another device current returns LOLHIP_ERR_DEVICE.
 * Nothing calls exit() (cf. ASSERT, types.h:36-41): errors come back as status codes.
 * There is NO CPU fallback: without a usable GPU every compute entry point
 * returns LOLHIP_ERR_NO_DEVICE.
 */
#ifndef LOLHIP_H
#define LOLHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOLHIP_API __attribute__((visibility("default")))

/* == PrimeExponent (types.h:27-31) == Haskell CPP = (Int16, Int16) (Backend.hs:78) */
typedef struct { int16_t prime; int16_t exponent; } lolhip_pp;

enum {
  LOLHIP_OK = 0,
  LOLHIP_ERR_INVALID = -1,      /* malformed prime-power list / sizes                      */
  LOLHIP_ERR_MODULUS = -2,      /* modulus outside [2, 2^62) or required inverse missing  */
  LOLHIP_ERR_NO_CRT = -3,       /* no CRT basis mod some q_t (q not prime or m !| q-1)    */
  LOLHIP_ERR_ROOT = -4,         /* caller-supplied root of unity has the wrong order      */
  LOLHIP_ERR_NO_DEVICE = -5,    /* no HIP device: compute entry points refuse to run      */
  LOLHIP_ERR_HIP = -6,          /* HIP runtime error                                      */
  LOLHIP_ERR_NOT_DIVISIBLE = -7,/* divG: oddRad(m) not invertible mod some q_t            */
  LOLHIP_ERR_DEVICE = -8        /* the calling thread's current HIP device is not the one the plan's tables live on */
};

/* ------------------------------------------------------------------------- */
/* (A) drop-in symbols                                                         */
/* ------------------------------------------------------------------------- */

/* replaces crt.cpp:562-566.  ru[k] = pp_k*tupSize residues, ru[k][i*tupSize+t] =
 * omega_{pp_k,t}^i (CPP.hs:422-432); the roots the caller chose are honoured. */
LOLHIP_API void tensorCRTRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr,
                            int16_t sizeOfPE, int64_t **ru, int64_t *qs);
/* replaces crt.cpp:569-581 (takes inverse roots and mhat^-1 per component) */
LOLHIP_API void tensorCRTInvRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr,
                               int16_t sizeOfPE, int64_t **ruinv, int64_t *mhatInv, int64_t *qs);
/* replaces mul.cpp:27-30: a = zipWith (*) a b */
LOLHIP_API void mulRq(int16_t tupSize, int64_t *a, int64_t *b, int64_t totm, int64_t *qs);
/* replace l.cpp:109-115 / 150-156 */
LOLHIP_API void tensorLRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr, int16_t sizeOfPE, int64_t *qs);
LOLHIP_API void tensorLInvRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr, int16_t sizeOfPE, int64_t *qs);
/* replace g.cpp:130-134 / 146-150 */
LOLHIP_API void tensorGPowRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr, int16_t sizeOfPE, int64_t *qs);
LOLHIP_API void tensorGDecRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr, int16_t sizeOfPE, int64_t *qs);
/* replace g.cpp:186-207 / 239-260: return 1 on success, 0 on failure (CPP.hs:309-323).
 * Unlike the reference, y is left untouched when 0 is returned. */
LOLHIP_API int16_t tensorGInvPowRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr, int16_t sizeOfPE, int64_t *qs);
LOLHIP_API int16_t tensorGInvDecRq(int16_t tupSize, int64_t *y, int64_t totm, lolhip_pp *peArr, int16_t sizeOfPE, int64_t *qs);
/* status of the last drop-in call on this thread (the reference's signatures are void) */
LOLHIP_API int lolhip_last_status(void);

/* ------------------------------------------------------------------------- */
/* (B) batched plan API                                                        */
/* ------------------------------------------------------------------------- */

typedef struct lolhip_plan lolhip_plan;
typedef struct lolhip_ext lolhip_ext;

/* Build the plan for index m = prod pps (ascending primes, as ppsFact does,
 * FactoredDefs.hs:360-361) and moduli qs[0..T).  Roots follow Lol's rule: omega_m =
 * g0^((q-1)/m), g0 the smallest generator of Z_q^* (ZqBasic.hs:144-165).  A plan
 * without a CRT basis is still valid for L/G/mul/twacePowDec/embedPow/embedDec.
 * `host_only != 0` skips the device upload (table inspection on a machine
 * without a GPU; compute calls then fail with LOLHIP_ERR_NO_DEVICE). */
LOLHIP_API int lolhip_plan_create(const lolhip_pp *pps, int npps, const int64_t *qs, int T,
                                  int host_only, lolhip_plan **out);
/* Same, with caller-chosen roots: omega_pp[k*T+t] = primitive pp_k-th root mod q_t,
 * and mhatinv[T] (either may be NULL for the default rule). */
LOLHIP_API int lolhip_plan_create_roots(const lolhip_pp *pps, int npps, const int64_t *qs, int T,
                                        const int64_t *omega_pp, const int64_t *mhatinv,
                                        int host_only, lolhip_plan **out);
/* lolhip_plan_create with options.  flags = 0 is lolhip_plan_create exactly; a bit that is not defined below answers
 * LOLHIP_ERR_INVALID.
 *   LOLHIP_PLAN_DENSE_GAUSS  the Gaussian map (lolhip_gaussian_dec_batch, and through it every sampler: encrypt,
 *       errorRounded / genSK, key-switch and tunnel hints, the Cont and Disc instances of RLWE, RingRLWE and the
 *       challenge entries) takes any index with n <= 8192 whose primes are below 2^15: an odd prime above 13 runs as
 *       a dense stage (a batched FP64 matrix product out of a transposed copy of its (p-1) x (p-1) matrix, which only
 *       such a plan builds), primes up to 13 keep their register stage.  Same summation order, so an index both
 *       routes take gives the same bits on either.  The 2-power rule of the samplers and the limit of crtc / crtinvc
 *       are unchanged. */
#define LOLHIP_PLAN_DENSE_GAUSS 1u
LOLHIP_API int lolhip_plan_create_flags(const lolhip_pp *pps, int npps, const int64_t *qs, int T,
                                        int host_only, uint32_t flags, lolhip_plan **out);
/* How lolhip_gaussian_dec_batch runs on this plan: 0 refused (LOLHIP_ERR_INVALID), 1 register stages only, 2 with a
 * dense stage.  A function of the prime powers and the flags (and the GAUSS_DENSE debug switch at creation, which
 * makes every odd prime of an opted-in plan dense), so host-only plans answer it too; 0 for a null plan. */
LOLHIP_API int lolhip_plan_gauss_route(const lolhip_plan *p);
/* The real matrix of tensorGaussianDec for prime power k of the plan (inspection, tests): row-major
 * (p-1) x (p-1) entries 2 c(row * col mod p) (transposed == 0), or the transposed copy the dense stage reads
 * (transposed != 0; empty unless that prime takes the dense stage).  Copies min(len, available) doubles and returns
 * the available count; 0 for p = 2 or a k out of range. */
LOLHIP_API int64_t lolhip_plan_gauss_table(const lolhip_plan *p, int k, int transposed, double *out, int64_t len);
/* lolhip_plan_create_flags with a route word.  A *flag* widens what a plan accepts; a *route* chooses among kernels
 * that give the same bits, so a plan created with a route answers every call exactly as the plan without it does.
 * routes = 0 is lolhip_plan_create_flags exactly; a bit that is not defined below answers LOLHIP_ERR_INVALID.
 *   LOLHIP_ROUTE_DENSE_ZQ  the Z_q stage programs (crt, crtInv and what is composed of them: the poly-mul, RingMul,
 *       the RLWE instances and challenges) run the stages of a prime above 13 as batched dense products out of an LDS
 *       tile of polynomials instead of one scalar dot product per output element.  Taken when n <= 8192 and the
 *       program about to be launched holds such a stage and at most 24 stages in all (every index of the reference's
 *       range is far below that; a longer program keeps the scalar interpreter); every other launch of the plan is what
 *       it was.  The cost is memory: per component and per such matrix the plan holds, on the host and on the device, a
 *       transposed copy (8 d^2 bytes beside the 8 d^2 it had) and, where the moduli fit the matrix cores, W <= 4 int8
 *       limb planes (W d'^2 bytes, d' = d rounded up to 32) - 15 MB per component for both directions at m = 797, about
 *       1.6 GB at a prime index near 8192 (lolhip_plan_zq_table reads them back).
 *   LOLHIP_ROUTE_SCAN_ZQ  (lolhip_plan_create_opts only; lolhip_plan_create_routes refuses the bit, and the value 2u is
 *       not defined)  the six prime ops over Z_q - lolhip_l_batch, lolhip_linv_batch, lolhip_mulgpow_batch,
 *       lolhip_mulgdec_batch, lolhip_divgpow_batch, lolhip_divgdec_batch and every pipeline that runs those stage
 *       programs (the challenges' and RLWE instances' basis changes, encrypt, decrypt, hints, modSwitch, ...) - run the
 *       stages of a prime above 13 as prefix sums, totals and neighbour differences on an LDS tile of polynomials
 *       (k_zq_scan: O(log) or O(1) modular additions per word) where the scalar interpreter spends up to p - 1 per
 *       output.  Modular addition is associative and exact: the same residues.  Taken when n <= 8192, the program about
 *       to be launched holds an L / L^-1 / mulG / divG stage of a prime above 13, nothing but such stages and diagonals,
 *       at most 24 stages in all, and would go to the scalar interpreter; every other launch of the plan is what it was
 *       (lolhip_plan_scan_route answers per op).  Needs no CRT basis, no tables and no plan memory. */
#define LOLHIP_ROUTE_DENSE_ZQ 1u
#define LOLHIP_ROUTE_SCAN_ZQ 4u
LOLHIP_API int lolhip_plan_create_routes(const lolhip_pp *pps, int npps, const int64_t *qs, int T, int host_only,
                                         uint32_t flags, uint32_t routes, lolhip_plan **out);
/* Which kernel a Z_q transform of this plan launches.  what: 0 a lone crt, 1 a lone crtInv, 2 the poly-mul.
 * Returns 0 for the launches of a plan without LOLHIP_ROUTE_DENSE_ZQ (whatever they are), 1 for the dense route on the
 * vector ALU, 2 for the dense route on the matrix cores.  For what = 2 a value >= 1 means ONE launch; 0 means the
 * poly-mul is composed of lone transforms, which may themselves be dense.  A function of the prime powers, the
 * moduli, the route word and the debug switches (ZQ_DENSE_VALU, ZQ_DENSE_MFMA, GENERIC_SCALAR) only, so host-only
 * plans answer it; 0 for a null plan.  Route 2 needs every modulus of the plan to fit W <= 4 balanced base-256 limbs
 * after centring (floor(q/2) <= 127 (256^W - 1) / 255: q <= 65279, 16711423, 4278124287 for W = 2, 3, 4; one W per
 * plan, the largest of its components) and a dense vector of at least 48 elements in the program: the vector ALU
 * measured faster at 42 and below, the matrix cores at 52 and above.  The poly-mul (what = 2) takes one
 * launch - both operands side by side in the LDS tile, the forward program over both, the pointwise product and the
 * inverse program on the first; c may alias a or b and a may equal b - when the stage programs alone make the transform
 * (no 2^e part, e >= 5, with kernels of its own), POLYMUL_UNFUSED is off, both programs take the dense route (route 2 only
 * if both do), 4 n words fit 152 KiB of LDS (every n <= 8192 at 4-byte words, n <= 4864 at 8-byte words), and a 64 KiB
 * tile leaves the inverse program, which runs on half of it, a whole register tile of columns (32 on the matrix cores,
 * 8 / 4 on the vector ALU at 4- / 8-byte words); below that the composed form measured faster. */
LOLHIP_API int lolhip_plan_zq_route(const lolhip_plan *p, int what);
/* Whether the scan kernel (LOLHIP_ROUTE_SCAN_ZQ) runs the stage program of prime op `op`, LOLHIP_OP_L ...
 * LOLHIP_OP_DIVGDEC: 1 if so, 0 otherwise - a null plan, an op out of that range, a plan that has not opted in, n > 8192,
 * an index whose primes are all <= 13 (the vector interpreter's, or a 2-power's).  A function of the prime powers, the
 * moduli, the route word and two debug switches read at launch (GENERIC_SCALAR: 0 everywhere; ZQ_SCAN: an opted-in plan
 * takes the scan kernel at primes up to 13 as well, also where the vector interpreter would run; GENERIC_SCALAR wins),
 * so host-only plans answer it.  divG's LOLHIP_ERR_NOT_DIVISIBLE is decided before any launch whatever the route. */
LOLHIP_API int lolhip_plan_scan_route(const lolhip_plan *p, int op);
/* A dense stage's matrix as the device reads it (inspection, tests).  inverse: the lone crtInv's program, else the lone
 * crt's; stage: index into that program (lolhip_plan_table 10 / 11); t: component.  limb = -1: the transposed word
 * matrix of the vector-ALU route, d * d residues in [0, q_t), entry [c][row].  limb >= 0: that int8 limb plane of the
 * matrix-core route, one int64 per entry, padded shape included.  Copies min(cap, available) values and returns the
 * available count; 0 for a stage that is not dense on this plan, or a plane this plan does not hold. */
LOLHIP_API int64_t lolhip_plan_zq_table(const lolhip_plan *p, int inverse, int stage, int t, int limb, int64_t *out,
                                        int64_t cap);
/* The creator with an options block: what lolhip_plan_create_routes takes, in a struct that carries its own size, so a
 * later option is a new bit or a new field and not another creator.  size must be sizeof(lolhip_plan_opts); a flag or
 * route bit that is not defined answers LOLHIP_ERR_INVALID.  Without LOLHIP_PLAN_DENSE_CPLX the plan is exactly the one
 * lolhip_plan_create_routes(flags, routes) builds.  Default roots only.
 *   LOLHIP_PLAN_DENSE_CPLX  (this creator only; lolhip_plan_create_flags / _routes refuse the bit)  crtc / crtinvc take
 *       indices with a prime above 13: the stages of such a prime (DFT_p, CRT_p, CRT_p^-1) run as batched dense complex
 *       products out of an LDS tile of polynomials, on the FP64 matrix cores (v_mfma_f64_16x16x4_f64; where the vector has
 *       at least 16 elements and a 64 KiB tile holds at least 16 of them, measured: DESIGN.md 3.4r) or the vector ALU,
 *       in the same launch as the register stages of the primes up to 13.  Accepted: every prime <= 1021, at most 12
 *       stages per program, and 16 n bytes (the one dense stage is the last stage of both programs: 2^e p up to
 *       n = 8192) or 32 n bytes (otherwise: every n <= 4864, so every n <= 4096 and 32 17 19) within 152 KiB of LDS.
 *       Everything else keeps the answer of a default plan.  The cost is memory: per dense matrix a transposed copy and
 *       three real planes, 40 d^2 bytes beside the 16 d^2 it had (84 MB for both directions at p = 1021).  A plan
 *       without the flag launches what it always did. */
typedef struct { uint32_t size; uint32_t flags; uint32_t routes; } lolhip_plan_opts;
#define LOLHIP_PLAN_DENSE_CPLX 2u
LOLHIP_API int lolhip_plan_create_opts(const lolhip_pp *pps, int npps, const int64_t *qs, int T, int host_only,
                                       const lolhip_plan_opts *opts, lolhip_plan **out);
/* How lolhip_crtc_batch / lolhip_crtinvc_batch run on this plan: 0 refused (LOLHIP_ERR_INVALID), 1 register stages only
 * (n <= 8192, every prime <= 13), 2 at least one dense stage (see LOLHIP_PLAN_DENSE_CPLX).  A function of the prime
 * powers, the flag and two debug switches read when the plan is built (CPLX_DENSE: every odd prime of an opted-in plan
 * is dense; CPLX_DENSE_VALU: no stage takes the matrix cores), so host-only plans answer it; 0 for a null plan. */
LOLHIP_API int lolhip_plan_cplx_route(const lolhip_plan *p);
/* A dense stage's matrix in the extra forms the device reads (inspection, tests).  inverse: crtinvc's program, else
 * crtc's; stage: index into it (the stage list is lolhip_plan_table 20 / 21's).  form 0: the transposed copy,
 * d * d complex entries [c][row], (re, im) interleaved: 2 d^2 doubles.  form 1, 2, 3: the planes M_re, M_im, -M_im of
 * the matrix route, row-major [d rounded up to 16][d rounded up to 4], zero padded (the device holds the same planes
 * tile by tile in lane order).  Copies min(cap, available) doubles and returns the available count; 0 for a stage
 * that is not dense on this plan. */
LOLHIP_API int64_t lolhip_plan_cplx_table(const lolhip_plan *p, int inverse, int stage, int form, double *out,
                                          int64_t cap);
LOLHIP_API void lolhip_plan_destroy(lolhip_plan *p);

LOLHIP_API int64_t lolhip_plan_n(const lolhip_plan *p);      /* totient(m) */
LOLHIP_API int64_t lolhip_plan_m(const lolhip_plan *p);
LOLHIP_API int lolhip_plan_T(const lolhip_plan *p);
LOLHIP_API int lolhip_plan_has_crt(const lolhip_plan *p);
/* Host tables exactly as lol-cpp's shim would marshal them.  Each copies min(len,
 * available) int64 values and returns the available count.
 *   which: 0 ru[k] (CPP.hs:422-432)   1 ruInv[k] (CPP.hs:434-442)   2 mhatInv
 *          3 gCRT  4 gInvCRT (CPP.hs:444-454; [n*T] AoS)            5 qs
 *          10 / 11 (inspection, tests): the stage program a lone crt / crtInv of an index that is not a power
 *          of two launches, four values per stage: kind, prime (first level for the 2-power tiles), vector
 *          length (levels for the tiles), stride.  The choice is the launch's own, current A/B switches included: the
 *          one-launch program with 2-power tiles where the vector interpreter takes it, the odd primes' program
 *          where the 2-power factor goes through the m = 2^k kernels, the whole stage program otherwise
 *          13 / 14 (inspection, tests): the forward / inverse program of a poly-mul that runs as one launch of the
 *          vector interpreter, same four values per stage; empty when the poly-mul is composed of lone transforms
 *          20 / 21 (inspection, tests): the stage program of crtc / crtinvc, five values per stage: kind, prime, vector
 *          length, stride and route (0 register stage or diagonal, 1 dense on the vector ALU, 2 dense on the matrix
 *          cores; the launcher's LOLHIP_CPLX_INFO line prints the same); empty when lolhip_plan_cplx_route is 0
 *          12 (inspection, tests): the lift constants of errorTerm / decrypt, [T + T*T + T]: (q_0 ... q_{i-1})^-1
 *          mod q_i (1 for i = 0); q_j mod q_i at [T + i*T + j]; the mixed-radix digits of floor((Q-1)/2),
 *          Q = prod q_t, least significant first                                  */
LOLHIP_API int64_t lolhip_plan_table(const lolhip_plan *p, int which, int k, int64_t *out, int64_t len);

/* smallest prime > lower congruent to 1 mod m (head of goodQs, ZqBasic.hs:71-73) */
LOLHIP_API int64_t lolhip_good_q(int64_t m, int64_t lower);

/* --- device-pointer batch operations (y, a, b, c live in HBM; stream = hipStream_t
 *     or NULL).  In place unless noted.  Return LOLHIP_OK or an error. ------------- */
LOLHIP_API int lolhip_crt_batch   (const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
LOLHIP_API int lolhip_crtinv_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
/* a *= b pointwise (mulRq / zipWithT (*), CPP.hs:257-260) */
LOLHIP_API int lolhip_mul_batch   (const lolhip_plan *p, void *stream, int64_t *a, const int64_t *b, int64_t B);
/* c = crtInv(crt(a) * crt(b)): one cyclotomic ring product per batch item, operands and
 * result in the powerful basis (Cyc (*), Cyc.hs:262-297).  c may alias a or b. */
LOLHIP_API int lolhip_polymul_batch(const lolhip_plan *p, void *stream, int64_t *c, const int64_t *a,
                                    const int64_t *b, int64_t B);
LOLHIP_API int lolhip_l_batch      (const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
LOLHIP_API int lolhip_linv_batch   (const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
LOLHIP_API int lolhip_mulgpow_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
LOLHIP_API int lolhip_mulgdec_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
/* LOLHIP_ERR_NOT_DIVISIBLE (y untouched) iff the reference would return 0 */
LOLHIP_API int lolhip_divgpow_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
LOLHIP_API int lolhip_divgdec_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
/* mulGCRT / divGCRT: pointwise by gCRT / gInvCRT (CPP.hs:230-231) */
LOLHIP_API int lolhip_mulgcrt_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);
LOLHIP_API int lolhip_divgcrt_batch(const lolhip_plan *p, void *stream, int64_t *y, int64_t B);

/* --- floating-point members of the class, float64, tolerance contract:
 *     relative 1e-12 against lol-cpp on the same inputs (integer paths are bit-exact) --------
 * crtc / crtinvc: replace tensorCRTC / tensorCRTInvC (crt.cpp:583-598), the CRT over C with
 *   omega_m = exp(2 pi i / m) that UCyc uses when a modulus has no CRT basis (CRTExt,
 *   UCyc.hs:422-444).  y [B][n] complex doubles, (re, im) interleaved, in place; crtinvc includes
 *   the mhat^-1 scaling.  Works for any plan (the moduli play no role).
 * gaussian_dec: replaces tensorGaussianDec (random.cpp:19-64; caller CPP.hs:376-389): y [B][n]
 *   doubles, on entry iid real Gaussians, on exit the sample in the decoding basis (the caller
 *   draws and scales the Gaussians and rounds the result, as cDispatchGaussian does).
 * Both need n <= 8192 and every prime of m <= 13, else LOLHIP_ERR_INVALID.  On a plan created with
 * LOLHIP_PLAN_DENSE_GAUSS, gaussian_dec takes every prime below 2^15 (n <= 8192 still); on a plan created with
 * LOLHIP_PLAN_DENSE_CPLX (lolhip_plan_create_opts), crtc / crtinvc take primes up to 1021 within the LDS rule stated
 * there (lolhip_plan_cplx_route says which indices). */
LOLHIP_API int lolhip_crtc_batch        (const lolhip_plan *p, void *stream, double *y, int64_t B);
LOLHIP_API int lolhip_crtinvc_batch     (const lolhip_plan *p, void *stream, double *y, int64_t B);
LOLHIP_API int lolhip_gaussian_dec_batch(const lolhip_plan *p, void *stream, double *y, int64_t B);

/* --- ring extension m | m' (twace/embed, Extension.hs:54-129) ------------------- */
LOLHIP_API int lolhip_ext_create(const lolhip_plan *p_m, const lolhip_plan *p_mprime, lolhip_ext **out);
LOLHIP_API void lolhip_ext_destroy(lolhip_ext *x);
/* out-of-place gathers; `lo` arrays are [B][n][T], `hi` arrays [B][n'][T] */
LOLHIP_API int lolhip_twace_powdec_batch(const lolhip_ext *x, void *stream, int64_t *lo_out, const int64_t *hi_in, int64_t B);
LOLHIP_API int lolhip_twace_crt_batch   (const lolhip_ext *x, void *stream, int64_t *lo_out, const int64_t *hi_in, int64_t B);
LOLHIP_API int lolhip_embed_pow_batch   (const lolhip_ext *x, void *stream, int64_t *hi_out, const int64_t *lo_in, int64_t B);
LOLHIP_API int lolhip_embed_dec_batch   (const lolhip_ext *x, void *stream, int64_t *hi_out, const int64_t *lo_in, int64_t B);
LOLHIP_API int lolhip_embed_crt_batch   (const lolhip_ext *x, void *stream, int64_t *hi_out, const int64_t *lo_in, int64_t B);
/* coeffs (class Tensor, Tensor.hs:174; CPP/Extension.hs:90-93): the phi(m')/phi(m) coefficient
 * vectors of each O_m' element with respect to the relative powerful (or decoding) basis,
 * lo_out [phi(m')/phi(m)][B][n][T] <- hi_in [B][n'][T].  Vector i1 pairs with the relative basis
 * element whose powerful-basis representation is the unit vector at index table5[i1*n]
 * (powBasisPow, Tensor.hs:177: sum_i1 embed(coeffs_i1 x) * b_i1 = x, CycTests.hs:71-76). */
LOLHIP_API int lolhip_coeffs_batch      (const lolhip_ext *x, void *stream, int64_t *lo_out, const int64_t *hi_in, int64_t B);
/* evalLin (lol Linear.hs:75-79): apply the E-linear function R -> S given by its values
 * ys_i in S on the relative decoding basis of R/E:
 *     out = sum_i ys_i * embed (coeffsDec_i r)
 * x_er: extension E in R, x_es: extension E in S (same plan for E in both).  r_dec [B][n_R][T]
 * in the decoding basis of R; ys_crt [n_R/n_E][n_S][T] in the CRT basis of S (what linearDec
 * stores, Linear.hs:68-72); out [B][n_S][T] in the CRT basis of S.  work: device scratch of
 * (n_R/n_E) * B * (n_E + n_S) * T int64.  A composition of the kernels above: coeffs gather,
 * embedDec, l, crt over all (n_R/n_E)*B polynomials at once, knapsack. */
LOLHIP_API int lolhip_evallin_batch(const lolhip_ext *x_er, const lolhip_ext *x_es, void *stream,
                                    const int64_t *r_dec, const int64_t *ys_crt, int64_t *out,
                                    int64_t *work, int64_t B);
/* tunnel (lol-apps SymmSHE.hs:549-570), the body after `toMSD . absorbGFactors`: for a linear
 * ciphertext [c0, c1] over R' (c0_dec in the decoding basis, c1_pow in the powerful basis, both
 * [B][n_R][T]),
 *     c0' = evalLin f c0;  c1s = coeffsPow c1 :: [E'];  c1' = sum_i switch hints_i (embed c1s_i)
 *     out = const c0' + c1'      [2][B][n_S][T], CRT basis of S'
 * ys_crt as for lolhip_evallin_batch; hints [n_R/n_E][L][2][n_S][T] (one KSHint per relative
 * powerful-basis element, CRT basis, L = lolhip_decompose_len of the S' plan); base as for
 * lolhip_keyswitch_batch.  work: lolhip_tunnel_work_len(...) int64 of device scratch. */
LOLHIP_API int64_t lolhip_tunnel_work_len(const lolhip_ext *x_er, const lolhip_ext *x_es, int64_t base, int64_t B);
LOLHIP_API int lolhip_tunnel_batch(const lolhip_ext *x_er, const lolhip_ext *x_es, void *stream,
                                   const int64_t *c0_dec, const int64_t *c1_pow, const int64_t *ys_crt,
                                   const int64_t *hints, int64_t base, int64_t *out, int64_t *work, int64_t B);
/* host index tables: which 0 extIndicesPowDec[n] 1 extIndicesCRT[n'] 2 embedPow[n'] (-1 = zero)
 * 3 embedDec[n'] (-1 zero, bit 30 = negate) 4 baseIndicesCRT[n'] (Tensor.hs:426-468)
 * 5 extIndicesCoeffs[n'/n][n] flattened (Tensor.hs:472-477)
 * 6 powBasisPow[n'/n] (CPP/Extension.hs:131-141): element i of the relative powerful basis of O_m'/O_m is the
 *   powerful-basis unit vector at index powBasisPow[i] (= table 5 at [i][0]); sum_i embedPow(coeffs_i x) b_i = x */
LOLHIP_API int64_t lolhip_ext_table(const lolhip_ext *x, int which, int32_t *out, int64_t len);

/* --- ring-level pipelines of SymmSHE, device pointers -----------
 * In the reference these are Haskell compositions of the Tensor methods above on one
 * ring element at a time; here each is one or two passes over a batch slab.  All slabs
 * are [.][B][n][T] int64, component t innermost.  Up to 16 RNS components.              */

/* Coefficients of  mulG <$> (c * d)  for two linear ciphertexts c = c0 + c1 s,
 * d = d0 + d1 s, every operand in the CRT basis (lol-apps SymmSHE.hs:444-449; mulG in the
 * CRT basis is the pointwise product with gCRT, CPP.hs:230):
 *   e0 = g c0 d0,  e1 = g (c0 d1 + c1 d0),  e2 = g c1 d1.
 * One pass: 4 reads, 3 writes.  Outputs may alias inputs. */
LOLHIP_API int lolhip_ctmul_crt_batch(const lolhip_plan *p, void *stream, const int64_t *c0, const int64_t *c1,
                                      const int64_t *d0, const int64_t *d1, int64_t *e0, int64_t *e1,
                                      int64_t *e2, int64_t B);

/* Gadget decomposition (Decompose gad (Cyc t m zq), Cyc.hs:592-604): base 0 = TrivGad
 * (ZqBasic.hs:227-232: one digit per component, its centred lift), base b >= 2 = BaseBGad b
 * (ZqBasic.hs:258-264: gadlen(b, q_t) centred base-b digits, Numeric.hs:202-205,227-234);
 * product rings concatenate, first component first (Gadget.hs:96-101).
 * lolhip_decompose_len: number of digits L (negative status on error).
 * lolhip_gadget: the gadget vector as [L][T] residues (b^k in its own component, zero
 *   elsewhere; Gadget.hs:92-94), host array of at least L*T entries; returns L.
 * lolhip_decompose_batch: c in the powerful basis [B][n][T] -> digits [L][B][n][T], every
 *   integer digit polynomial already reduced into all T components (`fmap reduce`,
 *   SymmSHE.hs:314). */
LOLHIP_API int lolhip_decompose_len(const lolhip_plan *p, int64_t base);
LOLHIP_API int lolhip_gadget(const lolhip_plan *p, int64_t base, int64_t *out, int64_t cap);
LOLHIP_API int lolhip_decompose_batch(const lolhip_plan *p, void *stream, const int64_t *c_pow, int64_t base,
                                      int64_t *digits, int64_t B);

/* knapsack (SymmSHE.hs:302-304): out_k = addend_k + sum_j xs_j * hint_jk, CRT basis.
 * xs [L][B][n][T]; hint [L][K][n][T], shared by the whole batch (K = 1..3 coefficients
 * of the hint polynomials); addend [K][B][n][T] or NULL; out [K][B][n][T] (may alias addend). */
LOLHIP_API int lolhip_knapsack_batch(const lolhip_plan *p, void *stream, const int64_t *xs_crt, int L,
                                     const int64_t *hint, int K, const int64_t *addend, int64_t *out, int64_t B);

/* `switch` (SymmSHE.hs:312-314) and with it keySwitchQuadCirc (:361-371, addend = the CRT
 * forms of c0, c1):  out = addend + knapsack hint (crt (reduce <$> decompose c2)).
 * c2 in the powerful basis [B][n][T]; work: caller-provided device scratch of
 * lolhip_decompose_len * B * n * T int64 (it holds the digit polynomials). */
LOLHIP_API int lolhip_keyswitch_batch(const lolhip_plan *p, void *stream, const int64_t *c2_pow, int64_t base,
                                      const int64_t *hint, int K, const int64_t *addend, int64_t *out,
                                      int64_t *work, int64_t B);

/* RescaleCyc (a,b) -> b (Cyc.hs:529-542): drop the first modulus of the tuple.  With
 * z = lift a coefficient-wise (powerful or decoding basis),
 *   out_s = q_0^-1 (c_s - z)  mod q_s   for s = 1..T-1.
 * c [B][n][T] -> out [B][n][T-1].  LOLHIP_ERR_MODULUS if q_0 is not invertible mod some q_s. */
LOLHIP_API int lolhip_rescale_drop_batch(const lolhip_plan *p, void *stream, const int64_t *c, int64_t *out,
                                         int64_t B);

/* errorTerm / decrypt (lol-apps SymmSHE.hs:153-178; decryptUnrestricted :200-208).
 * cs: ncs ciphertext components c_0..c_{ncs-1}, [ncs][B][n'][T], powerful basis (cs_crt = 0) or
 *     CRT basis (cs_crt = 1), over pq (index m', moduli q_0..q_{T-1}, CRT basis required).
 * s_crt: the secret key reduced into pq, CRT basis, [n'][T], shared by the whole batch.
 * enc: 0 = LSD, 1 = MSD (toLSD first, SymmSHE.hs:214-230; msdToLSD, Prelude.hs:139-140,311-315).
 * p: the plaintext modulus.
 * lolhip_error_term_batch: e_dec [B][n'] int64 = liftCyc Dec (evaluate c s) after toLSD, the centred lift mod
 *   Q = prod q_t of every decoding-basis coefficient ([-(Q-1)/2, (Q-1)/2] for odd Q); a lift that does not fit
 *   int64 is written as INT64_MIN (no status, no synchronisation).
 * lolhip_decrypt_batch: pt_pow [B][n_m] residues in [0, p), powerful basis of R_m, = l' twace (divG^k (reduce_p e))
 *   with e the error term (divGDec, then twacePowDec): l' = l for LSD, l (-Q)^-1 mod p for MSD.  pp: the plan of
 *   index m' over the single modulus p (any p >= 2, no CRT basis needed); x_p: an extension from the plan of
 *   (m, p) to pp, or NULL for m = m'.
 * Status: LOLHIP_ERR_INVALID for ncs < 1, pp not of index m' or not of one modulus, x_p not ending in pp's ring
 *   and modulus, T > 16; LOLHIP_ERR_NO_CRT when pq has no CRT basis; LOLHIP_ERR_MODULUS for MSD with gcd(Q, p) != 1
 *   (or moduli of pq that are not pairwise coprime); LOLHIP_ERR_NOT_DIVISIBLE for k > 0 when divGDec is impossible
 *   mod p.  Every one of these is decided on the host before any launch: e_dec / pt_pow are then not written.
 * work: caller-provided device scratch of lolhip_decrypt_work_len(pq, ncs, B) int64 (re-entrant calls); cs and
 *   s_crt are only read. */
LOLHIP_API int64_t lolhip_decrypt_work_len(const lolhip_plan *pq, int ncs, int64_t B);
LOLHIP_API int lolhip_error_term_batch(const lolhip_plan *pq, void *stream, const int64_t *cs, int ncs,
                                       int cs_crt, const int64_t *s_crt, int enc, int64_t p, int64_t *e_dec,
                                       int64_t *work, int64_t B);
LOLHIP_API int lolhip_decrypt_batch(const lolhip_plan *pq, const lolhip_plan *pp, const lolhip_ext *x_p,
                                    void *stream, const int64_t *cs, int ncs, int cs_crt, const int64_t *s_crt, int enc,
                                    int64_t k, int64_t l, int64_t *pt_pow, int64_t *work, int64_t B);

/* encrypt / genSK (lol-apps SymmSHE.hs:120-146): samplers over the ChaCha20 stream cipher (RFC 8439 §2.3 block function,
 * counter mode), so every sample is a pure function of (key, position) and does not depend on launch shape, stream or how
 * a batch is split.  Stream layout: batch item b of a call with offset ctr uses the nonce (domain, lo32(ctr + b),
 * hi32(ctr + b)) and block counters from 0; domain 0 = the Gaussians of encrypt, 1 = the uniform c1, 2 = errorRounded,
 * 3 / 4 = the Gaussians / uniform c1 of key-switch hints (lolhip_kshint_batch below, where the item is an LWE sample).
 *   Gaussian coefficient j (decoding basis): pair i = j >> 1 from block i >> 2, words w[4(i&3) .. 4(i&3)+3];
 *     a = w0 | w1 << 32, c = w2 | w3 << 32, u1 = ((a >> 11) + 1) 2^-53, u2 = (c >> 11) 2^-53, r = sigma sqrt(-2 ln u1),
 *     g_2i = r cos(2 pi u2), g_2i+1 = r sin(2 pi u2) (basic Box-Muller); for an index that is not a power of two the
 *     map of lolhip_gaussian_dec_batch follows.  sigma = sqrt(v (m'/rad m') / (2 pi)) (tGaussianDec v: scaled
 *     variance), v = svar * (p * p) (in double) for encrypt and svar for errorRounded.
 *   Uniform CRT-basis residue [j][t]: r = j*T + t from block r >> 2, (w0 + 2^32 w1 + 2^64 w2 + 2^96 w3) mod q_t.
 * THE CALLER'S DUTY: never use the same (key, ctr + b) twice for one domain: after a call with batch B, advance ctr by B
 * (a repeated nonce repeats the noise and c1, which gives the secret key away).  A hint call uses B*L items of domains 3
 * and 4 (advance ctr by B*L); its own domains keep hint noise disjoint from genSK's (2) and encrypt's (0, 1) at equal
 * ctr, so one counter may serve all three kinds of call.
 * lolhip_encrypt_batch: cs_out [2][B][n'][T] = (c0, c1) of CT LSD 0 1 [reduce e - c1 s, c1] over pq (index m', CRT
 *   basis required), in the CRT basis (out_crt = 1) or the powerful basis; the two are the same integers up to crtInv.
 *   e = errorCoset (svar) (embed pt): rep_j + p round((g_j - rep_j) / p) per decoding-basis coefficient (half to even),
 *   rep_j the centred ([-p/2, p/2)) decoding-basis coefficient of embed pt mod p.  pt_pow [B][n_m] in (-p, p), powerful
 *   basis of R_m; pp: the plan of index m' over p alone; x_p: an extension from the plan of (m, p) to pp, or NULL for
 *   m = m'.  s_crt [n'][T]: the secret key reduced into pq, CRT basis, shared by the batch.  work:
 *   lolhip_encrypt_work_len(pq, B) int64 of device scratch.
 * lolhip_error_rounded_batch: z_dec [B][n'] = errorRounded svar (genSK's key, SymmSHE.hs:120-122; UCyc.hs:422-429), the
 *   decoding-basis coefficients rounded half to even; the plan supplies the index only.  work is not used (the sampler
 *   runs in place in z_dec) and may be NULL.
 * Limits: T <= 16; n' <= 16384 for m' = 2^k; otherwise the limits of lolhip_gaussian_dec_batch (n' <= 8192, primes
 *   <= 13; primes below 2^15 when the plan of index m' was created with LOLHIP_PLAN_DENSE_GAUSS).
 * Status: LOLHIP_ERR_INVALID for svar <= 0 or not finite, B < 0, pp not of index m' or not of one modulus, x_p not
 *   ending in pp's ring and modulus, T > 16, an index beyond the limits; LOLHIP_ERR_NO_CRT when pq has no CRT basis;
 *   LOLHIP_ERR_MODULUS for p < 2; LOLHIP_ERR_NO_DEVICE on a host-only plan (an index beyond the limits is answered
 *   first, there too: it is a property of the plan).  Every one is decided on the host before any launch: the output is
 *   then not written.  No call synchronises or allocates. */
LOLHIP_API int64_t lolhip_encrypt_work_len(const lolhip_plan *pq, int64_t B);
LOLHIP_API int lolhip_encrypt_batch(const lolhip_plan *pq, const lolhip_plan *pp, const lolhip_ext *x_p, void *stream,
                                    const int64_t *pt_pow, const int64_t *s_crt, double svar, const uint8_t key[32],
                                    uint64_t ctr, int out_crt, int64_t *cs_out, int64_t *work, int64_t B);
LOLHIP_API int lolhip_error_rounded_batch(const lolhip_plan *p, void *stream, double svar, const uint8_t key[32],
                                          uint64_t ctr, int64_t *z_dec, int64_t *work, int64_t B);
/* inspection (tests): the ChaCha20 block function the kernels run, on the host; out[i] = word i of the block */
LOLHIP_API void lolhip_chacha20_block(const uint8_t key[32], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]);

/* key-switch hints (lol-apps SymmSHE.hs:262-296 lweSample / ksHint; ksLinearHint / ksQuadCircHint :330-355 are ksHint
 * with val = s_in and val = s*s; tunnelHint :531-545).  ksHint skout val is L rows over pq, one per gadget entry g_j
 * (the rows of lolhip_gadget, [L][T]; L = lolhip_decompose_len(pq, base)):
 *     hint_j = [ g_j val + c1_j (-s) + reduce e_j ,  c1_j ]      (CRT basis)
 *   e_j = errorRounded svar (svar: skout's scaled variance), a decoding-basis vector taken to the CRT basis by l and
 *   crt; c1_j uniform in the CRT basis.
 * Stream layout: row j of batch item b is LWE sample i = ctr + b*L + j.  Its Gaussians are those of errorRounded at
 *   item i of domain 3 (sigma = sqrt(svar (m'/rad m') / (2 pi)), then the map of lolhip_gaussian_dec_batch for an index
 *   that is not a power of two, rounded half to even); its c1 is the uniform residue sampler at item i of domain 4
 *   (residue r = c*T + t from block r >> 2, as for encrypt).  Advance ctr by B*L after a call.
 * lolhip_kshint_batch: hints_out [B][L][2][n][T] (hints_out + b*L*2*n*T is exactly the [L][K=2][n][T] hint of
 *   lolhip_keyswitch_batch) for vals_crt [B][n][T] in the CRT basis of pq; s_crt [n][T]: skout reduced into pq, CRT
 *   basis, shared by the batch.  work: lolhip_kshint_work_len(pq, base, B) = B*L*n*T int64 (m' = 2^k) or B*L*n*(T+1).
 * lolhip_tunnel_hint_batch: hints_out [rel][L][2][n_S][T] (rel = n_R/n_E; the hints of lolhip_tunnel_batch) with
 *   comps_i = evalLin f' (s_in p_i) for the relative powerful-basis elements p_i of R'/E' (p_i the powerful-basis unit
 *   vector at lolhip_ext_table(x_er, 5)[i*n_E], the pairing of lolhip_tunnel_batch); hint i = ksHint skout comps_i over
 *   the S' plan, items ctr .. ctr + rel*L - 1.  ys_crt [rel][n_S][T]: the linearDec table of f'q that
 *   lolhip_tunnel_batch takes (reduce commutes with the Z-linear evalLin); s_in_crt [n_R][T], s_out_crt [n_S][T]: the
 *   two keys in the CRT bases of R' and S'.  work: lolhip_tunnel_hint_work_len(x_er, x_es, base) int64.
 * Limits: T <= 16 and the sampler's index limits of lolhip_encrypt_batch (for S').
 * Status: LOLHIP_ERR_INVALID for svar <= 0 or not finite, B < 0, an invalid base, T > 16, an index beyond the limits,
 *   extensions that do not share E' and the moduli, NULL pointers; LOLHIP_ERR_NO_CRT when pq (S', R') has no CRT
 *   basis; LOLHIP_ERR_NO_DEVICE on a host-only plan.  Every one is decided on the host before any launch: the output is
 *   then not written.  No call synchronises or allocates. */
LOLHIP_API int64_t lolhip_kshint_work_len(const lolhip_plan *pq, int64_t base, int64_t B);
LOLHIP_API int lolhip_kshint_batch(const lolhip_plan *pq, void *stream, const int64_t *s_crt, const int64_t *vals_crt,
                                   double svar, int64_t base, const uint8_t key[32], uint64_t ctr, int64_t *hints_out,
                                   int64_t *work, int64_t B);
LOLHIP_API int64_t lolhip_tunnel_hint_work_len(const lolhip_ext *x_er, const lolhip_ext *x_es, int64_t base);
LOLHIP_API int lolhip_tunnel_hint_batch(const lolhip_ext *x_er, const lolhip_ext *x_es, void *stream,
                                        const int64_t *ys_crt, const int64_t *s_in_crt, const int64_t *s_out_crt,
                                        double svar, int64_t base, const uint8_t key[32], uint64_t ctr,
                                        int64_t *hints_out, int64_t *work);

/* key-homomorphic ring PRF of [BP14] (lol-apps KeyHomomorphicPRF.hs: buildDecTree, ringPRF'), one modulus q (T = 1).
 * A family is a full binary tree of k leaves (1 <= k <= 62) and two 1 x L row vectors a0, a1 over R_q, L =
 * lolhip_decompose_len(pq, base) (base 0 = TrivGad, b >= 2 = BaseBGad b, as for lolhip_decompose_batch).  For an input x:
 *     A_leaf(x) = a_x (x in {0, 1});   A_(I c l r)(x) = A_l(x >> c_r) * G^-1(A_r(x & (2^c_r - 1)))   (c_r: leaves of r)
 *   G^-1 = decomposeMatrix: column j of the L x L matrix holds the L digits of entry j, decomposed in the powerful basis
 *   and reduced mod q, so A(x)_j = sum_i A_l(..)_i digit_i(A_r(..)_j).  The rightmost leaf reads bit 0 of x.
 *     ringPRF s x = (rescaleDec . (s *)) <$> A_T(x):  y = fst (divModCent (p lift z) q) mod p per decoding-basis
 *   coefficient z of s A_T(x)_j (lift centred; divModCent a q = floor((a + q div 2) / q)).
 * lolhip_khprf_create: tree = the preorder list of leaf counts, 1 for a leaf, a node of count c > 1 followed by its left
 *   and then its right subtree (I 3 L (I 2 L L) = {3,1,2,1,1}); a0_crt, a1_crt: HOST arrays [L][n] in the CRT basis.  On
 *   a device plan it uploads a0, a1 and crt(G^-1(a0)), crt(G^-1(a1)) [L][L][n] each (allocates and synchronises; the
 *   family belongs to the plan's device and must be destroyed before the plan).  A host-only plan makes a family that
 *   only answers work_len.  LOLHIP_ERR_INVALID for a malformed tree, T != 1, an invalid base, NULL pointers;
 *   LOLHIP_ERR_NO_CRT when q has no CRT basis for m — which is the case of the reference's own toy shapes over Zq 8:
 *   those take lolhip_khprf_create_lifted below.
 * lolhip_khprf_work_len: the int64 scratch of both calls below over inputs [x0, x0 + B) (negative status on error).
 *   Node v with c_v leaves and s_v leaves to its right sees (x >> s_v) & (2^c_v - 1), which takes
 *   U_v = min(2^c_v, ((x0 + B - 1) >> s_v) - (x0 >> s_v) + 1) values over the range; each is computed once per call.  The
 *   scratch is sum over internal nodes v (the root included) of U_v L n, plus sum over internal right children r of
 *   L U_r L n (their digits); 0 for B = 0 or a one-leaf tree.
 * lolhip_khprf_eval_batch: out [B][L][n] = A_T(x) for x = x0 .. x0 + B - 1, CRT basis (exact mod q).
 * lolhip_khprf_batch: out [nkeys][B][L][n] = ringPRF s_key x, int64 in [0, p), decoding basis of R_p (lolhip_l_batch on a
 *   plan mod p gives the powerful basis); s_crt [nkeys][n] on the device, CRT basis.  A_T is computed once for all keys.
 * Status: LOLHIP_ERR_INVALID for x0 < 0, B < 0, x0 + B > 2^k, nkeys < 1, NULL pointers; LOLHIP_ERR_MODULUS for p < 2,
 *   p >= q or p q >= 2^63 (the reference computes p lift z in Int64); LOLHIP_ERR_NO_DEVICE on a host-only plan;
 *   LOLHIP_ERR_DEVICE when the calling thread's current device is not the plan's.  Every one is decided on the host
 *   before any launch: the output is then not written.  No call synchronises or allocates. */
typedef struct lolhip_khprf lolhip_khprf;
LOLHIP_API int lolhip_khprf_create(const lolhip_plan *pq, int64_t base, const int32_t *tree, int ntree,
                                   const int64_t *a0_crt, const int64_t *a1_crt, lolhip_khprf **out);
LOLHIP_API void lolhip_khprf_destroy(lolhip_khprf *f);
LOLHIP_API int64_t lolhip_khprf_work_len(const lolhip_khprf *f, int64_t x0, int64_t B);
LOLHIP_API int lolhip_khprf_eval_batch(const lolhip_khprf *f, void *stream, int64_t x0, int64_t B, int64_t *out,
                                       int64_t *work);
LOLHIP_API int lolhip_khprf_batch(const lolhip_khprf *f, void *stream, const int64_t *s_crt, int nkeys, int64_t p,
                                  int64_t x0, int64_t B, int64_t *out, int64_t *work);

/* The lifted family: the same PRF over q = 2^k, which has no CRT basis (the reference's own Zq 8 -> Zq 2 over F128, and
 * HomomPRF's ZP = Zq 8).  pq: a one-modulus plan mod q = 2^k (1 <= k); pQ: a one-modulus plan of the same index (the
 * same prime powers in the same order) over an NTT-friendly prime Q (lolhip_good_q); a0_pow, a1_pow: HOST arrays [L][n]
 * in the POWERFUL basis (any int64, taken mod q), L = lolhip_decompose_len(pq, base).
 *   Every node product sum_i L_i digit_i is computed exactly over the integers in the CRT basis mod Q, then crtInv,
 *   centred lift mod Q, reduced mod q, and lifted (centred, [-q/2, q/2)) and crt'd again where the next product needs
 *   it; decompose and lInv run on pq.  Creation certifies exactness: with C_m = max_k sum_{i,j} |(b_i b_j)_k| over the
 *   powerful basis b (n for m = 2^e, a product over the prime powers of m), L C_m (q/2) max|digit| < Q/2 and
 *   C_m (q/2)^2 < Q/2 (the key product of ringPRF); max|digit| is q/2 under TrivGad, else the larger of b/2 and the
 *   last centred digit's range.
 * lolhip_khprf_create_lifted: LOLHIP_ERR_INVALID as for lolhip_khprf_create, and for plans of different indices;
 *   LOLHIP_ERR_MODULUS when q is not a power of two or the bound above does not hold; LOLHIP_ERR_NO_CRT when Q has no
 *   CRT basis.  Uploads as lolhip_khprf_create does (both plans must be device plans of the same device; either one
 *   host-only makes a host-only family); the family must be destroyed before either plan.
 * lolhip_khprf_work_len, lolhip_khprf_eval_batch and lolhip_khprf_batch take the lifted family unchanged, except:
 *   eval_batch writes A_T(x) as residues in [0, q) in the POWERFUL basis (there is no CRT basis mod q);
 *   batch takes s_crt [nkeys][n] as the centred lift of s in R_q, reduced mod Q, in the CRT basis mod Q (crt on pQ);
 *   the rounding is y = ((p lift z + q/2) >> k) mod p, the same rescaleMod over q = 2^k.  The statuses are the same
 *   (p >= q and p q >= 2^63 give LOLHIP_ERR_MODULUS); LOLHIP_ERR_NO_DEVICE when either plan is host-only. */
LOLHIP_API int lolhip_khprf_create_lifted(const lolhip_plan *pq, const lolhip_plan *pQ, int64_t base,
                                          const int32_t *tree, int ntree, const int64_t *a0_pow,
                                          const int64_t *a1_pow, lolhip_khprf **out);

/* key-homomorphic PRF over standard lattices, eq. (2.3) of [BP14] (lol-apps KeyHomomorphicPRF.hs:189-207 latticePRF',
 * latticePRFM, over buildDecTree / evalTree), one modulus q, 2 <= q < 2^62 (even and 2-power moduli included: no
 * cyclotomic index and no CRT basis are involved).  With l = gadlen(base, q) (1 for base 0 = TrivGad) and K = n l, a
 * family is a full binary tree of k leaves (1 <= k <= 62, the encoding of lolhip_khprf_create) and A0, A1 in Z_q^(n x K):
 *     A_leaf(x) = A_x;   A_(I c l r)(x) = A_l(x >> c_r) * G^-1(A_r(x & (2^c_r - 1)))
 *   G^-1 = fmap reduce . decomposeMatrix (Gadget.hs:76-81) is K x K: row i l + j of column c is digit j of entry (i, c),
 *   digits ordered and centred as lolhip_decompose_batch does (ZqBasic.hs:227-232, 258-264).
 *     latticePRF' s x = rescale <$> s * A_T(x), s in Z_q^(1 x n):  y = fst (divModCent (p lift z) q) mod p per entry z
 *   (lift centred into [-q/2, q/2); divModCent a q = floor((a + q div 2) / q)).
 * lolhip_lprf_create: a0, a1 HOST arrays [n][K] of any int64, taken mod q.  The family lives on the calling thread's
 *   current device (as a plan does); without a device it is host-only and answers work_len only.  Allocates and
 *   synchronises; nothing after it does.
 * lolhip_lprf_work_len: int64 words of scratch of a call over inputs [x0, x0 + B); nkeys = 0 for eval_batch, the key count
 *   for batch (negative status on error).  With U_v = min(2^c_v, ((x0 + B - 1) >> s_v) - (x0 >> s_v) + 1) the slot count
 *   of node v (2 for a leaf) as for lolhip_khprf_work_len:
 *       sum over internal nodes v other than the root of U_v n K,  plus for nkeys > 0 and an internal root  U_l nkeys K
 *   (s A_l for every slot of the root's left child l); 0 for B = 0 or a one-leaf tree.  There is no per-slot K x K term:
 *   the digits of a right operand are produced where its tile is loaded and never stored.
 * lolhip_lprf_eval_batch: out [B][n][K] = A_T(x) for x = x0 .. x0 + B - 1, residues in [0, q); every distinct subtree
 *   value of the window is computed once.
 * lolhip_lprf_batch: s [nkeys][n] on the device, any int64 (taken mod q); out [nkeys][B][K] = latticePRF s_key x in
 *   [0, p).  The root is computed as (s A_l) * G^-1(A_r) (nkeys rows instead of n; the same residues mod q), with the
 *   rounding in its write-back.
 * Node products take one of two routes with the same bits: the matrix cores (i8 MFMA: the left operand in W <= 8
 *   balanced base-256 limbs, the digits as int8, one i32 sum per limb recombined mod q) where max|digit| <= 127 and
 *   K 128 max|digit| < 2^31 are certified from (q, base) and K >= 56 (below that a call is bound by its launches and
 *   the matrix route measured no faster), else int64 lazy sums on the vector ALU (debug switch LPRF_VALU forces this).  With the environment variable LOLHIP_LPRF_INFO set (read at every call) each node launch
 *   prints one line to stderr: "k_lprf: route <mfma|valu>, M <rows>, N <cols>, K <depth>, W <limbs>, slots <U>".
 * Status, decided on the host before any launch (the output is then not written): LOLHIP_ERR_INVALID for n < 1, a
 *   malformed tree or k > 62, base 1 or negative, NULL pointers, x0 < 0, B < 0, x0 + B > 2^k, nkeys < 1 for batch (< 0
 *   for work_len), n K >= 2^31; LOLHIP_ERR_MODULUS for q < 2, q >= 2^62, p < 2, p >= q, p q >= 2^63; LOLHIP_ERR_NO_DEVICE
 *   on a host-only family; LOLHIP_ERR_DEVICE when the current device is not the family's. */
typedef struct lolhip_lprf lolhip_lprf;
LOLHIP_API int lolhip_lprf_create(int64_t q, int64_t base, int n, const int32_t *tree, int ntree, const int64_t *a0,
                                  const int64_t *a1, lolhip_lprf **out);
LOLHIP_API void lolhip_lprf_destroy(lolhip_lprf *f);
LOLHIP_API int lolhip_lprf_n(const lolhip_lprf *f);
LOLHIP_API int lolhip_lprf_ell(const lolhip_lprf *f);
LOLHIP_API int64_t lolhip_lprf_work_len(const lolhip_lprf *f, int nkeys, int64_t x0, int64_t B);
LOLHIP_API int lolhip_lprf_eval_batch(const lolhip_lprf *f, void *stream, int64_t x0, int64_t B, int64_t *out,
                                      int64_t *work);
LOLHIP_API int lolhip_lprf_batch(const lolhip_lprf *f, void *stream, const int64_t *s, int nkeys, int64_t p, int64_t x0,
                                 int64_t B, int64_t *out, int64_t *work);

/* SymmSHE public operations and ciphertext addition (lol-apps SymmSHE.hs:214-230, 381-436; ZqBasic.hs:92-94,132-137).
 * A ciphertext is CT enc k l c over R'_q (pq: index m', moduli q_0..q_{T-1}, Q = prod q_t): components cs
 * [ncs][B][n'][T].  Public values are elements of R_m (m | m') mod p in the powerful basis, [B][n_m] int64 of any value
 * (taken mod p), item b at b * stride; stride 0 = one value for the whole batch, otherwise stride >= n_m (the lifted
 * output [B][L][n] of lolhip_khprf_eval_batch passes with stride L n).  decode' lifts v in [0, p) to v for 2v < p, else
 * v - p (p/2 lifts to -p/2).
 * lolhip_encode_scales: the encoding factors of the product ring, on the host (host-only plans too):
 *   to_msd = 1: lsdToMSD = (zp = -Q mod p, zq_t = p^-1 mod q_t);  to_msd = 0: msdToLSD = (zp = (-Q)^-1 mod p,
 *   zq_t = p mod q_t).  toMSD / toLSD multiply every c_i by zq and l by zp.
 * lolhip_ct_lincomb_batch: out_i = alpha_t a_i + beta_t b_i mod q_t for i < max(na, nb), a missing component counting
 *   as zero; alpha, beta: HOST arrays [T] of any int64; b = NULL with nb = 0 for out = alpha a.  Either basis.  out may
 *   alias a or b.  toMSD / toLSD / mulScalar (alpha = decode'(a) mod q_t) / negate (alpha = -1) / subtraction and the
 *   componentwise (+) are this one pass.
 * lolhip_add_public_batch: addPublic b (SymmSHE.hs:381-390): toLSD, then c_0 += embed (reduce (decode' v)) with
 *   v = l^-1 g_m^k b in R_m mod p (mulGPow of index m, k times).  cs in the powerful basis (cs_crt = 0) or the CRT basis
 *   (cs_crt = 1), out in the same basis; enc 0 = LSD, 1 = MSD; *l_out = l after toLSD; k is unchanged.  pp_m: the plan
 *   of index m over p alone (read for k > 0 only; it runs lolhip_mulgpow_batch).
 * lolhip_mul_public_batch: mulPublic a (SymmSHE.hs:405-411): every c_i times embed (reduce (decode' a)); cs and out in
 *   the CRT basis; enc, k and l do not change.  absorbGFactors (:464-473) is lolhip_divgpow_batch k times on the plan
 *   (m', p) applied to 1, then this call with stride 0 and x_q = NULL.
 * Both: x_q is an ext from the plan of (m, q_0..q_{T-1}) to pq, or NULL for m = m'; cs_shared = 1: one ciphertext for
 *   the whole batch ([ncs][1][n'][T]); out [ncs][B][n'][T] may alias cs unless cs is shared and B > 1.  The embedding
 *   is a gather folded into the pass: baseIndicesCRT (CRT basis; the public value goes through a crt of index m) or
 *   embedPow (powerful basis).  work: lolhip_public_work_len(pq, x_q, B) int64 of device scratch.
 * Status: LOLHIP_ERR_INVALID for ncs < 1, B < 0, T > 16, x_q not ending in pq's ring and moduli, a bad stride, pp_m not
 *   of index m over p alone (k > 0), out = a shared cs with B > 1, NULL pointers; LOLHIP_ERR_NO_CRT for a CRT-basis path
 *   whose plans have no CRT basis; LOLHIP_ERR_MODULUS for p < 2 or p >= 2^62, l not invertible mod p, MSD input with
 *   gcd(Q, p) != 1 (encode_scales: p not invertible mod some q_t for to_msd = 1); LOLHIP_ERR_NO_DEVICE on a host-only
 *   plan or ext; LOLHIP_ERR_DEVICE as elsewhere.  Every one is decided on the host before any launch: the output (and
 *   *l_out) is then not written.  No call synchronises or allocates. */
LOLHIP_API int lolhip_encode_scales(const lolhip_plan *pq, int64_t p, int to_msd, int64_t *zq_scale, int64_t *zp_scale);
LOLHIP_API int lolhip_ct_lincomb_batch(const lolhip_plan *pq, void *stream, const int64_t *a, int na, const int64_t *alpha,
                                       const int64_t *b, int nb, const int64_t *beta, int64_t *out, int64_t B);
LOLHIP_API int64_t lolhip_public_work_len(const lolhip_plan *pq, const lolhip_ext *x_q, int64_t B);
LOLHIP_API int lolhip_add_public_batch(const lolhip_plan *pq, const lolhip_ext *x_q, const lolhip_plan *pp_m, void *stream,
                                       const int64_t *b_pow, int64_t b_stride, const int64_t *cs, int ncs, int cs_shared,
                                       int cs_crt, int enc, int64_t k, int64_t l, int64_t p, int64_t *out, int64_t *l_out,
                                       int64_t *work, int64_t B);
LOLHIP_API int lolhip_mul_public_batch(const lolhip_plan *pq, const lolhip_ext *x_q, void *stream, const int64_t *a_pow,
                                       int64_t a_stride, int64_t p, const int64_t *cs, int ncs, int cs_shared,
                                       int64_t *out, int64_t *work, int64_t B);

/* Ciphertext modSwitch and multi-hop tunnelling (lol-apps SymmSHE.hs:236-246, HomomPRF.hs:153-155, 427-431;
 * lol Prelude.hs:227-232, 274-308).
 * lolhip_modswitch_batch: modSwitch of CT enc k l c from the moduli of `from` to those of `to`.  Both plans have the
 *   same index (same prime powers, same order); to's moduli are a suffix of from's (down: the first d = T - T' moduli
 *   are dropped, 1 <= d <= 5), from's are a suffix of to's (up: u = T' - T moduli are added in front, 1 <= u <= 5), or
 *   the lists are equal (toMSD alone).  cs [ncs][B][n][T] in the powerful basis (cs_crt = 0) or the CRT basis
 *   (cs_crt = 1), residues in (-q_t, q_t); it is only read.  out [ncs][B][n][T'] canonical, powerful basis
 *   (out_crt = 0) or CRT basis (out_crt = 1); it must not overlap cs or work.  enc 0 = LSD, 1 = MSD; the result is
 *   always MSD with *l_out = l mod p for MSD input and (-Q_from mod p) l mod p for LSD input (lolhip_encode_scales);
 *   k is unchanged.  c_0 is rescaled in the decoding basis, the other components in the powerful basis (modSwitchMSD).
 *   Down iterates the reference's one-step rule, which is not one rounding by q_0 ... q_{d-1}: for i = 0 .. d-1,
 *   z = lift c_i (a for 2a < q_i, else a - q_i) and c_s <- q_i^-1 (c_s - z) mod q_s for every s > i.  Up puts 0 into
 *   the new leading components and multiplies every old one by the product of the new moduli.
 *   Launch plan: crtInv on from (cs_crt) -> lInv on from over c_0 -> k_modswitch (toMSD scale, down / up, one pass)
 *   -> l on to over c_0 -> crt on to (out_crt).  With equal lists (the scale alone, which commutes with l / lInv) the
 *   two passes over c_0 are left out.
 *   work: lolhip_modswitch_work_len(from, to, ncs, B) = ncs B n T int64 of device scratch (0 for B = 0; a negative
 *   status for bad arguments): the copy of cs that crtInv / lInv transform.
 * Status: LOLHIP_ERR_INVALID for NULL pointers, ncs < 1, B < 0, enc not 0 / 1, plans of different indices, moduli lists
 *   that are not suffix-related, more than 5 moduli dropped or added, T or T' > 16; LOLHIP_ERR_MODULUS for p < 2 (or
 *   p >= 2^62), LSD input with p not invertible mod some q_t, a dropped modulus not invertible mod a kept one;
 *   LOLHIP_ERR_NO_CRT for a CRT-basis side whose plan has no CRT basis; LOLHIP_ERR_NO_DEVICE on a host-only plan;
 *   LOLHIP_ERR_DEVICE as elsewhere.  Every one is decided on the host before any launch: out and *l_out are then not
 *   written.  A failing launch (LOLHIP_ERR_HIP) leaves out undefined and *l_out unwritten.  The call does not allocate
 *   or synchronise. */
LOLHIP_API int64_t lolhip_modswitch_work_len(const lolhip_plan *from, const lolhip_plan *to, int ncs, int64_t B);
LOLHIP_API int lolhip_modswitch_batch(const lolhip_plan *from, const lolhip_plan *to, void *stream, const int64_t *cs,
                                      int ncs, int cs_crt, int enc, int64_t l, int64_t p, int64_t *out, int out_crt,
                                      int64_t *l_out, int64_t *work, int64_t B);
/* tunnelH (HomomPRF.hs:427-431) = roundCTDown . roundCTDown . tunnelInternal hints . roundCTUp as one call.
 * lolhip_tunnel_chain_create: hop i is lolhip_tunnel_batch(x_er[i], x_es[i], ys_crt[i], hints[i], base) from R'_i (the
 *   high plan of x_er[i]) to S'_i (the high plan of x_es[i]); ys_crt[i] and hints[i] are DEVICE pointers the chain
 *   borrows (layouts of lolhip_tunnel_batch; they must outlive the chain's calls), the exts and plans are borrowed too.
 *   All hops share one moduli list, the up list; S'_i and R'_{i+1} have the same index and moduli.  p_in: a plan of
 *   R'_0's index whose moduli are a suffix of the up list (u = 0..5 moduli are added on entry); p_out: a plan of the
 *   last S' index whose moduli are a suffix of the up list (d = 0..5 are dropped on exit).  nhops = 0: p_in and p_out
 *   have the same index and the call is lolhip_modswitch_batch(p_in, p_out).  Create validates and copies host
 *   metadata only.
 * lolhip_tunnel_chain_batch: cs [2][B][n_R'][T_in], a linear ciphertext with k = 0 (absorbGFactors stays the caller's
 *   job: lolhip_divgpow_batch on 1 and lolhip_mul_public_batch, as above), bases and enc / l / p as for
 *   lolhip_modswitch_batch; out [2][B][n_S'][T_out], MSD, *l_out as there.  Steps: modSwitch up from p_in (this is also
 *   toMSD) -> per hop the tunnel, and between hops one crtInv over both components and lInv over c_0 -> ONE modSwitch
 *   down by d after the last hop (successive roundCTDowns are one d-step pass: both act coefficient-wise in the same
 *   bases).  work: lolhip_tunnel_chain_work_len(c, B) int64 = 4 B n_max T_up (two ciphertext buffers, n_max over R'_0
 *   and every S'_i) + the largest of lolhip_modswitch_work_len(p_in, R'_0, 2, B) and the hops'
 *   lolhip_tunnel_work_len; for nhops = 0 it is lolhip_modswitch_work_len(p_in, p_out, 2, B).
 * Status: as for the pieces; LOLHIP_ERR_INVALID also for nhops < 0, mismatched neighbouring hops, hops over other
 *   moduli than the first, plans not of the end rings.  Nothing allocates or synchronises after create.  Every status
 *   but a failing launch is decided on the host before the first launch: out and *l_out are then not written.  A
 *   launch that fails mid-chain (LOLHIP_ERR_HIP, a transform's ring allocation included) leaves out undefined and *l_out
 *   unwritten. */
typedef struct lolhip_tunnel_chain lolhip_tunnel_chain;
LOLHIP_API int lolhip_tunnel_chain_create(int nhops, const lolhip_ext *const *x_er, const lolhip_ext *const *x_es,
                                          const int64_t *const *ys_crt, const int64_t *const *hints, int64_t base,
                                          const lolhip_plan *p_in, const lolhip_plan *p_out, lolhip_tunnel_chain **out);
LOLHIP_API void lolhip_tunnel_chain_destroy(lolhip_tunnel_chain *c);
LOLHIP_API int64_t lolhip_tunnel_chain_work_len(const lolhip_tunnel_chain *c, int64_t B);
LOLHIP_API int lolhip_tunnel_chain_batch(const lolhip_tunnel_chain *c, void *stream, const int64_t *cs, int cs_crt, int enc,
                                         int64_t l, int64_t p, int64_t *out, int out_crt, int64_t *l_out, int64_t *work,
                                         int64_t B);

/* Homomorphic rounding 2^e -> 2 (ptRound, lol-apps HomomPRF.hs:215-270 over SymmSHE.hs:236-258, 361-390, 444-452).
 * lolhip_ct_affine_mul_batch: the ciphertext product with both affine pre-steps folded in, CRT basis, one pass.  a, b:
 *   linear ciphertexts [2][B][n'][T], residues in (-q_t, q_t); the same pointer may be passed for both.  alpha, beta:
 *   HOST arrays [T] of any int64 (the toLSD / toMSD factors of lolhip_encode_scales, or 1).  va, vb: polynomials
 *   [npairs][n'][T] shared by the batch, residues in (-q_t, q_t), or NULL (zero).  For every pair j < npairs
 *     A0 = alpha_t a_0 + va_j,  A1 = alpha_t a_1;   B0 = beta_t b_0 + vb_j,  B1 = beta_t b_1
 *     out_j = (g A0 B0, g (A0 B1 + A1 B0), g A1 B1),  g = gCRT (as lolhip_ctmul_crt_batch)
 *   out [npairs][3][B][n'][T], canonical; with npairs = 1 it may alias a or b.  x (p x + v) (addPublic then (*)) is
 *   a = b = x, beta = p, vb = v; the fan-out (x + v_{2j-1}) (p (x + v_{2j})) over the pairs j reads x once per pair and
 *   never stores the fanned-out ciphertexts.  Two words per lane with 16-byte accesses when n' T is even and every pointer
 *   is 16-byte aligned, else one word per lane.
 *   Status: LOLHIP_ERR_INVALID for npairs < 1 or > 65535, B < 0, T > 16, NULL pointers (va, vb excepted), out = a or b
 *   with npairs > 1; LOLHIP_ERR_NO_CRT; LOLHIP_ERR_NO_DEVICE / LOLHIP_ERR_DEVICE as elsewhere; all before the launch.
 * lolhip_ptround_create: ptRound from plaintext modulus p = 2^e (1 <= e <= 16) to 2.  p_lvl[i], i < e: the plan of
 *   index m' over Z_i, Z_{i+1} = Z_i without its first modulus (ZqDown); p_up[i], i < e - 1: the plan of index m' over
 *   U_i = Z_i with one more modulus in front (ZqUp); hints[i], i < e - 1: DEVICE pointer, borrowed, ksQuadCircHint of
 *   the key over U_i, [L_i][2][n'][T(U_i)] with L_i = lolhip_decompose_len(p_up[i], base) (all hints over one gadget);
 *   pp_m: the plan of index m over p alone (mulGPow of the public constants; needed for e >= 2); x_q0 / x_q1: exts from
 *   the plans of (m, Z_0) / (m, Z_1) into p_lvl[0] / p_lvl[1], or both NULL for m = m'.  Plans, exts and hints are
 *   borrowed and must outlive the handle.  Create validates, copies host metadata and uploads the public constants'
 *   source (1 and y (1 - y), y = 1 .. p/4, as elements of R_m: (p/4 + 1) n_m words) when the plans are device plans.
 *   Status: LOLHIP_ERR_INVALID for e < 1 or > 16, NULL pointers, lists that are not this ladder, plans of different
 *   indices, T(U_0) > 16, a bad base, pp_m not of index m over p alone, exts not ending in p_lvl[0] / p_lvl[1] or not
 *   from one index; LOLHIP_ERR_MODULUS for p != 2^e or an even modulus (gcd(Q, 2) != 1); LOLHIP_ERR_NO_CRT for a plan
 *   of the ladder without a CRT basis; LOLHIP_ERR_HIP for a failing upload.
 * lolhip_ptround_batch: cs [2][B][n'][T(Z_0)], CT enc k l over plaintext modulus p, powerful basis (cs_crt = 0) or CRT
 *   basis (cs_crt = 1), enc 0 = LSD, 1 = MSD -> out [2][B][n'][T(Z_{e-1})], an MSD ciphertext of the rounding over
 *   plaintext modulus 2 in the basis out_crt asks for, *k_out = 2^(e-1) (k + 1) - 1, *l_out as the reference moves l
 *   (toLSD / toMSD factors, products, reduce . lift into every halved modulus).  e = 1: out = cs (copied when the
 *   pointers differ, the basis converted when cs_crt != out_crt), enc, k and l unchanged.  Launch plan, level i over
 *   plaintext modulus p_i = p / 2^i:
 *     constants  k_pub_lift -> mulGPow k times on pp_m -> k_pub_lift (l^-1 folded in) -> crt at index m -> k_pub_apply
 *                (the embed gather) -> k_ct_lincomb (the toMSD factor), once per call at B = 1: the constant 1 for level
 *                0, y (1 - y) for level 1
 *     level 0    k_ct_affine_mul x (p x + 1)  (a = b = x, beta = p for MSD input)
 *     level 1    k_ct_affine_mul (p_1 (xprod + v_{2j-1})) (xprod + v_{2j}) for every pair j < p/8, from xprod alone
 *     level >= 2 k_ct_affine_mul (p_i a) b over the pairs of the previous level's outputs
 *     then, per product: lolhip_modswitch_batch Z_i -> U_i (3 components, CRT in, powerful out), crt over c_0, c_1,
 *                lolhip_keyswitch_batch(hints[i]) over U_i, lolhip_modswitch_batch U_i -> Z_{i+1} (CRT in; CRT out, or
 *                the caller's basis into out after the last level)
 *   work: lolhip_ptround_work_len(c, B) int64 of device scratch, 16-byte aligned, with N = B n', T_i = T(Z_i),
 *   T_u = T_0 + 1 and every term rounded up to even:  the products max(3 N T_0, 3 (p/8) N T_1)  +  two ciphertext lists
 *   of max(2 N T_0, 2 (p/8) N T_2) each  +  3 N T_u (up)  +  2 N T_u (key-switch output)  +  max_i L_i N T_u (digits)
 *   +  max(3 N T_0, 2 N T_u) (modSwitch scratch)  +  the constants: (p/4 + 1) (n' T_0 + n_m T_0 + n_m) + n' T_0.
 *   0 for B = 0 or e = 1; a negative status for bad arguments.
 *   Status: LOLHIP_ERR_INVALID for NULL pointers, B < 0, enc not 0 / 1, k < 0 or k > 2^40 / p; LOLHIP_ERR_MODULUS
 *   for l not invertible mod p, and as lolhip_modswitch_batch; LOLHIP_ERR_NO_DEVICE on host-only plans;
 *   LOLHIP_ERR_DEVICE as elsewhere.
 *   Every status but a failing launch is decided on the host before the first launch: out, *k_out and *l_out are then
 *   not written.  A failing launch (LOLHIP_ERR_HIP) leaves out undefined and the scalars unwritten.  The call does not
 *   allocate or synchronise. */
LOLHIP_API int lolhip_ct_affine_mul_batch(const lolhip_plan *pq, void *stream, const int64_t *a, const int64_t *alpha,
                                          const int64_t *va, const int64_t *b, const int64_t *beta, const int64_t *vb,
                                          int npairs, int64_t *out, int64_t B);
typedef struct lolhip_ptround lolhip_ptround;
LOLHIP_API int lolhip_ptround_create(int e, int64_t p, const lolhip_plan *const *p_lvl, const lolhip_plan *const *p_up,
                                     const int64_t *const *hints, int64_t base, const lolhip_plan *pp_m,
                                     const lolhip_ext *x_q0, const lolhip_ext *x_q1, lolhip_ptround **out);
LOLHIP_API void lolhip_ptround_destroy(lolhip_ptround *c);
LOLHIP_API int64_t lolhip_ptround_work_len(const lolhip_ptround *c, int64_t B);
LOLHIP_API int lolhip_ptround_batch(const lolhip_ptround *c, void *stream, const int64_t *cs, int cs_crt, int enc, int64_t k,
                                    int64_t l, int64_t *out, int out_crt, int64_t *k_out, int64_t *l_out, int64_t *work,
                                    int64_t B);

/* The ciphertext product (*) of any degree (instance Ring.C (CT m zp (Cyc t m' zq)), lol-apps SymmSHE.hs:438-452).
 * lolhip_ct_mul_rule, host only: the rule of (*) (:444-452).  enc 0 = LSD, 1 = MSD.  Both MSD -> toLSD on the first
 *   operand: alpha_t = p mod q_t and l1 <- l1 (-Q)^-1 mod p (LOLHIP_ERR_MODULUS when gcd(Q, p) != 1), else alpha_t = 1.
 *   enc_out = LSD iff both are LSD, else MSD;  k_out = k1 + k2 + 1;  l_out = l1 l2 mod p.  alpha: HOST array [T].
 *   Status: LOLHIP_ERR_INVALID for NULL pointers, enc not 0 / 1, k < 0, T > 16; LOLHIP_ERR_MODULUS for p < 2 or
 *   p >= 2^62 (every encoding pair), and as above.  Nothing is written on error.
 * lolhip_ct_mul_batch: a [na][B][n'][T] times b [nb][B][n'][T], 1 <= na, nb <= LOLHIP_CT_MUL_MAX, residues in
 *   (-q_t, q_t), both in the CRT basis (cs_crt = 1) or both in the powerful basis (cs_crt = 0) ->
 *     out_k = alpha_t g sum_{i + j = k} a_i b_j mod q_t,  k < na + nb - 1,  g = gCRT (mulG <$> (c1 * c2), :449)
 *   out [na + nb - 1][B][n'][T], canonical, in the CRT basis (out_crt = 1) or the powerful basis (out_crt = 0).  alpha:
 *   HOST array [T] of any int64 (from lolhip_ct_mul_rule), or NULL for 1.  b == a with nb == na squares: every input
 *   word is read once, cross terms are doubled.  a and b are only read.  Launch plan: cs_crt = 0: a and b copied into
 *   work and one batched crt over all (na + nb) B polynomials there (the square: na B); k_ct_mul (component counts up
 *   to 3 x 3 compiled in: two words per lane with 16-byte accesses when n' T is even and every pointer is 16-byte
 *   aligned, else one word per lane; larger counts through the run-time form, one word per lane; two distinct linear
 *   operands with alpha = 1 through the kernel of lolhip_ctmul_crt_batch, which computes the same); out_crt = 0: crtInv in place on out.
 *   work: lolhip_ct_mul_work_len(pq, na, nb, cs_crt, square, B) int64 of device scratch, 16-byte aligned:
 *   (na + (square ? 0 : nb)) B n' T for cs_crt = 0, else 0 (work may then be NULL); a negative status for bad arguments.
 *   Status, decided on the host in this order before any launch (out is then not written): LOLHIP_ERR_INVALID for a
 *   NULL plan, na or nb outside 1 .. LOLHIP_CT_MUL_MAX, B < 0, T > 16, a NULL pointer beside B > 0 (alpha excepted;
 *   work only for cs_crt = 0), out = a or out = b (the output has more components than either input: it cannot alias);
 *   LOLHIP_ERR_NO_CRT when pq has no CRT basis; LOLHIP_ERR_NO_DEVICE on a host-only plan, LOLHIP_ERR_DEVICE as
 *   elsewhere.  B = 0 returns LOLHIP_OK.  A failing launch (LOLHIP_ERR_HIP) leaves out undefined.  The call does not
 *   allocate or synchronise (beyond what crt / crtInv do). */
#define LOLHIP_CT_MUL_MAX 8
LOLHIP_API int lolhip_ct_mul_rule(const lolhip_plan *pq, int64_t p, int enc1, int64_t k1, int64_t l1, int enc2, int64_t k2,
                                  int64_t l2, int64_t *alpha, int *enc_out, int64_t *k_out, int64_t *l_out);
LOLHIP_API int64_t lolhip_ct_mul_work_len(const lolhip_plan *pq, int na, int nb, int cs_crt, int square, int64_t B);
LOLHIP_API int lolhip_ct_mul_batch(const lolhip_plan *pq, void *stream, const int64_t *a, int na, const int64_t *b, int nb,
                                   int cs_crt, const int64_t *alpha, int64_t *out, int out_crt, int64_t *work, int64_t B);

/* --- gSqNormDec and RLWE / RLWR instances (lol RLWE/{Continuous,Discrete,RLWR}.hs; rlwe-challenges Generate.hs:192-218,
 * Verify.hs:346-366), device pointers ------------------------------------------------------------------------------
 * gSqNormDec (Tensor.hs:147-151; norm.cpp:15-75): e_dec [B][n] decoding-basis coefficients -> out [B],
 *     out_b = <e_b, y_b>,  y = (I_{p^(e-1)} (x) (I+J)_{p-1}) e  applied along the prime dimension of every odd prime p of m
 *   (the first prime power of the plan fastest-varying, tensor.h:40-80); sum e_j^2 for m = 2^k.  The plan supplies the
 *   index only; any index with n <= 16384 (no limit on the primes).
 *   lolhip_gsqnorm_batch: exact, or saturated: out = min(value, INT64_MAX), and INT64_MAX when a coefficient is INT64_MIN
 *   (the unliftable marker of lolhip_error_term_batch).  The reference wraps in Int64 instead.
 *   lolhip_gsqnorm_f64_batch: float64 under the tolerance contract above (relative 1e-12); the summation order is a
 *   function of n alone: no atomics, the same bits run to run, for every B and however a batch is split.
 * Samplers.  Three more domains of the ChaCha20 stream above, the item of sample b of a call being ctr + b: 5 = the
 *   uniform a, 6 = the Gaussians, 7 = the uniform secret; bit layouts of Gaussians and uniform residues exactly those of
 *   domains 0-2.  THE CALLER'S DUTY extends to them: never use one (key, ctr + b) twice for a domain; advance ctr by B
 *   after a sample call, and draw each secret at a ctr of its own (domain 7 is disjoint from 5 and 6 at equal ctr).
 *   kind: 0 = Discrete, 1 = Continuous, 2 = RLWR.
 *   lolhip_rlwe_secret: s_crt [n][T] uniform, CRT basis, item ctr of domain 7.
 *   lolhip_rlwe_sample_batch: a_crt [B][n][T] uniform, CRT basis, and
 *     Disc: b_out int64 [B][n][T], CRT basis, b = a s + reduce e, e = errorRounded svar with the arithmetic of
 *           lolhip_error_rounded_batch on domain 6 (Discrete.hs:38-45); any T <= 16.
 *     Cont: b_out double [B][n], decoding basis of K/(qR), in [0, q) (Continuous.hs:45-54 over RRq.hs:47-84): with
 *           x = (double) of the decoding-basis residue of a s in [0, q) and g = tGaussianDec svar (unrounded),
 *           r = g - q floor(g / q);  z = x + r;  b = z >= q ? z - q : z, these IEEE double operations in this order (b is
 *           a pure function of (x, g)).  T = 1.
 *     RLWR: b_out int64 [B][n] in [0, p), decoding basis, = roundedProd s a below; svar is ignored; T = 1, 2 <= p < q.
 *   p is read for RLWR only.  work: lolhip_rlwe_work_len(pq, kind, B) int64 of device scratch, which serves the sample
 *   call and the error / rounding calls of that kind alike.
 * lolhip_rlwe_error_batch (kind 0 or 1): the error term of B samples (a, b) under the purported secret s_crt and its
 *   gSqNorm.  Disc (Discrete.hs:48-59): e int64 [B][n] = liftDec (b - a s), the centred mixed-radix lift of
 *   lolhip_error_term_batch (INT64_MIN where it does not fit), norm int64 [B] as lolhip_gsqnorm_batch.  Cont
 *   (Continuous.hs:57-68): with x as above, nx = (-x) - q floor((-x) / q);  z = b + nx;  y = z >= q ? z - q : z;
 *   e = y + y < q ? y : y - q, doubles [B][n]; norm double [B] as lolhip_gsqnorm_f64_batch.  e_out or norm_out may be
 *   NULL (not both): with e_out = NULL the error slab stays in work.  norm_out needs n <= 16384.
 * lolhip_rlwr_rounded_prod_batch (RLWR.hs:34-44): per decoding-basis residue x of a s, l = 2x < q ? x : x - q,
 *   b = floor((p l + floor(q/2)) / q) mod p in [0, p), floor division in exact 128-bit integers (the reference agrees
 *   wherever its Int64 does not overflow).  lolhip_rlwr_check_batch: mismatch [B] int32 = the coefficients of sample b
 *   where the given b differs from that value, counted on the device; a valid sample has 0.
 * Limits: T <= 16; for Disc and Cont samples the sampler's index limits of lolhip_encrypt_batch.
 * Status, decided in this order on the host before any launch (outputs are then not written): LOLHIP_ERR_INVALID for an
 *   unknown kind, B < 0, T > 16, T != 1 where one modulus is required, p outside [2, q), svar <= 0 or not finite, an
 *   index beyond the limits; LOLHIP_ERR_NO_CRT when pq has no CRT basis; LOLHIP_ERR_MODULUS for a Disc error term over
 *   moduli that are not pairwise coprime; LOLHIP_ERR_NO_DEVICE on a host-only plan; LOLHIP_ERR_INVALID for NULL pointers
 *   at B > 0.  No call synchronises or allocates; output does not depend on how a batch is split.
 * lolhip_rlwe_error_bound (host; Continuous.hs:74-84, Discrete.hs:65-76): the bound the gSqNorm of an error of scaled
 *   variance svar over the index pps stays below except with probability about eps.  kind 1: mhat n svar stabilize(1/2pi)
 *   with x' = (1/2 + log(2 pi x)/2 - log(eps)/n)/pi iterated until x' - x < 0.0001; kind 0: ceiling(2^(odd primes of m) n
 *   stabilize'(1/2pi) + the continuous bound), x' = (1/2 + log(2 pi x)/2 - log eps)/pi, a double holding an integer.
 *   LOLHIP_ERR_INVALID for svar <= 0, eps outside (0, 1), non-finite inputs, a malformed prime-power list or kind. */
LOLHIP_API int lolhip_gsqnorm_batch    (const lolhip_plan *p, void *stream, const int64_t *e_dec, int64_t *out, int64_t B);
LOLHIP_API int lolhip_gsqnorm_f64_batch(const lolhip_plan *p, void *stream, const double *e_dec, double *out, int64_t B);
LOLHIP_API int64_t lolhip_rlwe_work_len(const lolhip_plan *pq, int kind, int64_t B);
LOLHIP_API int lolhip_rlwe_secret(const lolhip_plan *pq, void *stream, const uint8_t key[32], uint64_t ctr, int64_t *s_crt);
LOLHIP_API int lolhip_rlwe_sample_batch(const lolhip_plan *pq, void *stream, int kind, int64_t p, const int64_t *s_crt,
                                        double svar, const uint8_t key[32], uint64_t ctr, int64_t *a_crt, void *b_out,
                                        int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwe_error_batch(const lolhip_plan *pq, void *stream, int kind, const int64_t *a_crt, const void *b,
                                       const int64_t *s_crt, void *e_out, void *norm_out, int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwr_rounded_prod_batch(const lolhip_plan *pq, int64_t p, void *stream, const int64_t *a_crt,
                                              const int64_t *s_crt, int64_t *b_out, int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwr_check_batch(const lolhip_plan *pq, int64_t p, void *stream, const int64_t *a_crt, const int64_t *b,
                                       const int64_t *s_crt, int32_t *mismatch, int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwe_error_bound(const lolhip_pp *pps, int npps, double svar, double eps, int kind, double *out);

/* --- crtSetDec, crtSet, and the clear-text tunnel of HomomPRF (lol-cpp CPP/Extension.hs:131-164; lol UCyc.hs:540-565,
 * ZmStar.hs:52-88, Tensor.hs:300-313; lol-apps HomomPRF.hs:400-411, 510-531) ---------------------------------------
 * powBasisPow is lolhip_ext_table(x, 6): the n'/n indices at which the relative powerful basis elements are unit vectors.
 * lolhip_crtset_dec (host): the mod-p CRT set of O_m'/O_m, p prime, p not dividing m', m | m'.  With d = ord_m'(p),
 *   K = (phi(m')/d) / (phi(m)/ord_m(p)) elements; out [K][phi(m')] residues in [0, p), decoding basis of O_m':
 *     element c, entry j = mhat'^-1 Tr_{GF(p^d)/F_p}( sum_{i in reps_c} twCRTs(j, zmsToIndex i) )
 *   twCRTs(j, i) = prod_k w_k^(-pow_k(j_k) i) (1 - w_k^(i p_k^(e_k - 1)))  over the prime powers p_k^e_k of m' (the
 *   second factor for odd p_k only), w_k = w^(m'/p_k^e_k), pow_k = indexToPow, j_0 (the first prime power) fastest.
 *   reps_c: partitionCosets, in the reference's order.  The cosets of <p> in Z_m'^* are grouped by the coset of <p> in
 *   Z_m^* they reduce to; the groups are ordered by their smallest residue mod m, each group holds its cosets by
 *   DESCENDING smallest element, and element c takes coset c of every group (its smallest element is the representative).
 *   THE ROOT w.  GF(p^d) = F_p[x]/(f): f = x^d + a_(d-1) x^(d-1) + ... + a_0 is the first irreducible when the tuples
 *   (a_(d-1), ..., a_0) are counted up as base-p numbers, a_0 the least significant digit, from 0.  gen is the first
 *   element of multiplicative order p^d - 1 when the polynomials c_0 + c_1 x + ... are counted up as base-p numbers
 *   c = sum c_i p^i from 1.  w = gen^((p^d - 1)/m').  Another root only permutes the set; the reference's own choice
 *   (its table of irreducibles) is not reproduced, and nothing needs it: a TunnelHint message carries its function.
 *   cap: rows of out (out = NULL or cap = 0 queries K); min(K, cap) rows are written.  Returns K, or LOLHIP_ERR_INVALID
 *   for malformed lists, m not dividing m', p not prime or p | m'; LOLHIP_ERR_MODULUS when p^d >= 2^62.
 * crtSet(m, m', p, e): the mod-p^e CRT set of O_m'/O_m in the powerful basis, [K][phi(m')] residues in [0, p^e).
 *   mbar, mbar' = m, m' without their p-parts; c = crtSetDec(mbar, mbar', p) lifted to [0, p), taken to the powerful
 *   basis (l), reduced mod p^e, raised to the p-th power e - 1 times with a reduction mod p^e after every product,
 *   then embedPow from mbar' to m'.  The products are exact: each is computed over the integers.
 *   lolhip_crtset_modulus: the smallest prime Q = 1 mod mbar' with C_mbar' floor(p^e/2)^2 < Q/2 (C: the growth constant
 *     of the lifted PRF above), or LOLHIP_ERR_MODULUS when there is none below 2^61.
 *   lolhip_crtset (device): pQ = a one-modulus device plan of index mbar' over such a Q (CRT basis required, the bound
 *     is checked again).  Launch plan: upload, l on pQ, k_relift (reduce mod p^e, centred lift mod Q), then per power
 *     p - 1 times lolhip_polymul_batch over the K elements and k_relift, a last k_relift to residues, the embedPow
 *     gather.  out_dev [cap][phi(m')] on the device; min(K, cap) rows are written.  Setup-time: allocates and
 *     synchronises the stream.
 *   lolhip_crtset_host: the same set by schoolbook products on the host (no device, no Q; out is a host array): the
 *     same bits.  Meant for tests and small indices (its cost is K e phi(mbar')^2).
 *   All three return K, or: LOLHIP_ERR_INVALID as lolhip_crtset_dec, for e < 1, a plan of another index or of more
 *   than one modulus; LOLHIP_ERR_MODULUS when p^e >= 2^62 or no Q below 2^61 certifies the products (the host path
 *   reports it too), or pQ's modulus does not; LOLHIP_ERR_NO_CRT; LOLHIP_ERR_NO_DEVICE on a host-only plan.
 * ptTunnel: evalLin f_h hop by hop on a plaintext over Z_(p^e), which has no CRT basis.  Hop h maps R_h to S_h = R_(h+1)
 *   over E_h; x_er[h] / x_es[h]: the exts E_h in R_h / E_h in S_h, all three plans over ONE NTT prime Q_h (CRT basis
 *   required for S_h).  funcs_pow[h]: HOST array [rel_h][n_S_h], rel_h = n_R_h / n_E_h, the values of f_h on the
 *   relative decoding basis, any int64 taken mod p^e, powerful basis of S_h (the shape of TunnelChain.hints' funcs).
 *   Create lifts them (centred) and uploads crt of them mod Q_h.  Per hop: coeffs gather, embedDec, l, crt, knapsack
 *   (lolhip_evallin_batch over Q_h), crtInv, then k_relift: one pass that reads crtInv's output, takes the centred lift
 *   mod Q_h, reduces mod p^e and writes the residues in [0, p^e) (the hop's result, powerful basis of S_h) and / or
 *   their centred lift mod Q_(h+1); lInv on R_(h+1) then gives the next hop's decoding-basis input.
 *   Exactness, certified at create: with H = floor(p^e/2), C_S the growth constant of S_h, G_S = prod (p_k - 1) over
 *   the odd primes of S_h (l on lifted coefficients) and D_R = 2^(odd primes of R_h) for h > 0, 1 for h = 0 (lInv on
 *   lifted coefficients),   rel_h C_S G_S D_R H^2 < Q_h / 2.   lolhip_pt_tunnel_modulus(R_h, S_h, rel_h, first_hop, p, e):
 *   twice the left side (Q_h must exceed it; first_hop != 0: D_R = 1), or LOLHIP_ERR_MODULUS when that is not below 2^61.
 *   lolhip_pt_tunnel_batch: x_dec [B][n_R0] any int64 (taken mod p^e), decoding basis of R_0 -> out_pow [B][n_S_last]
 *   residues in [0, p^e), powerful basis.  nhops = 0 is not a tunnel: LOLHIP_ERR_INVALID.  work:
 *   lolhip_pt_tunnel_work_len(c, B) int64 of device scratch, 16-byte aligned: two slabs of B n_max (rounded up to even;
 *   n_max over R_0 and every S_h: a hop's input and output) + max_h rel_h B (n_E_h + n_S_h) (evalLin's scratch).  The call
 *   does not allocate or synchronise.
 *   Status: LOLHIP_ERR_INVALID for NULL pointers, nhops < 1 or > 16, e < 1, B < 0, exts of one hop over different
 *   E-plans or moduli, plans of more than one modulus, S_h and R_(h+1) of different indices; LOLHIP_ERR_MODULUS for
 *   p < 2, p^e >= 2^62 or a hop whose Q_h fails the bound; LOLHIP_ERR_NO_CRT for an S_h without a CRT basis;
 *   LOLHIP_ERR_NO_DEVICE from the compute calls of a chain over host-only plans (create then validates only);
 *   LOLHIP_ERR_DEVICE as elsewhere.  All decided on the host before any launch. */
LOLHIP_API int64_t lolhip_crtset_dec(const lolhip_pp *pps_m, int npps_m, const lolhip_pp *pps_m2, int npps_m2, int64_t p,
                                     int64_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_crtset_modulus(const lolhip_pp *pps_m2, int npps_m2, int64_t p, int e);
LOLHIP_API int64_t lolhip_crtset_host(const lolhip_pp *pps_m, int npps_m, const lolhip_pp *pps_m2, int npps_m2, int64_t p,
                                      int e, int64_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_crtset(const lolhip_plan *pQ, const lolhip_pp *pps_m, int npps_m, const lolhip_pp *pps_m2,
                                 int npps_m2, int64_t p, int e, void *stream, int64_t *out_dev, int64_t cap);
typedef struct lolhip_pt_tunnel lolhip_pt_tunnel;
LOLHIP_API int64_t lolhip_pt_tunnel_modulus(const lolhip_pp *pps_r, int npps_r, const lolhip_pp *pps_s, int npps_s,
                                            int64_t rel, int first_hop, int64_t p, int e);
LOLHIP_API int lolhip_pt_tunnel_create(int nhops, const lolhip_ext *const *x_er, const lolhip_ext *const *x_es,
                                       const int64_t *const *funcs_pow, int64_t p, int e, lolhip_pt_tunnel **out);
LOLHIP_API void lolhip_pt_tunnel_destroy(lolhip_pt_tunnel *c);
LOLHIP_API int64_t lolhip_pt_tunnel_work_len(const lolhip_pt_tunnel *c, int64_t B);
LOLHIP_API int lolhip_pt_tunnel_batch(const lolhip_pt_tunnel *c, void *stream, const int64_t *x_dec, int64_t *out_pow,
                                      int64_t *work, int64_t B);

/* --- exact ring product over moduli without a CRT basis (ringmul_api.cpp, ringmul.hip) ----------------------------
 * out = a * b in R_q = Z_q[zeta_m] for ANY moduli q_0 .. q_(T-1) in [2, 2^62): 2^e, p^e, odd composites, primes of the
 * wrong residue class, where lolhip_polymul_batch answers LOLHIP_ERR_NO_CRT.  The exact counterpart of the reference's
 * fallback through the CRT over C (Cyc (*), Cyc.hs:262-297; CRTExt, UCyc.hs:422-444), which is approximate once
 * n q^2 leaves 53 bits.
 *   pq: any plan of index m over the q_t, T <= 16, no CRT basis needed.  pQ: a plan of the SAME index (same prime
 *   powers in the same order) over K <= 3 pairwise distinct NTT primes Q_0 .. Q_(K-1), CRT basis required.
 *   Lift convention (that of k_relift above): an operand coefficient, any int64, is taken mod q_t; the residue r lifts
 *   to r when 2 r < q_t, else to r - q_t, so |lift| <= H_t = floor(q_t / 2).
 *   Exactness, certified at create in 256-bit arithmetic: a powerful-basis coefficient of the integer product is at
 *   most C_m H^2 in absolute value, C_m the growth constant of the index (that of the lifted PRF and of crtSet above),
 *   H = max_t H_t; the product over prod Q is exact iff   2 C_m H^2 < Q_0 ... Q_(K-1).
 *   Way back: the centred lift of the K residues (mixed radix over pQ's own lift constants, lolhip_plan_table 12; the
 *   sign from a most-significant-first digit comparison), reduced mod q_t into [0, q_t).
 * lolhip_ringmul_moduli(pps, npps, qs, T, Qs): the default primes, by this rule.  bound = 2 C_m H^2.  For K = 1, 2, 3 in
 *   this order: r = the smallest integer with r^K >= bound (exact); Q_0 = the smallest prime = 1 mod m above r
 *   (lolhip_good_q(m, r)), Q_i = lolhip_good_q(m, Q_(i-1)); the first K whose primes all lie below 2^61 wins.  Every
 *   prime exceeds r, so the product exceeds the bound (were it not to, the window of K consecutive primes would move up
 *   one prime at a time).  Returns K and writes Qs[0..K), zero above; LOLHIP_ERR_MODULUS when no K <= 3 serves (the
 *   growth constant saturates at 2^62, or the bound is beyond three primes) or a q_t lies outside [2, 2^62);
 *   LOLHIP_ERR_INVALID for NULL pointers, T < 1, a list that is not ascending primes with exponents >= 1.
 * lolhip_ringmul_create(pq, pQ, &h): validates, certifies the bound and precomputes per component P_i mod q_t
 *   (P_i = Q_0 ... Q_(i-1)) and prod Q mod q_t; they travel by value in every launch (H_t = q_t >> 1 needs no table:
 *   the kernels test 2 r < q_t).  pQ must outlive the handle; pq is not referenced after create.  Over host-only plans it validates only: the compute calls then return LOLHIP_ERR_NO_DEVICE.
 * lolhip_ringmul_work_len(h, B): int64 words of device scratch, 16-byte aligned:  2 * even(B T n K)  — the lifted a
 *   and b, each rounded up to an even word count.
 * lolhip_ringmul_batch(h, stream, out, a, b, work, B): a, b, out [B][n][T], powerful basis; out in [0, q_t).  out may
 *   alias a or b, a may equal b.  Launch plan: k_ring_lift a, k_ring_lift b (one launch when a == b),
 *   lolhip_polymul_batch on pQ over B T polynomials, k_ring_fold.
 * lolhip_ringmul_prepare(h, stream, bhat, b, work, Bb): bhat [Bb T][n][K] = crt over pQ of the lifted b [Bb][n][T]
 *   (k_ring_lift, crt).  work is not used (NULL is accepted).
 * lolhip_ringmul_prepared_batch(h, stream, out, a, bhat, Bb, work, B): the same product against a prepared operand,
 *   Bb = B (one per item) or Bb = 1 (one public element against the batch).  Launch plan: k_ring_lift a, crt, pointwise
 *   product with period Bb T n K, crtInv, k_ring_fold.  work as for lolhip_ringmul_batch (half of it is used).
 * The compute calls neither allocate nor synchronise beyond what lolhip_polymul_batch / crt do on pQ.
 * Status, all decided on the host before any launch (outputs are then not written): LOLHIP_ERR_INVALID for NULL
 *   pointers, B < 0, B T >= 2^31, Bb not in {1, B}, a period T n K >= 2^31 with Bb = 1 < B, plans of different indices,
 *   K > 3, T > 16; LOLHIP_ERR_MODULUS when the Q_i are not pairwise distinct or the bound fails; LOLHIP_ERR_NO_CRT
 *   when pQ has no CRT basis; LOLHIP_ERR_NO_DEVICE from the compute calls over host-only plans; LOLHIP_ERR_DEVICE as
 *   elsewhere.  B = 0 is a no-op that returns LOLHIP_OK. */
typedef struct lolhip_ringmul lolhip_ringmul;
LOLHIP_API int lolhip_ringmul_moduli(const lolhip_pp *pps, int npps, const int64_t *qs, int T, int64_t Qs[3]);
LOLHIP_API int lolhip_ringmul_create(const lolhip_plan *pq, const lolhip_plan *pQ, lolhip_ringmul **out);
LOLHIP_API void lolhip_ringmul_destroy(lolhip_ringmul *h);
LOLHIP_API int64_t lolhip_ringmul_work_len(const lolhip_ringmul *h, int64_t B);
LOLHIP_API int lolhip_ringmul_batch(const lolhip_ringmul *h, void *stream, int64_t *out, const int64_t *a,
                                    const int64_t *b, int64_t *work, int64_t B);
LOLHIP_API int lolhip_ringmul_prepare(const lolhip_ringmul *h, void *stream, int64_t *bhat, const int64_t *b,
                                      int64_t *work, int64_t Bb);
LOLHIP_API int lolhip_ringmul_prepared_batch(const lolhip_ringmul *h, void *stream, int64_t *out, const int64_t *a,
                                             const int64_t *bhat, int64_t Bb, int64_t *work, int64_t B);

/* --- RLWE / RLWR instances over moduli without a CRT basis (rlwe_ring_api.cpp, rlwe_ring.hip) -------
 * The instances of lolhip_rlwe_* above for ANY single modulus 2 <= q < 2^62 (2^k, p^e, 105, 500, 900 ...: most of
 * rlwe-challenges' parameter list), where those entries answer LOLHIP_ERR_NO_CRT.  a s is the exact ring product of
 * lolhip_ringmul_* against a prepared secret; the reference computes it through the CRT over C (exact only while
 * n q^2 < 2^53).  Every call takes the RingMul handle h and pq, THE PLAN h WAS CREATED FROM: one modulus (T = 1), the
 * index of h's pQ, the q of h.  A q that has a CRT basis is accepted too.
 * Bases: a [B][n], the secret [n] and the Disc b [B][n] are int64 in the POWERFUL basis, outputs in [0, q); the Cont b
 *   (double [B][n], in [0, q)) and the RLWR b (int64 [B][n], in [0, p)) are in the decoding basis, as above.
 * shat [n][K]: lolhip_ringmul_prepare of the secret with Bb = 1.  lolhip_rlwe_ring_secret draws a uniform secret from
 *   item ctr of domain 7 and writes both s_pow [n] and shat; a caller with its own secret calls lolhip_ringmul_prepare.
 * Stream: a_pow[b][j] is the uniform residue j of item ctr + b of domain 5, the very words lolhip_rlwe_sample_batch
 *   writes to a_crt over a one-modulus plan of the same q, read as powerful-basis coefficients.  Gaussians come from
 *   domain 6 with the bit layout and arithmetic of lolhip_rlwe_sample_batch.  THE CALLER'S DUTY extends unchanged.
 * Semantics, with x = the decoding-basis residues in [0, q) of a s (the exact product, then lInv over pq):
 *   Disc sample  b = (a s + l(e)) mod q, e the integers lolhip_rlwe_sample_batch draws for (index, svar, key, ctr + b):
 *                e does not depend on q, a or s.
 *   Disc error   e = the lift of lInv(b - a s) mod q, a residue r lifting to r when 2 r < q, else r - q (RingMul's
 *                convention, the reference's lift); b is any int64 taken mod q.  norm as lolhip_gsqnorm_batch.
 *   Cont sample / error   exactly the double operations stated above on (x, g) and (x, b); norm as
 *                lolhip_gsqnorm_f64_batch.
 *   RLWR rounded product / check   the rounding stated above on x, 2 <= p < q.
 * Launch plans (la: the lifted a, [B][n][K]):
 *   way in   sample: k_rr_draw_lift (a_pow and la in one pass); a given: k_ring_lift.
 *   product  crt on pQ, the pointwise product with shat (period n K), crtInv on pQ.
 *   way out  k_rr_fold: the fold of k_ring_fold with a tail in registers.  At a 2-power index (L, lInv and the Gaussian
 *            map are identities) the tail finishes the call: + the rounded Gaussian drawn in the pass (Disc sample),
 *            b - fold then the lift (Disc error), the RRq add of a Gaussian drawn in the pass (Cont sample), the Cont
 *            error, the RLWR rounding.  Elsewhere: Disc sample  the sampler of errorRounded -> l on pq -> k_rr_fold
 *            (+ addend);  Disc error  k_rr_fold (b - fold) -> lInv on pq -> k_rr_centre -> gSqNorm;  Cont and RLWR
 *            k_ring_fold -> lInv on pq -> the element-wise passes of lolhip_rlwe_*.  The RLWR check always ends in
 *            lInv and the counting pass.  Debug switch RLWE_RING_UNFUSED forces the second form at a 2-power index; both
 *            give the same bits.
 * work: lolhip_rlwe_ring_work_len(h, pq, kind, B) int64 of device scratch, 16-byte aligned:
 *   even(B n K) + even(B n) + (kind == 2 ? 0 : even(B n)), even(x) = x rounded up to an even count.  It answers on
 *   host-only handles and serves the sample, error and rounding calls of that kind alike.
 * Limits: T = 1; for Disc and Cont the sampler's index limits of lolhip_encrypt_batch; n <= 16384 for norm_out; the
 *   size limits of lolhip_ringmul_prepared_batch.
 * Status, decided on the host in this order before any launch (outputs are then not written): LOLHIP_ERR_INVALID for a
 *   NULL h or pq, an unknown kind, B < 0 or beyond RingMul's limits, a pq that is not h's plan (index, T != 1, q), p
 *   outside [2, q), svar <= 0 or not finite, an index beyond the sampler's limits (Disc and Cont);
 *   LOLHIP_ERR_NO_DEVICE over host-only plans; LOLHIP_ERR_DEVICE as elsewhere; LOLHIP_ERR_INVALID for NULL pointers at
 *   B > 0 (e_out or norm_out may be NULL, not both; norm_out needs n <= 16384).  B = 0 returns LOLHIP_OK.  No call
 *   allocates or synchronises beyond what crt on pQ does; output does not depend on how a batch is split.
 * With the environment variable LOLHIP_RLWE_RING_INFO set (read at every call) each call that launches prints one line
 *   to stderr: "rlwe_ring: <entry> kind <kind>, route <fused|unfused>, K <K>, n <n>, B <B>". */
LOLHIP_API int64_t lolhip_rlwe_ring_work_len(const lolhip_ringmul *h, const lolhip_plan *pq, int kind, int64_t B);
LOLHIP_API int lolhip_rlwe_ring_secret(const lolhip_ringmul *h, const lolhip_plan *pq, void *stream, const uint8_t key[32],
                                       uint64_t ctr, int64_t *s_pow, int64_t *shat);
LOLHIP_API int lolhip_rlwe_ring_sample_batch(const lolhip_ringmul *h, const lolhip_plan *pq, void *stream, int kind, int64_t p,
                                             const int64_t *shat, double svar, const uint8_t key[32], uint64_t ctr,
                                             int64_t *a_pow, void *b_out, int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwe_ring_error_batch(const lolhip_ringmul *h, const lolhip_plan *pq, void *stream, int kind,
                                            const int64_t *a_pow, const void *b, const int64_t *shat, void *e_out,
                                            void *norm_out, int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwr_ring_rounded_prod_batch(const lolhip_ringmul *h, const lolhip_plan *pq, int64_t p, void *stream,
                                                   const int64_t *a_pow, const int64_t *shat, int64_t *b_out,
                                                   int64_t *work, int64_t B);
LOLHIP_API int lolhip_rlwr_ring_check_batch(const lolhip_ringmul *h, const lolhip_plan *pq, int64_t p, void *stream,
                                            const int64_t *a_pow, const int64_t *b, const int64_t *shat, int32_t *mismatch,
                                            int64_t *work, int64_t B);

/* --- whole RLWE / RLWR challenges (challenge_api.cpp, challenge.hip; rlwe-challenges Generate.hs:105-218,
 * Verify.hs:236-366), device pointers -----------------------------------------------------------------
 * A challenge is I instances of L samples, each instance under a secret of its own.  One call generates all of it and
 * one call verifies all of it; item b = i L + l (sample l of instance i) uses secret i = b / L.  kind, p, svar and the
 * arithmetic of every sample are those of lolhip_rlwe_* above.  These entries serve moduli WITH a CRT basis.
 * Bases: every array is in the DECODING basis, the basis of the wire format (Cyc.hs toProto): s [I][n][T],
 *   a [I L][n][T], residues in [0, q_t); b int64 [I L][n][T] residues (Disc), double [I L][n] in [0, q) (Cont), int64
 *   [I L][n] in [0, p) (RLWR).
 * lolhip_chall_generate_batch.  THE STREAM CONTRACT: secret i is what lolhip_rlwe_secret gives at counter ctr_s + i;
 *   sample (i, l) is what lolhip_rlwe_sample_batch gives for that secret at counter ctr + i L + l; s, a and the Disc b
 *   are then taken to the decoding basis with crtInv and lInv.  THE CALLER'S DUTY extends: a call uses the items
 *   ctr_s .. ctr_s + I - 1 of domain 7 and ctr .. ctr + I L - 1 of domains 5 and 6.
 *   Launch plan: the I secrets in one launch -> the plan of lolhip_rlwe_sample_batch over I L items, the pass with the
 *   secret (k_chall_uniform) reading row b / L -> crtInv, lInv of the outputs.
 * lolhip_chall_verify_batch.  Per instance i, over its L samples under s_dec[i]:
 *     Disc  fails[i] = #{l : not (bound_disc > norm)}, worst[i] = the largest norm, int64; norm as
 *           lolhip_rlwe_error_batch gives it, so a saturated norm (INT64_MAX) fails under every bound
 *     Cont  the same with bound_cont in doubles, worst double; a NaN norm fails and makes worst[i] NaN
 *     RLWR  fails[i] = #{l : a coefficient of sample l mismatches}, worst[i] = the largest per-sample mismatch count of
 *           lolhip_rlwr_check_batch, int64
 *   The comparison is strict (Verify.hs:350-356).  fails int32 [I]; an instance is valid when fails[i] = 0.  Only the
 *   bound of the kind is read.  Inputs are any int64 (taken mod q_t) and are not written.
 *   Launch plan: l, crt of s, a (and the Disc b) into work -> k_chall_as (a s_i, or b - a s_i) -> crtInv, lInv -> the
 *   error and norm passes of lolhip_rlwe_error_batch, or the counting pass of lolhip_rlwr_check_batch ->
 *   k_chall_verdict, one wave per instance, no atomics.
 * work: lolhip_chall_work_len(pq, kind, I, L) int64 of device scratch (any 8-byte alignment), with B = I L and even(x) = x
 *   rounded up to an even count:  even(I n T) + even(B n T) + (kind == 0 ? even(B n T) : 0) + (kind == 2 ? 0 :
 *   even(B n)) + even(B).  It answers on host-only plans and serves both calls.
 * Limits: I >= 0, L >= 1, I L <= 2^31 - 1; T <= 16, T = 1 for Cont and RLWR; 2 <= p < q; generate: the sampler's index
 *   limits for Disc and Cont; verify: n <= 16384 for Disc and Cont.
 * Status, decided on the host in this order before any launch (outputs are then not written): LOLHIP_ERR_INVALID for a
 *   NULL pq, an unknown kind, I < 0, L < 1, I L too large, T beyond the limits, p outside [2, q), svar <= 0 or not
 *   finite, an index beyond the limits; LOLHIP_ERR_NO_CRT when pq has no CRT basis; LOLHIP_ERR_MODULUS for a Disc
 *   verification over moduli that are not pairwise coprime; LOLHIP_ERR_NO_DEVICE on a host-only plan;
 *   LOLHIP_ERR_INVALID for NULL pointers at I > 0.  I = 0 returns LOLHIP_OK.  No call synchronises or allocates. */
LOLHIP_API int64_t lolhip_chall_work_len(const lolhip_plan *pq, int kind, int64_t I, int64_t L);
LOLHIP_API int lolhip_chall_generate_batch(const lolhip_plan *pq, void *stream, int kind, int64_t p, double svar,
                                           const uint8_t key[32], uint64_t ctr_s, uint64_t ctr, int64_t I, int64_t L,
                                           int64_t *s_out, int64_t *a_out, void *b_out, int64_t *work);
LOLHIP_API int lolhip_chall_verify_batch(const lolhip_plan *pq, void *stream, int kind, int64_t p, int64_t bound_disc,
                                         double bound_cont, int64_t I, int64_t L, const int64_t *s_dec,
                                         const int64_t *a_dec, const void *b, int32_t *fails, void *worst, int64_t *work);

/* lolhip_chall_ring_*: the same two calls for ANY single modulus 2 <= q < 2^62, on the plans of lolhip_rlwe_ring_*
 * above: h the RingMul handle, pq the plan h was created from (T = 1).  Arrays, kinds, verdicts and bounds exactly as
 * for lolhip_chall_*: everything in the DECODING basis, s [I][n], a [I L][n].
 * THE STREAM CONTRACT: secret i is the s_pow of lolhip_rlwe_ring_secret at counter ctr_s + i; sample (i, l) is what
 *   lolhip_rlwe_ring_sample_batch gives for its shat at counter ctr + i L + l; s, a and the Disc b are then taken from
 *   the powerful to the decoding basis with lInv on pq.
 * Launch plans: generate  k_rr_draw_lift of the I secrets, crt on pQ -> k_rr_draw_lift of a -> crt on pQ, k_chall_as
 *   over rows of n K words (the product with shat_(b / L)), crtInv on pQ -> the way out of
 *   lolhip_rlwe_ring_sample_batch (the fused tails of k_rr_fold at a 2-power index: they do not read the secret) ->
 *   lInv.  verify  l on pq of s, a (and the Disc b) -> k_ring_lift of both, crt on pQ -> the same product -> the way
 *   out of lolhip_rlwe_ring_error_batch, or k_ring_fold, lInv and the counting pass (RLWR) -> k_chall_verdict.
 * work: lolhip_chall_ring_work_len(h, pq, kind, I, L) int64 of device scratch, 16-byte aligned, B = I L:
 *   even(I n K) + even(B n K) + even(B n) + (kind == 2 ? 0 : even(B n)) + even(I n) + even(B n) +
 *   (kind == 0 ? even(B n) : 0) + even(B).
 * Limits and status as for lolhip_rlwe_ring_* with I, L in place of B (I >= 0, L >= 1, I L <= 2^31 - 1, and n K <= 2^31 - 1
 *   whatever the item count, work_len included); verify needs
 *   the sampler's index limits and n <= 16384 for Disc and Cont.  I = 0 returns LOLHIP_OK. */
LOLHIP_API int64_t lolhip_chall_ring_work_len(const lolhip_ringmul *h, const lolhip_plan *pq, int kind, int64_t I, int64_t L);
LOLHIP_API int lolhip_chall_ring_generate_batch(const lolhip_ringmul *h, const lolhip_plan *pq, void *stream, int kind,
                                                int64_t p, double svar, const uint8_t key[32], uint64_t ctr_s, uint64_t ctr,
                                                int64_t I, int64_t L, int64_t *s_out, int64_t *a_out, void *b_out,
                                                int64_t *work);
LOLHIP_API int lolhip_chall_ring_verify_batch(const lolhip_ringmul *h, const lolhip_plan *pq, void *stream, int kind,
                                              int64_t p, int64_t bound_disc, double bound_cont, int64_t I, int64_t L,
                                              const int64_t *s_dec, const int64_t *a_dec, const void *b, int32_t *fails,
                                              void *worst, int64_t *work);

/* --- the messages of rlwe-challenges (wire.cpp; lol/RLWE.proto, rlwe-challenges/Challenges.proto), host pointers ------
 * Readers and writers with the two-pass / capacity convention of the wire entries below: a writer with out = NULL
 * returns the length; a reader with NULL arrays answers the sizes.  kind: 0 = Disc, 1 = Cont, 2 = RLWR.
 * The parameters of a kind travel as ip [4] = (m, q, x, numSamples), x = the int64 bound (Disc), unused (Cont) or p
 * (RLWR), and dp [2] = (svar, the double bound of Cont); RLWRParams has no svar.
 * lolhip_challenge_*: Challenge, hdr [4] = (challengeID, numInstances, beaconEpoch, beaconOffset) and the params oneof
 *   (fields 5 / 6 / 7 = Cont / Disc / RLWR).  Returns 0 (read) or the length (write).
 * lolhip_instance_*: Instance{Cont,Disc,RLWR} and their Product forms.  ids [2] = (challengeID, instanceID); a
 *   [L][n][T] canonical residues, decoding basis; b [L][n][T] residues mod q_t (Disc) or mod p (RLWR, T = 1), or doubles
 *   (Cont).  The reader takes both generations, as readInstanceU does (Verify.hs:199-232): it tells them apart by the
 *   wire type of field 1 of the ring elements (varint m: legacy Rq / Kq; length-delimited rqlist: Product) and reports
 *   product_out = 0 / 1; it returns n and count_out = L.  The writer emits the Product forms (what Generate.hs writes);
 *   legacy != 0 selects the forms of the 2016 release (T = 1).  The moduli of an element must be the q of its
 *   parameters (one modulus, or a tuple whose product is q); the RLWR b is over p.
 * lolhip_secret_*: Secret / SecretProduct: ids, m, q, the seed bytes and s [n][T].  Returns n (read) or the length.
 * Unknown fields are skipped.  LOLHIP_ERR_INVALID for truncated or malformed data, a missing required field, samples of
 *   mixed generations or shapes, an m or q of an element that disagrees with its parameters, a capacity too small;
 *   LOLHIP_ERR_MODULUS for a modulus outside [2, 2^62). */
LOLHIP_API int64_t lolhip_challenge_read(const uint8_t *buf, int64_t len, int64_t *hdr, int *kind_out, int64_t *ip, double *dp);
LOLHIP_API int64_t lolhip_challenge_write(const int64_t *hdr, int kind, const int64_t *ip, const double *dp, uint8_t *out,
                                          int64_t cap);
LOLHIP_API int64_t lolhip_instance_read(const uint8_t *buf, int64_t len, int kind, int64_t *ids, int64_t *ip, double *dp,
                                        int *product_out, int *T_out, int64_t *qs, int cap_T, int64_t *count_out, int64_t *a,
                                        int64_t cap_a, void *b, int64_t cap_b);
LOLHIP_API int64_t lolhip_instance_write(int kind, int legacy, const int64_t *ids, const int64_t *ip, const double *dp,
                                         const int64_t *qs, int T, int64_t L, int64_t n, const int64_t *a, const void *b,
                                         uint8_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_secret_read(const uint8_t *buf, int64_t len, int64_t *ids, int64_t *m_out, int64_t *q_out,
                                      uint8_t *seed, int64_t cap_seed, int64_t *seed_len_out, int *product_out, int *T_out,
                                      int64_t *qs, int cap_T, int64_t *xs, int64_t cap_xs);
LOLHIP_API int64_t lolhip_secret_write(int legacy, const int64_t *ids, int64_t m, int64_t q, const uint8_t *seed,
                                       int64_t seed_len, const int64_t *qs, int T, const int64_t *xs, int64_t n, uint8_t *out,
                                       int64_t cap);

/* --- gadget error correction (gadget_api.cpp, gadget.hip) ----------------------------------------------------------
 * Correct gad (Cyc t m zq) (Cyc.hs:615-621 over Gadget.hs:84-134 and ZqBasic.hs:234-314), the inverse direction of
 * lolhip_gadget / lolhip_decompose_batch: from L = lolhip_decompose_len(p, base) noisy multiples xs_j = g_j s + e_j of
 * the gadget it recovers u (= s when the e_j are small) and the L integer error polynomials, coefficient by coefficient
 * in the DECODING basis.  base as for lolhip_decompose_batch (0 = TrivGad, b >= 2 = BaseBGad b).  Defined for every
 * input, an encoding or not.  For one modulus q, k = gadlen(b, q) digits, v_i the centred lift of entry i and
 * divModCent (a, d) = floor ((a + floor (d/2)) / d):
 *     w_i = divModCent (b v_i - v_(i+1), q) (i < k-1),  x = sum_i w_i floor (q / b^(i+1)),
 *     y_0 = x, y_(i+1) = b y_i - q w_i,  v' = v - y,  s = divModCent (v'_(k-1), b^(k-1)),  e_i = v'_i - s b^i,
 *     u = xs_0 - e_0 mod q;                     k = 1 and TrivGad: u = xs_0, e = [0].
 * A pair (q_a, q_b) carries the gadget g_a x (1, 0) ++ g_b x (0, 1) (the rows of lolhip_gadget): a row (a, beta) of the
 * first block has x = lift beta and the entry q_b^-1 (a - x) mod q_a to correct over q_a, its error is x + q_b e'; the
 * second block the same with the roles swapped; u = (q_b u'_a mod q_a, q_a u'_b mod q_b).
 * T = 1 or 2 (the class instance is for fields and pairs of fields).
 * Domain: with h = floor (q/2), W = max (floor ((b+2) h / q), ceil (b h / q)) >= |w_i|,
 *     Y_i = W (sum_{j<i} b^(i-1-j) (q mod b^(j+1)) + b^i sum_{i<=j<k-1} floor (q / b^(j+1))) >= |y_i|   (Y_0 >= |x|),
 *     S = floor ((h + Y_(k-1) + ceil (b^(k-1) / 2)) / b^(k-1)) >= |s|,   E = max_i (h + Y_i + S b^i) >= |v'_i|, |e_i|,
 * every modulus with k >= 2 needs E + b^(k-1) < 2^63 and, in a pair, h_other + q_other E < 2^63 (with k = 1 the errors
 * of its block are the x alone); anything else is refused with LOLHIP_ERR_MODULUS.  Inside the domain every value is
 * exact: the kernel's 64-bit sums wrap, and a wrapped sum whose true value fits is that value.
 * lolhip_gadget_correct_work_len(p, base, basis, B): int64 words of device scratch: 0 for LOLHIP_BASIS_DEC, L B n T for
 *   LOLHIP_BASIS_POW / LOLHIP_BASIS_CRT (the copy the basis change runs on).  Negative status on error.
 * lolhip_gadget_correct_batch(p, stream, xs, base, basis, u_dec, es_dec, work, B): xs [L][B][n][T], any int64 taken
 *   mod q_t, in `basis`; for POW the copy in work goes through lInv, for CRT through crtInv and lInv (one launch plan
 *   over L B polynomials each), then k_gadget_correct runs once.  u_dec [B][n][T] in [0, q_t), es_dec [L][B][n] int64 or
 *   NULL (no error is stored, u is the same).  u_dec and es_dec must not overlap xs.
 * lolhip_gadget_encode_batch(p, stream, s, base, e, out, B): Gadget.encode plus noise, out_j = g_j s + reduce (e_j):
 *   s [B][n][T] (any int64 mod q_t), e [L][B][n] int64 or NULL (no noise), out [L][B][n][T] in [0, q_t); any T <= 16
 *   and any basis (s and the e_j in the same one).
 * Status, all decided on the host before any launch (outputs are then not written): LOLHIP_ERR_INVALID for a NULL plan,
 *   base 1 or negative, T > 2 (correct) or T > 16 (encode), an unknown basis, B < 0, NULL pointers (es_dec, e and a
 *   zero-length work excepted) with B > 0; LOLHIP_ERR_MODULUS for moduli of a pair that are not coprime
 *   and for tuples outside the domain above; LOLHIP_ERR_NO_CRT for LOLHIP_BASIS_CRT on a plan without a CRT basis;
 *   LOLHIP_ERR_NO_DEVICE on a host-only plan; LOLHIP_ERR_DEVICE as elsewhere.  B = 0 is a no-op returning LOLHIP_OK.
 *   The calls neither allocate nor synchronise. */
enum { LOLHIP_BASIS_DEC = 0, LOLHIP_BASIS_POW = 1, LOLHIP_BASIS_CRT = 2 };
LOLHIP_API int64_t lolhip_gadget_correct_work_len(const lolhip_plan *p, int64_t base, int basis, int64_t B);
LOLHIP_API int lolhip_gadget_correct_batch(const lolhip_plan *p, void *stream, const int64_t *xs, int64_t base, int basis,
                                           int64_t *u_dec, int64_t *es_dec, int64_t *work, int64_t B);
LOLHIP_API int lolhip_gadget_encode_batch(const lolhip_plan *p, void *stream, const int64_t *s, int64_t base,
                                          const int64_t *e, int64_t *out, int64_t B);

/* --- host-pointer convenience (H2D, run, D2H on an internal stream) --------------
 * op: see LOLHIP_OP_*.  y (and b for MUL/POLYMUL) are host arrays of B polynomials. */
enum {
  LOLHIP_OP_CRT = 0, LOLHIP_OP_CRTINV = 1, LOLHIP_OP_MUL = 2, LOLHIP_OP_POLYMUL = 3,
  LOLHIP_OP_L = 4, LOLHIP_OP_LINV = 5, LOLHIP_OP_MULGPOW = 6, LOLHIP_OP_MULGDEC = 7,
  LOLHIP_OP_DIVGPOW = 8, LOLHIP_OP_DIVGDEC = 9, LOLHIP_OP_MULGCRT = 10, LOLHIP_OP_DIVGCRT = 11
};
LOLHIP_API int lolhip_op_host(const lolhip_plan *p, int op, int64_t *y, const int64_t *b, int64_t B);
enum {
  LOLHIP_EXT_TWACE_POWDEC = 0, LOLHIP_EXT_TWACE_CRT = 1, LOLHIP_EXT_EMBED_POW = 2,
  LOLHIP_EXT_EMBED_DEC = 3, LOLHIP_EXT_EMBED_CRT = 4, LOLHIP_EXT_COEFFS = 5
};
LOLHIP_API int lolhip_ext_host(const lolhip_ext *x, int op, int64_t *out, const int64_t *in, int64_t B);
/* The host-pointer calls (and the drop-in symbols, which go through them) check a staging set — one stream, a
 * pinned staging area and two device buffers, grown on demand — out of a process-wide pool for the duration of
 * the call: the steady state of a call is memcpy, H2D, kernels, D2H and a wait on that set's stream — no
 * allocation, no device-wide synchronisation.  The pool holds as many sets as calls have run concurrently; sets
 * belong to no thread, so exiting worker threads leave nothing behind.  This frees every idle set (optional;
 * e.g. to hand the memory back between phases).  The name dates from round 2, when the sets were per thread. */
LOLHIP_API void lolhip_thread_release(void);

/* --- L, L^-1, mulG, divG over Z, R and C, and mulC (eltops_api.cpp, eltops.hip) ------------------------
 * The Tensor members l, lInv, mulGPow, mulGDec, divGPow, divGDec for the element types that are not Z_q (tensorL{R,Double,
 * C}, tensorLInv*, tensorG{Pow,Dec}{R,C}, tensorGInv{Pow,Dec}{R,C} of l.cpp / g.cpp), in place on a device slab
 * y [B][n][T] with the T components innermost (the reference's tupSize).  elt: LOLHIP_ELT_I64 int64, LOLHIP_ELT_F64
 * double, LOLHIP_ELT_C64 complex double stored (re, im): every op is a real-linear map applied componentwise, so a C64
 * slab is run as an F64 slab of 2 T components.  The index is the plan's; its moduli play no role.  op is one of
 * LOLHIP_OP_L ... LOLHIP_OP_DIVGDEC.  The structure is tensorFuserPrime's (tensor.h:39-74): the plan's prime powers in
 * order, the first fastest-varying, p^e as I_lts (x) A_p (x) I_rts with p^(e-1) folded into lts, p = 2 the identity.
 * Per (p-1)-vector every op runs the recurrence of the reference in its order (l.cpp:28-57, 67-98; g.cpp:16-35, 37-58,
 * 60-90, 92-123); divG then divides by oddrad = the product of the odd primes of m.
 *   I64  arithmetic mod 2^64.  divG: ok[b] = 1 and item b holds the exact quotients when every coefficient of the
 *        transform (as a wrapped int64) is divisible by oddrad; otherwise ok[b] = 0 and item b holds the undivided
 *        transform (nothing is truncated).  m a power of two: ok[b] = 1, data untouched.  ok is int32 [B], required for
 *        divG over I64 and ignored (may be NULL) everywhere else.
 *   F64 / C64  every IEEE operation rounded on its own, in the reference's order (no contraction): L, LInv, mulGPow,
 *        mulGDec equal the reference bit for bit.  divG is the reference's transform and then y / (double) oddrad; it
 *        always succeeds.  (The reference's own tensorGInv*R invert the divisibility test and tensorGInv*C scale by the
 *        integer quotient 1 / oddrad = 0: g.cpp:169-184, 209-237, 262-273.)
 * One launch reads and writes every word once while n T (2 T for C64) words fit the 160 KiB of LDS; larger items take one
 * pass over the slab per odd prime straight from HBM (debug switch ELT_GLOBAL forces that route; both give the same
 * bits).  Primes of any size; a (p-1)-vector is one thread's sequential work, so large primes run slowly.
 * lolhip_mulc_batch: a[i] *= b[i] over count complex doubles (mulC, types.h:146-152): re = a_re b_re - a_im b_im,
 * im = a_re b_im + a_im b_re, each product and sum rounded on its own.  b may equal a.
 * Status, decided on the host before any launch, in this order: LOLHIP_ERR_INVALID for a NULL plan, an unknown op or
 * elt, T < 1 or T > 16, B < 0 or n > 16384 (mulc: count < 0); LOLHIP_ERR_NO_DEVICE on a host-only plan (mulc: without a
 * device), LOLHIP_ERR_DEVICE as elsewhere; LOLHIP_ERR_INVALID for NULL y with B > 0 or NULL ok for divG over I64 with
 * B > 0 (mulc: NULL a or b with count > 0).  B = 0 (count = 0) returns LOLHIP_OK with nothing launched.  No call
 * synchronises or allocates; the result does not depend on how a batch is split.
 * With the environment variable LOLHIP_ELT_INFO set (read at every call) each lolhip_elt_op_batch that launches prints
 * one line to stderr: "k_elt: route <lds|global>, op <op>, word <u64|f64>, n <n>, W <words per coefficient>, lds <bytes> B". */
enum { LOLHIP_ELT_I64 = 0, LOLHIP_ELT_F64 = 1, LOLHIP_ELT_C64 = 2 };
LOLHIP_API int lolhip_elt_op_batch(const lolhip_plan *p, void *stream, int op, int elt, int T, void *y, int32_t *ok,
                                   int64_t B);
LOLHIP_API int lolhip_mulc_batch(void *stream, double *a, const double *b, int64_t count);

/* --- wire format: Lol's protobuf ring elements, host side -------
 * message Rq { uint32 m = 1; uint64 q = 2; repeated sint64 xs = 3; }   (lol/Lol.proto)
 * message RqProduct { repeated Rq rqlist = 1; }
 * One Rq per RNS modulus, first component first; xs are decoding-basis coefficients written
 * as centred lifts (IZipVector.hs:127-205).  Ingest = read -> [n][T] slab -> l -> crt.
 * read : returns n (coefficients per modulus); fills m, T, qs[T] and, when xs != NULL, the
 *        reduced residues xs[j*T + t] in [0, q_t).  Pass xs = NULL to query sizes.
 * write: returns the number of bytes (needed when out == NULL, written otherwise); xs as
 *        above (any representative in (-q, q)).  Unpacked sint64 encoding (proto2 default);
 *        the reader also accepts the packed form.  Negative return = LOLHIP_ERR_*. */
LOLHIP_API int64_t lolhip_rqproduct_read(const uint8_t *buf, int64_t len, uint32_t *m, int64_t *qs, int cap_T,
                                         int *T, int64_t *xs, int64_t cap_xs);
LOLHIP_API int64_t lolhip_rqproduct_write(uint32_t m, const int64_t *qs, int T, const int64_t *xs, int64_t n,
                                          uint8_t *out, int64_t cap);

/* KSHint (lol-apps/SHE.proto: repeated RqPolynomial hint = 1; TypeRep gad = 2; RqPolynomial =
 * repeated RqProduct coeffs, constant coefficient first): the L hint polynomials of K
 * coefficients each -> xs [L][K][n][T], decoding basis, canonical residues; l and crt over the
 * L*K polynomials then give the hint slab of lolhip_keyswitch_batch.  Returns n; xs = NULL
 * queries L, K, T, m, qs.  The gadget fingerprint is skipped. */
LOLHIP_API int64_t lolhip_kshint_read(const uint8_t *buf, int64_t len, uint32_t *m, int64_t *qs, int cap_T, int *T,
                                      int *L, int *K, int64_t *xs, int64_t cap_xs);

/* The remaining messages of lol/Lol.proto and lol-apps/SHE.proto, same conventions:
 *  r_read          message R { m = 1; repeated sint64 xs = 2 }: integer coefficients, decoding basis.  Returns n.
 *  secretkey_read  message SecretKey { R sk = 1; double v = 2 } (SHE.proto:9).  Returns n.
 *  kqproduct_read  message KqProduct / Kq (`repeated double xs`): xs [n][T] doubles.  Returns n.
 *  linearrq_read   message LinearRq { e = 1; r = 2; repeated RqProduct coeffs = 3 } (Lol.proto:11): the
 *                  values of an E-linear function on the relative decoding basis, xs [C][n][T]; after l
 *                  and crt, the ys of lolhip_evallin_batch.  Returns n; xs = NULL queries the sizes.
 *  kshint_write    the inverse of kshint_read; gad_a/gad_b = the two words of the TypeRep fingerprint.
 *  tunnelhint_read message TunnelHint (SHE.proto:26): e, r, s, p and the byte ranges (offset, length
 *                  into buf) of the embedded LinearRq and KSHints, for the readers above.  Returns the
 *                  number of KSHints. */
LOLHIP_API int64_t lolhip_r_read(const uint8_t *buf, int64_t len, uint32_t *m, int64_t *xs, int64_t cap_xs);
LOLHIP_API int64_t lolhip_secretkey_read(const uint8_t *buf, int64_t len, uint32_t *m, double *v, int64_t *xs, int64_t cap_xs);
LOLHIP_API int64_t lolhip_kqproduct_read(const uint8_t *buf, int64_t len, uint32_t *m, int64_t *qs, int cap_T, int *T,
                                         double *xs, int64_t cap_xs);
LOLHIP_API int64_t lolhip_linearrq_read(const uint8_t *buf, int64_t len, uint32_t *e, uint32_t *r, int *C, uint32_t *m,
                                        int64_t *qs, int cap_T, int *T, int64_t *xs, int64_t cap_xs);
LOLHIP_API int64_t lolhip_kshint_write(uint32_t m, const int64_t *qs, int T, int L, int K, const int64_t *xs, int64_t n,
                                       uint64_t gad_a, uint64_t gad_b, uint8_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_tunnelhint_read(const uint8_t *buf, int64_t len, uint32_t *e, uint32_t *r, uint32_t *s, uint64_t *p,
                                          int64_t *func_off, int64_t *func_len, int64_t *hint_off, int64_t *hint_len,
                                          int cap_hints);

/* Round 3: the remaining writers (same conventions as the readers above; out = NULL queries the size) and the chain
 * messages of lol-apps/HomomPRF.proto:18-26 (LinearFuncChain, TunnelHintChain, RoundHintChain: `repeated X = 1`).
 *  r_write / secretkey_write   message R / SecretKey from integer decoding-basis coefficients xs[n] (and the variance v)
 *  linearrq_write              message LinearRq from xs [C][n][T] (decoding-basis residues of the output ring m)
 *  tunnelhint_write            message TunnelHint from an encoded LinearRq, nh encoded KSHints and e, r, s, p
 *  chain_read                  number of elements + byte ranges (offset, length into buf) of up to cap of them
 *  chain_write                 the chain message of `count` encoded elements */
LOLHIP_API int64_t lolhip_r_write(uint32_t m, const int64_t *xs, int64_t n, uint8_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_secretkey_write(uint32_t m, double v, const int64_t *xs, int64_t n, uint8_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_linearrq_write(uint32_t e, uint32_t r, uint32_t m, const int64_t *qs, int T, int C, const int64_t *xs,
                                         int64_t n, uint8_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_tunnelhint_write(const uint8_t *func, int64_t func_len, const uint8_t *const *hints, const int64_t *hint_len,
                                           int nh, uint32_t e, uint32_t r, uint32_t s, uint64_t p, uint8_t *out, int64_t cap);
LOLHIP_API int64_t lolhip_chain_read(const uint8_t *buf, int64_t len, int64_t *off, int64_t *elem_len, int cap);
LOLHIP_API int64_t lolhip_chain_write(const uint8_t *const *elems, const int64_t *elem_len, int count, uint8_t *out, int64_t cap);

/* Measurement aid: device-to-device copy of `bytes` (a multiple of 16; both pointers 16-byte aligned) with
 * 16 bytes per lane — the read-once/write-once ceiling bench.py quotes beside every HBM-bound leg.
 * variant 0: one tile per workgroup; 1: persistent workgroups. */
LOLHIP_API int lolhip_copy_slab(void *stream, void *dst, const void *src, int64_t bytes, int variant);

/* Test and A/B aid, not part of the drop-in surface: force a launch path.  `name` is one of
 * GENERIC_SCALAR, NO_FUSED2, NO_POW2_PART, POLYMUL_UNFUSED, KEYSWITCH_UNFUSED, NO_T1, NO_PIPE, FORCE_PIPE, NO_OWN_DIAG, NO_MERGE, NO_KRON, NO_LAZY (these four read when a plan is built), NO_TRUNC, ELT_GLOBAL, LPRF_VALU, RLWE_RING_UNFUSED and GAUSS_DENSE (read when a plan is built: every odd prime of a plan created with LOLHIP_PLAN_DENSE_GAUSS takes the dense stage of the Gaussian map), and ZQ_DENSE_VALU (read at launch: a plan created with LOLHIP_ROUTE_DENSE_ZQ takes the vector-ALU form of its dense stages where it would take the matrix cores) and ZQ_DENSE_MFMA (read at launch: such a plan takes the matrix cores wherever its moduli fit, however short the dense vectors; ZQ_DENSE_VALU wins over it) (each is
 * also read ONCE at first use from the environment variable LOLHIP_<name>); value 0 restores the
 * default path.  Every path computes the same residues.  Returns LOLHIP_OK or LOLHIP_ERR_INVALID.
 * Two environment variables are test hooks of the persistent pipelined poly-mul, read at EVERY launch of it:
 *   LOLHIP_PIPE_GRID=<G>  its grid is G workgroups (clamped to the batch) instead of the resident-workgroup count;
 *   LOLHIP_PIPE_INFO      (set to anything) each launch prints one line to stderr, before the grid is clamped:
 *                         "k_pow2_pipe<L,AR>: lds <bytes> B, per_cu <w>, occupancy query <o> (err <e>), grid <G>".
 * One more is read at every launch of the Gaussian map:
 *   LOLHIP_GAUSS_INFO     (set to anything) each launch prints one line to stderr naming the route of every stage:
 *                         "k_gauss: n <n>, B <B>, stages reg" for a program of register stages, else
 *                         "k_gauss_dense: n <n>, B <B>, items <I>, bufs <1|2>, lds <bytes> B, grid <G>, stages <route> ...",
 *                         route one of reg, dense-rows (lanes along the rows, stride < 64), dense-cols (lanes along r).
 * Two are read at every launch of the dense Z_q stages (plans created with LOLHIP_ROUTE_DENSE_ZQ):
 *   LOLHIP_ZQ_DENSE_INFO  (set to anything) each launch prints one line to stderr:
 *                         "k_zq_dense: route <r>, W <W>, n <n>, B <B>, T <T>, word <4|8>, items <I>, lds <bytes> B, grid <G>, polymul <0|1>, stages <kind> ...",
 *                         kind one of elt (element-wise), dense-rows (lanes along the rows, stride < 64), dense-cols
 *                         (lanes along r); the one-launch poly-mul lists the forward program, "*", the inverse program;
 *   LOLHIP_ZQ_DENSE_GRID=<G>  the grid is G workgroups (at least 1) instead of one per (tile, component), so that a
 *                         small batch exercises the grid-stride loop.
 * ZQ_SCAN is one more name for lolhip_debug_set (read at launch: see lolhip_plan_scan_route), and two more variables are
 * read at every launch of the scan kernel (plans created with LOLHIP_ROUTE_SCAN_ZQ):
 *   LOLHIP_ZQ_SCAN_INFO   (set to anything) each launch prints one line to stderr:
 *                         "k_zq_scan: n <n>, B <B>, T <T>, word <4|8>, items <I>, lds <bytes> B, grid <G>, threads <t>, stages <kind>:<p>:<d>:<rts>:<layout> ...",
 *                         kind one of l, linv, gpow, gdec, ginvpow, ginvdec, diag; layout one of lanes (stride below a
 *                         wave: the wave scans across lanes), cols (a lane walks one column), elt (element-wise);
 *   LOLHIP_ZQ_SCAN_GRID=<G>  the grid is G workgroups (at least 1) instead of one per (tile, component). */
LOLHIP_API int lolhip_debug_set(const char *name, int value);

/* number of HIP devices visible (0 without a GPU); never initialises a context */
LOLHIP_API int lolhip_device_count(void);
LOLHIP_API const char *lolhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LOLHIP_H */
