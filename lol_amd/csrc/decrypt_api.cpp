// lol_amd/csrc/decrypt_api.cpp — the C ABI of SymmSHE errorTerm / decrypt (include/lolhip.h; lol-apps
// SymmSHE.hs:153-178): host checks, the p-dependent lift constants and the launch plan over the kernels of
// decrypt.hip and the existing transforms.
#include <hip/hip_runtime_api.h>

#include "she_host.h"

using namespace lolhip;

// ---- errorTerm / decrypt (lol-apps SymmSHE.hs:153-178) ---------------------------------------
namespace {

// host checks shared by both entries and the lift's p-dependent constants.  enc: 0 LSD, 1 MSD; p: the plaintext
// modulus; l: the ciphertext's scalar (decrypt only; l' = l, or l (-Q)^-1 mod p for MSD: msdToLSD, Prelude.hs:311-315)
int decrypt_setup(const Plan& P, int ncs, int enc, int64_t p, int64_t l, LiftParams& lp) {
  if (ncs < 1 || (enc != 0 && enc != 1) || P.T > PIPE_MAX_T) return LOLHIP_ERR_INVALID;
  if (!P.has_crt) return LOLHIP_ERR_NO_CRT;
  if (!p_ok(p) || !P.lift_ok) return LOLHIP_ERR_MODULUS;
  const u64 up = (u64)p;
  lp = LiftParams();
  lp.T = P.T;
  lp.msd = enc;
  lp.mp = make_modctx(up);
  u64 prefix = 1 % up;
  for (int t = 0; t < P.T; ++t) {
    lp.pw[t] = prefix;
    prefix = mulmod(prefix, P.qs[(size_t)t] % up, up);
  }
  lp.qp = prefix;
  u64 zp = 1;
  if (enc == 1) {                                              // msdToLSD: p mod q_t on the residues, (-Q)^-1 mod p on l
    const int rc = encode_scales(P, p, false, lp.scale, &zp); if (rc) return rc;
  }
  lp.lp = encode_l(l, zp, up);
  return LOLHIP_OK;
}

// c(s) over B ciphertexts, ready for the lift: *v a decoding-basis slab [B][n][T] and *add a second one to add to it
// (or null).  Launch plan:
//   cs in the CRT basis   sk_eval over all ncs components -> crtInv -> lInv
//   powerful, ncs = 1     lInv (m = 2^k: nothing; the lift reads c_0 itself)
//   powerful, ncs >= 2    crt of c_1.. (one batched launch) -> sk_eval (times s) -> crtInv, then c_0 joins:
//                         m = 2^k: inside the lift (L = id);  otherwise one add pass, then lInv.  Adding before lInv
//                         costs one pass over two slabs; transforming c_0 as well would cost a crt of one more slab.
int eval_dec(const Plan& P, hipStream_t s, const int64_t* cs, int ncs, bool cs_crt, const int64_t* s_crt, int64_t* work,
             int64_t B, const int64_t** v, const int64_t** add) {
  const size_t slab = (size_t)(B * P.n * P.T);
  const bool l_id = P.prog_linv.stages.empty();
  *add = nullptr;
  *v = work;
  int rc = LOLHIP_OK;
  if (cs_crt) {
    if (launch_sk_eval(s, cs, ncs, false, s_crt, work, B, P.n, P.T, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
    rc = do_crt(P, s, work, B, true);
    return rc ? rc : run_prog_or_copy(P, P.prog_linv, s, work, B, nullptr);
  }
  if (ncs == 1) {
    if (l_id) { *v = cs; return LOLHIP_OK; }
    return run_prog(P, P.prog_linv, s, work, B, cs);
  }
  if (hipMemcpyAsync(work, cs + slab, sizeof(int64_t) * slab * (size_t)(ncs - 1), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return LOLHIP_ERR_HIP;
  rc = do_crt(P, s, work, B * (ncs - 1), false);
  if (rc) return rc;
  if (launch_sk_eval(s, work, ncs - 1, true, s_crt, work, B, P.n, P.T, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  rc = do_crt(P, s, work, B, true);
  if (rc) return rc;
  if (l_id) { *add = cs; return LOLHIP_OK; }
  if (launch_addmod(s, work, cs, B, P.n, P.T, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  return run_prog(P, P.prog_linv, s, work, B, nullptr);
}

// work: the q side of eval_dec [max(ncs - 1, 1)][B][n'][T] | e [B][n'] residues mod p (decrypt only)
struct DecWork { int64_t *q, *e; };
DecWork dec_work(Work& w, const Plan& P, int ncs, int64_t B) {
  return {w.take((int64_t)(ncs > 2 ? ncs - 1 : 1) * B * P.n * P.T), w.take(B * P.n)};
}

}  // namespace

extern "C" {

int64_t lolhip_decrypt_work_len(const lolhip_plan* pq, int ncs, int64_t B) {
  if (!pq || ncs < 1 || B < 0) return LOLHIP_ERR_INVALID;
  return measure(dec_work, pq->P, ncs, B);
}

int lolhip_error_term_batch(const lolhip_plan* pq, void* stream, const int64_t* cs, int ncs, int cs_crt,
                            const int64_t* s_crt, int enc, int64_t p, int64_t* e_dec, int64_t* work, int64_t B) {
  int rc = need_device(pq); if (rc) return rc;
  const Plan& P = pq->P;
  LiftParams lp;
  rc = decrypt_setup(P, ncs, enc, p, 1, lp); if (rc) return rc;
  if (B < 0 || (B > 0 && (!cs || !s_crt || !e_dec || !work))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t *v, *add;
  rc = eval_dec(P, s, cs, ncs, cs_crt != 0, s_crt, work, B, &v, &add); if (rc) return rc;       // work: the q side alone
  return hip_status(launch_lift(s, v, add, e_dec, B * P.n, lp, false, P.d_lift, P.d_mod));
}

// decrypt = l' * twace (divG^k (reduce_p e)): the lift writes l' * reduce_p e (decoding basis of R'_p, l' folded in:
// every later step is Z_p-linear), then divGDec k times and twacePowDec over the p plans, and L into the powerful basis
int lolhip_decrypt_batch(const lolhip_plan* pq, const lolhip_plan* pp, const lolhip_ext* x_p, void* stream,
                         const int64_t* cs, int ncs, int cs_crt, const int64_t* s_crt, int enc, int64_t k, int64_t l,
                         int64_t* pt_pow, int64_t* work, int64_t B) {
  int rc = need_device(pq); if (rc) return rc;
  if (!pp) return LOLHIP_ERR_INVALID;
  rc = need_device(pp); if (rc) return rc;
  const Plan &P = pq->P, &PP = pp->P;
  if (PP.T != 1 || PP.m != P.m || k < 0) return LOLHIP_ERR_INVALID;
  const Plan* PM = &PP;                                       // the plan of the output ring R_m over p
  if (x_p) {
    const ExtPlan& X = x_p->X;
    if (X.hi->m != PP.m || X.hi->qs != PP.qs) return LOLHIP_ERR_INVALID;
    if (!X.d_twace_powdec) return LOLHIP_ERR_NO_DEVICE;
    PM = X.lo;
  }
  LiftParams lp;
  rc = decrypt_setup(P, ncs, enc, (int64_t)PP.qs[0], l, lp); if (rc) return rc;
  if (k > 0 && !divg_ok(PP)) return LOLHIP_ERR_NOT_DIVISIBLE;
  if (B < 0 || (B > 0 && (!cs || !s_crt || !pt_pow || !work))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t *v, *add;
  Work w(work);
  const auto [q, e] = dec_work(w, P, ncs, B);
  rc = eval_dec(P, s, cs, ncs, cs_crt != 0, s_crt, q, B, &v, &add); if (rc) return rc;
  if (launch_lift(s, v, add, e, B * P.n, lp, true, P.d_lift, P.d_mod) != hipSuccess) return LOLHIP_ERR_HIP;
  for (int64_t i = 0; i < k; ++i) {
    rc = run_prog(PP, PP.prog_ginvdec, s, e, B, nullptr); if (rc) return rc;
  }
  if (x_p) {
    rc = lolhip_twace_powdec_batch(x_p, stream, pt_pow, e, B); if (rc) return rc;
    return run_prog_or_copy(*PM, PM->prog_l, s, pt_pow, B, nullptr);
  }
  return run_prog_or_copy(PP, PP.prog_l, s, pt_pow, B, e);
}

}  // extern "C"
