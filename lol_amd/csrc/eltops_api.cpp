// lol_amd/csrc/eltops_api.cpp — the C ABI of L, L^-1, mulG and divG over Z, R and C and of mulC (include/lolhip.h;
// tensorL{R,Double,C}, tensorLInv*, tensorG{Pow,Dec}{R,C}, tensorGInv{Pow,Dec}{R,C} and mulC of the reference's backend,
// Backend.hs:304-337): host checks, the route rule and the launches of eltops.hip.
#include <hip/hip_runtime_api.h>

#include "eltops.h"
#include "she_host.h"

using namespace lolhip;

extern "C" {

int lolhip_elt_op_batch(const lolhip_plan* p, void* stream, int op, int elt, int T, void* y, int32_t* ok, int64_t B) {
  if (!p || op < LOLHIP_OP_L || op > LOLHIP_OP_DIVGDEC || elt < LOLHIP_ELT_I64 || elt > LOLHIP_ELT_C64) return LOLHIP_ERR_INVALID;
  const Plan& P = p->P;
  if (T < 1 || T > ELT_MAX_T || B < 0 || P.n > ELT_MAX_N) return LOLHIP_ERR_INVALID;
  const int rc = need_device(p); if (rc) return rc;
  const bool divi = elt == LOLHIP_ELT_I64 && (op == LOLHIP_OP_DIVGPOW || op == LOLHIP_OP_DIVGDEC);
  if (B > 0 && (!y || (divi && !ok))) return LOLHIP_ERR_INVALID;
  if (B == 0) return LOLHIP_OK;

  hipStream_t s = (hipStream_t)stream;
  EltLaunch a;
  a.stream = s; a.y = y; a.ok = ok; a.B = B; a.n = P.n;
  a.W = elt == LOLHIP_ELT_C64 ? 2 * T : T;
  a.f64 = elt != LOLHIP_ELT_I64;
  a.op = op - LOLHIP_OP_L;
  a.nd = norm_dims(P);
  a.oddrad = 1;
  for (const PP& pe : P.pps) if (pe.p != 2) a.oddrad *= pe.p;
  if (a.nd.k == 0)                       // m = 2^k: every map is the identity
    return divi ? hip_status(launch_elt_ok(s, ok, B)) : LOLHIP_OK;
  // the route is a function of (n, T, elt) alone
  a.global = sw(SW_ELT_GLOBAL) || !elt_fits_lds(P.n, a.W);
  return hip_status(launch_elt(a));
}

int lolhip_mulc_batch(void* stream, double* a, const double* b, int64_t count) {
  if (count < 0) return LOLHIP_ERR_INVALID;
  int devs = 0;
  if (hipGetDeviceCount(&devs) != hipSuccess || devs == 0) return LOLHIP_ERR_NO_DEVICE;
  if (count > 0 && (!a || !b)) return LOLHIP_ERR_INVALID;
  return hip_status(launch_mulc((hipStream_t)stream, a, b, count));
}

}  // extern "C"
