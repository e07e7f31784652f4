// lol_amd/csrc/capi_internal.h — what the host translation units of the C ABI share: the handle types behind
// include/lolhip.h and the launch helpers capi.cpp owns (defined there).  Not part of the public interface.
#pragma once
#include <hip/hip_runtime_api.h>

#include "lolhip.h"
#include "pipeline.h"
#include "plan.h"

struct lolhip_plan { lolhip::Plan P; };
struct lolhip_ext { lolhip::ExtPlan X; };

namespace lolhip {
// LOLHIP_OK, or why the plan cannot compute on the calling thread's current device
int capi_need_device(const lolhip_plan* p);
// y = program(src or y) over B polynomials (the vector interpreter or the scalar one)
int capi_run_prog(const Plan& P, const StageProgram& sp, hipStream_t s, int64_t* y, int64_t B, const int64_t* src);
// crt / crtInv of B polynomials in place, through whichever path the plan has
int capi_do_crt(const Plan& P, hipStream_t s, int64_t* y, int64_t B, bool inverse);
// 1 when divG is possible modulo every q_t of the plan
int capi_divg_ok(const Plan& P);
// digit counts and the invariant-divisor constants of `base` over the plan's moduli (lolhip_decompose_batch's own)
int capi_make_decomp(const Plan& P, int64_t base, DecompParams& d);
}  // namespace lolhip
