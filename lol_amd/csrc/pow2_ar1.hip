// lol_amd/csrc/pow2_ar1.hip — the m = 2^k kernels of arithmetic class AR = 1 (see pow2_impl.h)
#include "pow2_impl.h"
namespace lolhip {
template hipError_t launch_pow2_ar<1, false>(const Pow2Launch&, int);
}  // namespace lolhip
