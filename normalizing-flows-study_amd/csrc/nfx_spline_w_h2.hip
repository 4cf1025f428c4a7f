// Wide spline-coupling kernels (8 < d <= 64) for hidden tiles HT = 2: spline_wide_pick
// (nfx_spline_kernel.h) lists the shapes.
#include "nfx_spline_kernel.h"

namespace nfx {
template <> spline_kernel_t spline_wide_pick_ht<2>(int K, int dir, bool logp) { return spline_wide_pick<2>(K, dir, logp); }
}  // namespace nfx
