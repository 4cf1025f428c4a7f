// Wide spline-coupling kernels (8 < d <= 64) for hidden tiles HT = 4: spline_wide_pick
// (nfx_spline_kernel.h) lists the shapes.
#include "nfx_spline_kernel.h"

namespace nfx {
template <> spline_kernel_t spline_wide_pick_ht<4>(int K, int dir, bool logp) { return spline_wide_pick<4>(K, dir, logp); }
}  // namespace nfx
