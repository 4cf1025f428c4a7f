// Spline-coupling kernels for hidden tiles HT = 2, runtime d <= 8: spline_pick (nfx_spline_kernel.h)
// lists the shapes.
#include "nfx_spline_kernel.h"

namespace nfx {
template <> spline_kernel_t spline_pick_ht<2, 0>(int K, int dir, bool logp) { return spline_pick<2, 0>(K, dir, logp); }
}  // namespace nfx
