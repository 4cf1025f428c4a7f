// Spline-coupling kernels for hidden tiles HT = 3, runtime d <= 8: spline_pick (nfx_spline_kernel.h)
// lists the shapes.
#include "nfx_spline_kernel.h"

namespace nfx {
template <> spline_kernel_t spline_pick_ht<3, 0>(int K, int dir, bool logp) { return spline_pick<3, 0>(K, dir, logp); }
}  // namespace nfx
