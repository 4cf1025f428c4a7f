// Spline-coupling kernels for hidden tiles HT = 2, compile-time d = 2: spline_pick (nfx_spline_kernel.h)
// lists the shapes.
#include "nfx_spline_kernel.h"

namespace nfx {
template <> spline_kernel_t spline_pick_ht<2, 2>(int K, int dir, bool logp) { return spline_pick<2, 2>(K, dir, logp); }
}  // namespace nfx
