// Spline-coupling backward kernels for hidden tiles HT = 2: spline_bwd_pick
// (nfx_spline_bwd_kernel.h) lists the shapes.
#include "nfx_spline_bwd_kernel.h"

namespace nfx {
template <> spline_bwd_kernel_t spline_bwd_pick_ht<2>(int K, int inv) { return spline_bwd_pick<2>(K, inv); }
}  // namespace nfx
