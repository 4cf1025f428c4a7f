// Streaming spline chain kernels for hidden tiles HT = 2: spline_schain_pick
// (nfx_spline_schain_kernel.h) lists the shapes.
#include "nfx_spline_schain_kernel.h"

namespace nfx {
template <>
spline_schain_t spline_schain_pick_ht<2>(int K, int dir, bool logp, bool small) {
    return spline_schain_pick<2>(K, dir, logp, small);
}
}  // namespace nfx
