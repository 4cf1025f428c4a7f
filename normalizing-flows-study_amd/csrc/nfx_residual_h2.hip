// ResidualFlow kernels, padded hidden width 64 (one translation unit per padded width).
#include "nfx_residual_kernel.h"

namespace nfx {
template <> residual_kernel_t res_pick_ht<2>(int d) { return res_pick<2>(d); }
}  // namespace nfx
