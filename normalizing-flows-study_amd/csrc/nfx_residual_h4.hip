// ResidualFlow kernels, padded hidden width 128 (one translation unit per padded width).
#include "nfx_residual_kernel.h"

namespace nfx {
template <> residual_kernel_t res_pick_ht<4>(int d) { return res_pick<4>(d); }
}  // namespace nfx
