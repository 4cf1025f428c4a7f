// ResidualFlow kernels, padded hidden width 32 (one translation unit per padded width).
#include "nfx_residual_kernel.h"

namespace nfx {
template <> residual_kernel_t res_pick_ht<1>(int d) { return res_pick<1>(d); }
}  // namespace nfx
