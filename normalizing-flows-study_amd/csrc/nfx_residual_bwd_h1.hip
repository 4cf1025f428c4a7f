// ResidualFlow backward kernels, padded width 32 (one translation unit per padded width).
#include "nfx_residual_bwd_kernel.h"

namespace nfx {
template <> residual_bwd_kernel_t res_bwd_pick_ht<1>(int d) { return res_bwd_pick<1>(d); }
}  // namespace nfx
