// ResidualFlow backward kernels, padded width 64 (one translation unit per padded width).
#include "nfx_residual_bwd_kernel.h"

namespace nfx {
template <> residual_bwd_kernel_t res_bwd_pick_ht<2>(int d) { return res_bwd_pick<2>(d); }
}  // namespace nfx
