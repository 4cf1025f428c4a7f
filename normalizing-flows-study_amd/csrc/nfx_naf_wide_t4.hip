// NeuralAutoregressiveFlow wide kernel, 4 out tile(s) per wave (one translation unit per count).
#include "nfx_naf_wide_kernel.h"

namespace nfx {
template <> naf_wide_kernel_t naf_wide_pick<4>() { return naf_wide_kernel<4>; }
}  // namespace nfx
