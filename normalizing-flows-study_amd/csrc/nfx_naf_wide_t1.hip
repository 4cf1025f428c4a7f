// NeuralAutoregressiveFlow wide kernel, 1 out tile(s) per wave (one translation unit per count).
#include "nfx_naf_wide_kernel.h"

namespace nfx {
template <> naf_wide_kernel_t naf_wide_pick<1>() { return naf_wide_kernel<1>; }
}  // namespace nfx
