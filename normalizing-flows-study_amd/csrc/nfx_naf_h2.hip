// NeuralAutoregressiveFlow kernel, widest hidden layer padded to 64 (one translation unit per padded width).
#include "nfx_naf_kernel.h"

namespace nfx {
template <> naf_kernel_t naf_pick_ht<2>() { return naf_kernel<2>; }
}  // namespace nfx
